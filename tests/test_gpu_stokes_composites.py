"""The two generic Stokes function classes (hyteg_amd/host/stokes.hpp) in both instantiations -- P1-P1 (P1StokesFunction) and
Taylor-Hood (P2 velocity, P1 pressure) -- through the facade, bit for bit, on pyramid_2el at level 2 (the smallest size with
shared primitives):
 * assign on the composite leaves exactly the bits that the same assign on its borrowed component functions leaves;
 * dot is ((du + dv) + dw) + dp of the component functions' own global dot products, the order VectorFunction::dotGlobal and
   StokesFunction::dotGlobal add in;
 * the Taylor-Hood operator's apply leaves in the pressure what its div block alone leaves (x Replace, then y and z Add)."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LEVEL = 2
KINDS = ["P1StokesFunction", "TaylorHoodFunction"]


def _env():
    import torch

    import hostutil as hu
    from hyteg_amd import host

    assert torch.cuda.is_available()
    return host, hu


def _parts(f):
    """the component functions u, v, w, p (borrowed views) of either composite"""
    return list(f.components) if hasattr(f, "components") else list(f.velocity) + [f.pressure]


def _fill(host, st, part, rng):
    for c in range(st.n_local_cells):
        if isinstance(part, host.P2Function):
            nv, ne = part.sizes(LEVEL)
            part.upload(LEVEL, rng.standard_normal(nv), rng.standard_normal(ne), cell=c)
        else:
            part.upload_cell(c, LEVEL, rng.standard_normal(host.cell_size(LEVEL)))


def _arrays(host, st, f):
    """every cell's vertex (and edge) array of every component"""
    out = []
    for part in _parts(f):
        for c in range(st.n_local_cells):
            if isinstance(part, host.P2Function):
                out.extend(part.download(LEVEL, cell=c))
            else:
                out.append(part.download_cell(c, LEVEL))
    return out


def _make(host, hu, kind, names, seed):
    st = host.Storage.from_gmsh(hu.MESHES / "pyramid_2el.msh")
    assert st.n_local_cells == 2
    rng = np.random.default_rng(seed)
    fs = [getattr(host, kind)(st, n, LEVEL, LEVEL) for n in names]
    for f in fs:
        for part in _parts(f):
            _fill(host, st, part, rng)
    return st, fs


@pytest.mark.parametrize("flag_name", ["All", "Inner"])
@pytest.mark.parametrize("kind", KINDS)
def test_assign_equals_assign_on_the_components(kind, flag_name):
    host, hu = _env()
    flag = getattr(host, flag_name)
    st, (f, g, w, w2) = _make(host, hu, kind, ["f", "g", "w", "w2"], 11)
    # w2 starts from w's bits (every array entry, copied through the host), so that what a flag leaves untouched is equal too
    for a, b in zip(_parts(w2), _parts(w)):
        for c in range(st.n_local_cells):
            if isinstance(a, host.P2Function):
                a.upload(LEVEL, *b.download(LEVEL, cell=c), cell=c)
            else:
                a.upload_cell(c, LEVEL, b.download_cell(c, LEVEL))
    before = _arrays(host, st, w)
    assert all(np.array_equal(a, b) for a, b in zip(before, _arrays(host, st, w2)))
    w.assign([2.0, -0.5], [f, g], LEVEL, flag)
    for a, pf, pg in zip(_parts(w2), _parts(f), _parts(g)):
        a.assign([2.0, -0.5], [pf, pg], LEVEL, flag)
    got, want = _arrays(host, st, w), _arrays(host, st, w2)
    assert len(got) == len(want) == (8 if kind == KINDS[0] else 14)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert any(not np.array_equal(a, b) for a, b in zip(got, before))
    for o in (f, g, w, w2, st):
        o.close()


@pytest.mark.parametrize("flag_name", ["All", "Inner"])
@pytest.mark.parametrize("kind", KINDS)
def test_dot_adds_the_component_dots_in_order(kind, flag_name):
    host, hu = _env()
    flag = getattr(host, flag_name)
    st, (f, g) = _make(host, hu, kind, ["f", "g"], 12)
    du, dv, dw, dp = [a.dot(b, LEVEL, flag) for a, b in zip(_parts(f), _parts(g))]
    assert f.dot(g, LEVEL, flag) == ((du + dv) + dw) + dp
    for o in (f, g, st):
        o.close()


def test_taylor_hood_apply_pressure_is_the_div_block():
    host, hu = _env()
    st, (src, dst, dst2) = _make(host, hu, KINDS[1], ["src", "dst", "dst2"], 13)
    op = host.TaylorHoodStokesOperator(st, LEVEL, LEVEL)
    op.apply(src, dst, LEVEL, host.All)
    op.apply_div(src, dst2, LEVEL, host.All)
    for c in range(st.n_local_cells):
        assert np.array_equal(dst.pressure.download_cell(c, LEVEL), dst2.pressure.download_cell(c, LEVEL))
    for o in (src, dst, dst2, op, st):
        o.close()
