"""P1toP1QuadraticProlongationThroughP2Injection on the GPU: the reference's VertexDoFQuadraticProlongation3DTest.cpp:47-151 on its
3-D meshes with lower level 3 -- constants, linears and a quadratic are prolongated exactly -- plus what the host layer promises
on top: the copies of a shared DoF stay bit-identical, and the call is exactly P1toP2Conversion, P2toP2QuadraticProlongation,
P2toP1Conversion."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
MESHES = ROOT / "hyteg_amd" / "data" / "meshes"
LOWER = 3

FUNCTIONS = {
    "zero": lambda x, y, z: 0.0 * x,
    "one": lambda x, y, z: 1.0 + 0.0 * x,
    "constant": lambda x, y, z: 42.0 + 0.0 * x,
    "linear in x": lambda x, y, z: 42.0 * x,
    "linear in x and y": lambda x, y, z: 42.0 * x + y,
    "quadratic": lambda x, y, z: 2.0 * x * x + 3.0 * x + 13.0 + 4.0 * y + 5.0 * y * y + z * z + 6.0,
}


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, capi, host, hu


@pytest.mark.parametrize("mesh", ["tet_1el", "pyramid_2el", "pyramid_4el", "pyramid_tilted_4el", "regular_octahedron_8el"])
def test_reference_checks_and_shared_copies(env, mesh):
    torch, capi, host, hu = env
    st = host.Storage.from_gmsh(MESHES / f"{mesh}.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    orc = hu.MultiCellOracle(st)
    flag = host.Inner | host.NeumannBoundary
    u, exact, err, full = (host.P1Function(st, n, LOWER, LOWER + 1) for n in ("u", "u_exact", "err", "full"))
    prolongation = host.P1QuadraticProlongation(st, LOWER, LOWER + 1)
    plans = [st.plan(LOWER + 1, cls) for cls in (0, 1)]  # the groups of copies of the inner and of the boundary DoFs
    for name, fn in FUNCTIONS.items():
        hu.upload(u, orc.interpolate(fn, LOWER), LOWER)
        hu.upload(full, orc.interpolate(fn, LOWER + 1), LOWER + 1)
        exact.assign([1.0], [full], LOWER + 1, flag)  # resultExact.interpolate( uFunction, lowerLevel + 1, Inner | NeumannBoundary )
        prolongation.prolongate(u, LOWER, flag)
        err.assign([1.0, -1.0], [u, exact], LOWER + 1, flag)
        e2, scale = err.dot(err, LOWER + 1, flag), exact.dot(exact, LOWER + 1, flag)
        print(f"{mesh}: u {name}: squared error {e2:.3e}, |exact|^2 {scale:.3e}")
        assert e2 <= 1e-26 * max(scale, 1.0), name
        # every copy of a DoF shared between macro-cells holds the same bits
        fine = hu.download(u, LOWER + 1)
        for cls, p in enumerate(plans):
            gp, eb, eo = p["group_ptr"], p["entry_buf"], p["entry_off"]
            for g in range(p["ngroups"]):
                copies = [fine[eb[k]][eo[k]] for k in range(gp[g], gp[g + 1])]
                assert all(c == copies[0] for c in copies), (name, cls, g)
    # the prolongation did something: the last function is not zero inside
    assert max(np.abs(a).max() for a in hu.download(u, LOWER + 1)) > 1.0
    for o in (prolongation, u, exact, err, full, st):
        o.close()


def test_equals_the_three_calls_made_by_hand(env):
    torch, capi, host, hu = env
    st = host.Storage.from_gmsh(MESHES / "tet_1el.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    orc = hu.MultiCellOracle(st)
    flag = host.Inner | host.NeumannBoundary
    fn = lambda x, y, z: np.sin(3.0 * x) * y + np.cosh(z) + x * y * z  # noqa: E731
    a, b = host.P1Function(st, "a", LOWER, LOWER + 1), host.P1Function(st, "b", LOWER, LOWER + 1)
    rng = np.random.default_rng(5)
    junk = [rng.standard_normal(capi.cell_size(LOWER + 1))]
    for f in (a, b):
        hu.upload(f, orc.interpolate(fn, LOWER), LOWER)
        hu.upload(f, junk, LOWER + 1)
    host.prolongate_quadratic(a, LOWER, flag)
    tmp = host.P2Function(st, "tmp", LOWER - 1, LOWER)
    host.p1_to_p2(b, tmp, LOWER - 1, host.All)
    host.p2_prolongate(tmp, LOWER - 1, flag)
    host.p2_to_p1(tmp, b, LOWER + 1, host.All)
    ga, gb = a.download_cell(0, LOWER + 1), b.download_cell(0, LOWER + 1)
    assert np.array_equal(ga, gb)
    # the last conversion is `All`: the points the flag excludes hold the temporary's zeros, not the previous content
    boundary = ~hu.point_mask(LOWER + 1, st.mask(0, flag))
    assert boundary.any() and np.array_equal(ga[boundary], np.zeros(int(boundary.sum())))
    assert not np.array_equal(ga[~boundary], junk[0][~boundary])
    # the source level is only read
    assert np.array_equal(a.download_cell(0, LOWER), orc.interpolate(fn, LOWER)[0])
    with pytest.raises(host.HytegHostError, match="p1MinLevel"):
        host.P1QuadraticProlongation(st, 0, 1)
    for o in (tmp, a, b, st):
        o.close()
