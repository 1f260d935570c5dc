"""GPU tests of the P2 div-k-grad kernels with a P2 coefficient (include/hyteg_hip.h section b-4 (P2)) through the C-ABI on the macro-cell
of tet_1el, entry by entry against the numpy restatement of tests/p2divkgradutil.py (pinned by tests/test_p2_divkgrad_reference.py).
Criteria: relative L2 <= 1e-12 and max entry error <= 1e-12 * max|dst| (the project's fp64 parity bar, as tests/test_gpu_divkgrad.py);
entries outside the point-class mask and the kind mask are bit-identical to the sentinel the destination was filled with.
Every case runs through both forms: the shipped dispatch with the inner form from level 2, and the gather form on every DoF."""
import functools

import numpy as np
import pytest

import gmgutil
import p2divkgradutil as pu

pytestmark = pytest.mark.gpu
TOL = 1e-12
LEVELS = range(5)
FORMS = ["inner", "gather"]


@functools.lru_cache(maxsize=None)
def tet():
    v, c = gmgutil.mesh("tet_1el")
    return tuple(map(tuple, np.asarray(v, dtype=np.float64)[np.asarray(c)[0]]))


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi

    assert torch.cuda.is_available()
    capi.lib()
    before = capi.p2_elementwise_divkgrad_set_inner_min_level(2)  # the inner form wherever it exists, whatever level ships it
    yield torch, capi
    capi.p2_elementwise_divkgrad_set_inner_min_level(before)


def _dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")  # a copy: the shared cases are read-only arrays


def sentinel(n):
    return 7.0 + 3.0 * np.sin(0.37 * np.arange(n))


@functools.lru_cache(maxsize=None)
def case(level):
    """src in [-1, 1], k in [0.5, 2] on the DoF vector, the geometry-independent restatement matrix: computed once per level, read-only"""
    rng = np.random.default_rng(300 + level)
    n = pu.size(level)
    src, k = rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 2.0, n)
    A = pu.cell_matrix(k, tet(), level)
    ref = A @ src
    for a in (src, k, ref):
        a.setflags(write=False)
    return src, k, A, ref


def split(level, vec):
    nv = pu.vertex_size(level)
    return vec[:nv], vec[nv:]


def check(got, expected, sel, filled):
    """selected entries against the restatement, the others against the sentinel, bit by bit"""
    assert np.array_equal(got[~sel], filled[~sel]), "entries outside the masks were written"
    if not sel.any():
        return
    scale = np.abs(expected[sel]).max()
    err = np.abs(got[sel] - expected[sel])
    assert err.max() <= TOL * scale, (err.max(), scale)
    assert np.linalg.norm(err) <= TOL * np.linalg.norm(expected[sel])


def run_apply(torch, capi, level, form, mask=pu.MASK_ALL, kinds=0xFF, update=0, alpha=1.0, src=None):
    s, k, _, ref = case(level)
    if src is not None:
        s, ref = src
    filled = sentinel(pu.size(level))
    arrays = [_dev(torch, part) for vec in (filled, s, k) for part in split(level, vec)]  # named: temporaries' memory would be reused
    geometry = capi.p2_elementwise_divkgrad_geometry(tet(), level)
    capi.p2_elementwise_divkgrad_apply_cell(*[a.data_ptr() for a in arrays], level, geometry, alpha, update, mask, kinds, gather=form == "gather")
    torch.cuda.synchronize()
    got = np.concatenate([arrays[0].cpu().numpy(), arrays[1].cpu().numpy()])
    expected = alpha * ref + filled if update == capi.ADD else alpha * ref
    check(got, expected, pu.dof_mask(level, mask, kinds), filled)
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("update,alpha", [("replace", 1.0), ("add", 1.0), ("replace", -0.75), ("add", 2.5)])
@pytest.mark.parametrize("level", LEVELS)
def test_apply_replace_add_and_alpha(env, level, update, alpha, form):
    torch, capi = env
    run_apply(torch, capi, level, form, update=capi.ADD if update == "add" else capi.REPLACE, alpha=alpha)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_every_single_point_class(env, level, form):
    torch, capi = env
    for cls in range(15):
        run_apply(torch, capi, level, form, mask=1 << cls, update=capi.ADD if cls % 2 else capi.REPLACE, alpha=1.5)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_every_single_kind(env, level, form):
    torch, capi = env
    for kind in range(8):
        run_apply(torch, capi, level, form, kinds=1 << kind)
        run_apply(torch, capi, level, form, kinds=1 << kind, mask=pu.MASK_SHELL, update=capi.ADD)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_inner_only_and_shell_only_masks(env, level, form):
    torch, capi = env
    run_apply(torch, capi, level, form, mask=pu.MASK_INNER)
    run_apply(torch, capi, level, form, mask=pu.MASK_INNER, update=capi.ADD, alpha=-2.0, kinds=0xA5)
    run_apply(torch, capi, level, form, mask=pu.MASK_SHELL)


@pytest.mark.parametrize("level", LEVELS)
def test_diagonal(env, level):
    """every DoF receives the sum of A_e[i][i] over its adjacent micro-cells"""
    torch, capi = env
    _, k, A, _ = case(level)
    filled = sentinel(pu.size(level))
    arrays = [_dev(torch, part) for vec in (filled, k) for part in split(level, vec)]
    capi.p2_elementwise_divkgrad_diagonal_cell(*[a.data_ptr() for a in arrays], level, capi.p2_elementwise_divkgrad_geometry(tet(), level))
    torch.cuda.synchronize()
    got = np.concatenate([arrays[0].cpu().numpy(), arrays[1].cpu().numpy()])
    check(got, A.diagonal(), np.ones(len(got), dtype=bool), filled)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_constant_source_gives_zero(env, level, form):
    """rows sum to zero: | A 1 | <= 1e-12 * max k * max | A_e |, A_e the element matrices with k = 1"""
    torch, capi = env
    _, k, _, _ = case(level)
    n = pu.size(level)
    filled = sentinel(n)
    arrays = [_dev(torch, part) for vec in (filled, np.full(n, 3.0), k) for part in split(level, vec)]
    capi.p2_elementwise_divkgrad_apply_cell(*[a.data_ptr() for a in arrays], level, capi.p2_elementwise_divkgrad_geometry(tet(), level),
                                            gather=form == "gather")
    torch.cuda.synchronize()
    got = np.concatenate([arrays[0].cpu().numpy(), arrays[1].cpu().numpy()])
    laplace = np.abs(pu.type_tensors(tet(), level)[0].sum(axis=1)).max()
    assert np.abs(got).max() <= 1e-12 * k.max() * laplace * 3.0  # the source is the constant 3


def _check_inner_form_equals_gather_form(env, level):
    torch, capi = env
    rng = np.random.default_rng(level)
    nv, ne = pu.vertex_size(level), pu.edge_size(level)
    sv, se, kv, ke = (_dev(torch, a) for a in (rng.standard_normal(nv), rng.standard_normal(ne), rng.uniform(0.5, 2.0, nv), rng.uniform(0.5, 2.0, ne)))
    geometry = capi.p2_elementwise_divkgrad_geometry(tet(), level)
    for mask, update in ((pu.MASK_ALL, 0), (pu.MASK_ALL, 1), (pu.MASK_INNER, 0)):
        out = {}
        for gather in (False, True):
            dv, de = torch.full((nv,), 0.25, dtype=torch.float64, device="cuda"), torch.full((ne,), -0.5, dtype=torch.float64, device="cuda")
            capi.p2_elementwise_divkgrad_apply_cell(dv.data_ptr(), de.data_ptr(), sv.data_ptr(), se.data_ptr(), kv.data_ptr(), ke.data_ptr(), level,
                                                    geometry, 1.0, update, mask, 0xFF, gather=gather)
            torch.cuda.synchronize()
            out[gather] = (dv.cpu().numpy(), de.cpu().numpy())
        (av, ae), (bv, be) = out[False], out[True]
        scale = max(np.abs(av).max(), np.abs(ae).max())
        assert np.abs(av - bv).max() <= 1e-13 * scale and np.abs(ae - be).max() <= 1e-13 * scale, (level, hex(mask), update)
        assert np.array_equal(av == 0.25, bv == 0.25) and np.array_equal(ae == -0.5, be == -0.5)  # untouched entries are untouched in both
        if update == 0:  # exactly the DoFs of the mask were written
            assert np.array_equal(np.concatenate([av != 0.25, ae != -0.5]), pu.dof_mask(level, mask))


@pytest.mark.parametrize("level", [5, 6])
def test_inner_form_equals_gather_form(env, level):
    """levels the restatement is not run at; level 6 has rows longer than a wave.  The two forms differ in the order of the micro-cells
    only: max difference <= 1e-13 * max|dst|, the bound of tests/test_gpu_p2_class_rows.py for two P2 kernels with different partial sums"""
    _check_inner_form_equals_gather_form(env, level)


def test_inner_form_equals_gather_form_at_level_6(env):
    """the one-lane gather form: level 6 is the smallest level at which "every DoF" is dispatched with one lane per DoF (47,905 vertex
    and about 318,000 edge entries).  Same cases and bound as above; the parent commit holds 1e-13 (profiles/p2_varcoef_checks.txt)"""
    _check_inner_form_equals_gather_form(env, 6)
