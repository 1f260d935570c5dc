"""GPU tests of the P2 epsilon kernels with a P2 viscosity (include/hyteg_hip.h section b-4 (P2 epsilon)) through the C-ABI on the
macro-cell of tet_1el, entry by entry against the numpy restatement of tests/p2epsilonutil.py (pinned by
tests/test_p2_epsilon_reference.py).  Criteria, those of tests/test_gpu_p2_divkgrad.py: relative L2 <= 1e-12 and max entry error
<= 1e-12 * max|dst|; entries outside a component's point-class mask and the kind mask are bit-identical to the sentinel the destination
was filled with.  Every case runs through both forms: the shipped dispatch with the inner form from level 2, and the gather form on
every DoF."""
import functools

import numpy as np
import pytest

import gmgutil
import p2divkgradutil as pu
import p2epsilonutil as pe

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
    before = capi.p2_elementwise_epsilon_set_inner_min_level(2)  # the inner form wherever it exists, whatever level ships it
    yield torch, capi
    capi.p2_elementwise_epsilon_set_inner_min_level(before)


def _dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to("cuda")  # a copy: the shared cases are read-only arrays


def sentinel(level):
    n = pu.size(level)
    return 7.0 + 3.0 * np.sin(0.37 * np.arange(3 * n)).reshape(3, n)


@functools.lru_cache(maxsize=None)
def case(level):
    """src (3, n) in [-1, 1], mu in [0.5, 2] on the DoF vector, the restatement matrix: computed once per level, read-only"""
    rng = np.random.default_rng(400 + level)
    n = pu.size(level)
    src, mu = rng.uniform(-1.0, 1.0, (3, n)), rng.uniform(0.5, 2.0, n)
    A = pe.cell_matrix(mu, tet(), level)
    ref = (A @ src.reshape(3 * n)).reshape(3, n)
    for a in (src, mu, ref):
        a.setflags(write=False)
    return src, mu, A, ref


def check(got, expected, sel, filled):
    """selected entries against the restatement, the others against the sentinel, bit by bit"""
    assert np.array_equal(got[~sel], filled[~sel]), "entries outside the masks were written"
    if not sel.any():
        return
    scale = np.abs(expected[sel]).max()
    err = np.abs(got[sel] - expected[sel])
    assert err.max() <= TOL * scale, (err.max(), scale)
    assert np.linalg.norm(err) <= TOL * np.linalg.norm(expected[sel])


class Arrays:
    """device copies of (3, n) component vectors and of the viscosity, split into vertex and edge arrays (named: temporaries' memory
    would be reused)"""

    def __init__(self, torch, level, dst, src, mu):
        nv = pu.vertex_size(level)
        self.torch = torch
        self.dv, self.de = [_dev(torch, dst[k][:nv]) for k in range(3)], [_dev(torch, dst[k][nv:]) for k in range(3)]
        self.sv, self.se = [_dev(torch, src[k][:nv]) for k in range(3)], [_dev(torch, src[k][nv:]) for k in range(3)]
        self.mv, self.me = _dev(torch, mu[:nv]), _dev(torch, mu[nv:])

    @staticmethod
    def ptrs(arrays):
        return [a.data_ptr() for a in arrays]

    def result(self):
        self.torch.cuda.synchronize()
        return np.stack([np.concatenate([self.dv[k].cpu().numpy(), self.de[k].cpu().numpy()]) for k in range(3)])


def run_apply(torch, capi, level, form, mask=pu.MASK_ALL, kinds=0xFF, update=0, alpha=1.0, src=None):
    s, mu, _, ref = case(level)
    if src is not None:
        s, ref = src
    filled = sentinel(level)
    a = Arrays(torch, level, filled, s, mu)
    geometry = capi.p2_elementwise_epsilon_geometry(tet(), level)
    capi.p2_elementwise_epsilon_apply_cell(a.ptrs(a.dv), a.ptrs(a.de), a.ptrs(a.sv), a.ptrs(a.se), a.mv.data_ptr(), a.me.data_ptr(), level,
                                           geometry, alpha, update, mask, kinds, gather=form == "gather")
    got = a.result()
    expected = alpha * ref + filled if update == capi.ADD else alpha * ref
    check(got, expected, pe.dof_masks(level, mask, kinds), filled)
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


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_a_mask_that_differs_on_one_component(env, level, form):
    """the components of a velocity may carry different boundary conditions: a component whose mask excludes a DoF keeps its sentinel
    there, the others are written"""
    torch, capi = env
    face = 1 << 6  # one macro-face
    for masks in ([pu.MASK_INNER, pu.MASK_INNER, pu.MASK_ALL], [pu.MASK_ALL, pu.MASK_INNER | face, pu.MASK_ALL], [0, pu.MASK_SHELL, 0],
                  [pu.MASK_INNER, 0, pu.MASK_SHELL]):
        run_apply(torch, capi, level, form, mask=masks)
        run_apply(torch, capi, level, form, mask=masks, update=capi.ADD, alpha=-0.75, kinds=0x5B)


@pytest.mark.parametrize("level", LEVELS)
def test_diagonals_of_the_three_diagonal_blocks(env, level):
    """component i of every DoF receives the sum of A_e^{ii}[row][row] over its adjacent micro-cells"""
    torch, capi = env
    _, mu, A, _ = case(level)
    n = pu.size(level)
    filled = sentinel(level)
    a = Arrays(torch, level, filled, filled, mu)
    capi.p2_elementwise_epsilon_diagonal_cell(a.ptrs(a.dv), a.ptrs(a.de), a.mv.data_ptr(), a.me.data_ptr(), level,
                                              capi.p2_elementwise_epsilon_geometry(tet(), level))
    got = a.result()
    want = A.diagonal().reshape(3, n)
    for k in range(3):
        check(got[k], want[k], np.ones(n, dtype=bool), filled[k])
    assert not np.array_equal(want[0], want[1])  # the three differ: d_i phi d_i phi


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("level", LEVELS)
def test_rigid_rotation_gives_zero(env, level, form):
    """u = omega x ( x - x0 ) has no strain: | A u | <= 1e-12 * max mu * max | u | * max | int_e phi_m ( ... ) |, the scale of the terms
    that cancel"""
    torch, capi = env
    _, mu, _, _ = case(level)
    x = pu.dof_points(tet(), level)
    omega, x0 = np.array([0.3, -1.1, 0.7]), np.array([0.2, 0.1, -0.4])
    u = np.cross(omega, x - x0).T.copy()
    filled = sentinel(level)
    a = Arrays(torch, level, filled, u, mu)
    capi.p2_elementwise_epsilon_apply_cell(a.ptrs(a.dv), a.ptrs(a.de), a.ptrs(a.sv), a.ptrs(a.se), a.mv.data_ptr(), a.me.data_ptr(), level,
                                           capi.p2_elementwise_epsilon_geometry(tet(), level), gather=form == "gather")
    got = a.result()
    assert np.abs(got).max() <= 1e-12 * mu.max() * np.abs(u).max() * pe.max_entry(tet(), level)


def _check_inner_form_equals_gather_form(env, level):
    torch, capi = env
    rng = np.random.default_rng(level)
    n = pu.size(level)
    src, mu = rng.standard_normal((3, n)), rng.uniform(0.5, 2.0, n)
    geometry = capi.p2_elementwise_epsilon_geometry(tet(), level)
    filled = np.stack([np.full(n, 0.25), np.full(n, -0.5), np.full(n, 1.75)])
    for mask, update in ((pu.MASK_ALL, 0), (pu.MASK_ALL, 1), ([pu.MASK_INNER, pu.MASK_ALL, pu.MASK_INNER], 0)):
        out = {}
        for gather in (False, True):
            a = Arrays(torch, level, filled, src, mu)
            capi.p2_elementwise_epsilon_apply_cell(a.ptrs(a.dv), a.ptrs(a.de), a.ptrs(a.sv), a.ptrs(a.se), a.mv.data_ptr(), a.me.data_ptr(), level,
                                                   geometry, 1.0, update, mask, 0xFF, gather=gather)
            out[gather] = a.result()
        scale = np.abs(out[True]).max()
        assert np.abs(out[False] - out[True]).max() <= 1e-13 * scale, (hex(mask) if isinstance(mask, int) else mask, update)
        assert np.array_equal(out[False] == filled, out[True] == filled)  # untouched entries are untouched in both
        if update == 0:  # exactly the DoFs of the masks were written
            assert np.array_equal(out[False] != filled, pe.dof_masks(level, mask))


def test_inner_form_equals_gather_form_at_level_5(env):
    """a level the restatement is not run at.  The two forms differ in the order of the micro-cells only: max difference
    <= 1e-13 * max|dst|, the bound of tests/test_gpu_p2_divkgrad.py for form against form"""
    _check_inner_form_equals_gather_form(env, 5)


def test_inner_form_equals_gather_form_at_level_6(env):
    """the one-lane gather form: level 6 is the smallest level at which "every DoF" is dispatched with one lane per DoF (47,905 vertex
    and about 318,000 edge entries per component).  Same cases and bound as at level 5; the parent commit holds 1e-13
    (profiles/p2_varcoef_checks.txt)"""
    _check_inner_form_equals_gather_form(env, 6)
