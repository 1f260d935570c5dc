"""GPU tests of the fused residual and Chebyshev modes of the variable-coefficient P1 kernels (include/hyteg_hip.h sections b-4 and
b-5: ..._residual_macro_3d, ..._chebyshev_start_macro_3d, ..._chebyshev_step_macro_3d) through the C-ABI, for the epsilon operator
(three components) and div-k-grad (one), on one skew macro-cell.  Entry by entry against ( A src ) of the numpy element loops of
tests/epsilonutil.py / tests/divkgradutil.py (pinned by their own CPU tests) plus the mode's arithmetic (tests/epsilongmgutil.py).
Inputs: every array random in [-1, 1] (inverse diagonals in [0.5, 2]), the coefficient smooth with contrast 20.
Criteria per component at the inner points: relative L2 <= 1e-12 and max entry error <= 1e-12 * max|expected| (the project's fp64
parity bar); every shell entry of every output array is bit-identical to its prior content.  The z-march against the point form:
relative L2 <= 1e-13.  Levels: 2 has a single inner point, 3 has rows shorter than a wave, 4 has bricks with fewer slices than a
brick marches, 6 is the first with several 64-wide x-segments per row and bricks on every XCD slab."""
import functools

import numpy as np
import pytest

import epsilongmgutil as gu
from conftest import SKEW_TET
from divkgradutil import MASK_INNER, cell_size, point_mask

pytestmark = pytest.mark.gpu
TOL = 1e-12
TOL_FORMS = 1e-13
TET = SKEW_TET
LEVELS = (2, 3, 4, 6)
OPS = ("epsilon", "divkgrad")
C_PREV, C_CUR = 0.37, -1.21


@pytest.fixture(scope="module")
def env():
    import torch

    from hyteg_amd import capi

    assert torch.cuda.is_available()
    capi.lib()
    return torch, capi


@functools.lru_cache(maxsize=None)
def case(name, level):
    """the inputs of one operator at one level and ( A src ) of the restatement: computed once, read-only.  src doubles as the x of
    the start and the t_in of the step."""
    nc = 3 if name == "epsilon" else 1
    rng = np.random.default_rng(1300 + 10 * level + nc)
    n = cell_size(level)
    c = {"src": rng.uniform(-1.0, 1.0, (nc, n)), "rhs": rng.uniform(-1.0, 1.0, (nc, n)), "x": rng.uniform(-1.0, 1.0, (nc, n)),
         "invd": rng.uniform(0.5, 2.0, (nc, n)), "coef": gu.smooth_coefficient(TET, level), "sentinel": 7.0 + 3.0 * np.sin(0.37 * np.arange(nc * n)).reshape(nc, n)}
    assert c["coef"].max() / c["coef"].min() >= 10.0
    import epsilonutil as eu
    import divkgradutil as du

    c["A"] = eu.apply_cell(c["src"], c["coef"], TET, level) if nc == 3 else du.apply_cell(c["src"][0], c["coef"], TET, level)[None, :]
    for a in c.values():
        a.setflags(write=False)
    return c


def dev(torch, a):
    """device copies of the rows of a and their pointers"""
    t = [torch.from_numpy(np.array(x, dtype=np.float64)).to("cuda") for x in a]
    return t, [x.data_ptr() for x in t]


def host(t):
    return np.stack([x.cpu().numpy() for x in t])


def check(got, expected, prior, level, tol=TOL, written=None):
    """inner points against `expected`, every other entry (and every entry of a component that is not written) bit-identical to
    `prior`.  Returns the largest relative L2 error of a component."""
    inner = point_mask(level, MASK_INNER)
    worst = 0.0
    for c in range(got.shape[0]):
        if written is not None and not written[c]:
            assert np.array_equal(got[c], prior[c]), f"component {c} is switched off and was written"
            continue
        assert np.array_equal(got[c][~inner], prior[c][~inner]), f"component {c}: a shell entry was written"
        g, e = got[c][inner], expected[c][inner]
        err = np.abs(g - e)
        scale = np.abs(e).max()
        assert scale > 0.0
        assert err.max() <= tol * scale, (c, err.max(), scale)
        rel = np.linalg.norm(err) / np.linalg.norm(e)
        assert rel <= tol, (c, rel)
        worst = max(worst, rel)
    return worst


def run_mode(torch, op, mode, level, has_prev=True, comps=None):
    """one call of one entry on fresh device arrays; returns ( outputs, expected, prior ) as lists with one item per output array"""
    c = case(op.name, level)
    (st, sp), (rt, rp), (it, ip), (ct, cp) = dev(torch, c["src"]), dev(torch, c["rhs"]), dev(torch, c["invd"]), dev(torch, [c["coef"]])
    dt, dp = dev(torch, c["sentinel"])
    if mode == "residual":
        op.residual(dp, sp, rp, cp[0], TET, level, comps=comps)
        torch.cuda.synchronize()
        return [host(dt)], [gu.residual(c["A"], c["rhs"])], [c["sentinel"]]
    if mode == "start":
        op.chebyshev_start(dp, rp, sp, ip, cp[0], TET, level, comps=comps)
        torch.cuda.synchronize()
        return [host(dt)], [gu.chebyshev_start(c["A"], c["rhs"], c["invd"])], [c["sentinel"]]
    xt, xp = dev(torch, c["x"])
    op.chebyshev_step(dp, xp, sp, ip, cp[0], TET, level, C_PREV, C_CUR, has_prev, comps=comps)
    torch.cuda.synchronize()
    t_out, x_new = gu.chebyshev_step(c["A"], c["src"], c["x"], c["invd"], C_PREV, C_CUR, has_prev)
    return [host(dt), host(xt)], [t_out, x_new], [c["sentinel"], c["x"]]


MODES = [("residual", True), ("start", True), ("step", False), ("step", True)]


@pytest.mark.parametrize("mode,has_prev", MODES, ids=["residual", "start", "step-first", "step-prev"])
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", OPS)
def test_entry_against_the_restatement(env, name, level, mode, has_prev):
    torch, capi = env
    op = gu.Operator(capi, name)
    got, expected, prior = run_mode(torch, op, mode, level, has_prev)
    for g, e, p in zip(got, expected, prior):
        print(f"{name} {mode} level {level} has_prev {has_prev}: relative L2 {check(g, e, p, level):.3e}")


@pytest.mark.parametrize("mode,has_prev", MODES, ids=["residual", "start", "step-first", "step-prev"])
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", OPS)
def test_zmarch_against_the_point_form(env, name, level, mode, has_prev):
    """the one-thread-per-point kernel is the second implementation of every mode: same inputs, both at the parity bar against the
    restatement and at 1e-13 against each other"""
    torch, capi = env
    op = gu.Operator(capi, name)
    zm, expected, prior = run_mode(torch, op, mode, level, has_prev)
    try:
        op.set_inner_by_points(True)
        pt, _, _ = run_mode(torch, op, mode, level, has_prev)
    finally:
        op.set_inner_by_points(False)
    for z, p, e, pr in zip(zm, pt, expected, prior):
        check(p, e, pr, level)
        print(f"{name} {mode} level {level}: z-march against point form {check(z, p, pr, level, tol=TOL_FORMS):.3e}")


@pytest.mark.parametrize("mode,has_prev", MODES, ids=["residual", "start", "step-first", "step-prev"])
@pytest.mark.parametrize("name", OPS)
def test_every_brick_shape_gives_the_same_bits(env, name, mode, has_prev):
    """level 6: several bricks per row with every compiled shape.  A shape a mode is not compiled for leaves the mode at its default."""
    torch, capi = env
    op = gu.Operator(capi, name)
    out = []
    try:
        for ny, lz in ((0, 0),) + tuple(op.shapes):
            op.set_shape(ny, lz)
            out.append(run_mode(torch, op, mode, 6, has_prev)[0])
    finally:
        op.set_shape(0, 0)
    for o in out[1:]:
        for a, b in zip(o, out[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("by_points", [False, True], ids=["zmarch", "points"])
@pytest.mark.parametrize("level", [3, 6])
def test_a_component_switched_off_is_not_written(env, level, by_points):
    """comps = 0b101: the arrays of component 1 (t_out and x) keep their bits, the others are computed as before; comps = 0
    launches nothing"""
    torch, capi = env
    op = gu.Operator(capi, "epsilon")
    try:
        op.set_inner_by_points(by_points)
        for mode in ("residual", "start", "step"):
            got, expected, prior = run_mode(torch, op, mode, level, True, comps=0b101)
            for g, e, p in zip(got, expected, prior):
                check(g, e, p, level, written=(True, False, True))
            got, expected, prior = run_mode(torch, op, mode, level, True, comps=0)
            for g, p in zip(got, prior):
                assert np.array_equal(g, p)
    finally:
        op.set_inner_by_points(False)


@pytest.mark.parametrize("name", OPS)
def test_aliasing_is_rejected_without_a_launch(env, name):
    """dst against every input, t_out / x / t_in pairwise, anything against the coefficient: EINVAL, and no array changes"""
    torch, capi = env
    op = gu.Operator(capi, name)
    level = 3
    c = case(name, level)
    arrays = {k: dev(torch, c[k]) for k in ("src", "rhs", "x", "invd", "sentinel")}
    ct, cp = dev(torch, [c["coef"]])
    P = {k: v[1] for k, v in arrays.items()}
    coef, K = cp[0], [cp[0]] * op.nc

    def swapped(ptrs, other):
        """the last component's pointer replaced by the first of `other`"""
        return ptrs[:-1] + [other[0]]

    bad = []
    for other in (P["src"], P["rhs"], K):
        bad.append(lambda o=other: op.residual(swapped(P["sentinel"], o), P["src"], P["rhs"], coef, TET, level))
    bad.append(lambda: op.residual(P["sentinel"], swapped(P["src"], K), P["rhs"], coef, TET, level))
    for other in (P["src"], P["rhs"], P["invd"], K):
        bad.append(lambda o=other: op.chebyshev_start(swapped(P["sentinel"], o), P["rhs"], P["src"], P["invd"], coef, TET, level))
    for other in (P["x"], P["src"], P["invd"], K):
        bad.append(lambda o=other: op.chebyshev_step(swapped(P["sentinel"], o), P["x"], P["src"], P["invd"], coef, TET, level, C_PREV, C_CUR, True))
    for other in (P["src"], P["invd"], K):
        bad.append(lambda o=other: op.chebyshev_step(P["sentinel"], swapped(P["x"], o), P["src"], P["invd"], coef, TET, level, C_PREV, C_CUR, True))
    bad.append(lambda: op.chebyshev_step(P["sentinel"], P["x"], P["src"], swapped(P["invd"], K), coef, TET, level, C_PREV, C_CUR, True))
    if op.nc == 3:  # two components of one written array
        bad.append(lambda: op.residual([P["sentinel"][0], P["sentinel"][1], P["sentinel"][0]], P["src"], P["rhs"], coef, TET, level))
        bad.append(lambda: op.chebyshev_step(P["sentinel"], [P["x"][0], P["x"][0], P["x"][2]], P["src"], P["invd"], coef, TET, level, C_PREV, C_CUR, True))
    for call in bad:
        with pytest.raises(capi.HytegHipError, match=r"code 1\).*alias"):
            call()
    torch.cuda.synchronize()
    for k, (t, _) in arrays.items():
        assert np.array_equal(host(t), c[k]), k
    assert np.array_equal(ct[0].cpu().numpy(), c["coef"])
