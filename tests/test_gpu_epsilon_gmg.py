"""GPU tests of the multigrid cycle on the epsilon operator through hyteg_amd/host.py: the fused residual and Chebyshev steps of
P1ElementwiseAffineEpsilonOperator and P1ElementwiseDivKGrad against their composed sequences (1e-13, the bar of the existing
fused-against-composed tests), and residual, smoother calls, cycle iterates and residual reductions against the global restatement
of tests/epsilongmgutil.py (pinned and measured by tests/test_epsilon_gmg_restatement.py).  Bound of every comparison with the
restatement: gmgutil.tolerance( d ) = 1e-12 + 50 d with d the difference between the float64 and the 80-bit run of the restated
case; nothing is calibrated on a GPU result.  Meshes: cube_6el levels 1-3 and tet_1el levels 2-4, contrast-40 viscosity, Dirichlet
velocity."""
import numpy as np
import pytest

import epsilongmgutil as egu
import gmgutil as gm

pytestmark = pytest.mark.gpu
FUSED_TOL = 1e-13
MESHES = [("cube_6el", 1, 3), ("tet_1el", 2, 4)]


@pytest.fixture(scope="module")
def env():
    import torch

    import hostutil as hu
    from hyteg_amd import capi, host

    assert torch.cuda.is_available()
    capi.lib()
    host.lib()
    return torch, host, hu


def device(env, mesh, lo, hi):
    torch, host, hu = env
    return egu.Device(host, hu, torch.cuda.current_stream().cuda_stream, mesh, lo, hi)


def close_enough(got, want, d, what):
    bound = gm.tolerance(d)
    l2, worst = gm.rel(got, want), float(np.abs(got - want).max() / np.abs(want).max())
    print(f"{what}: relative L2 {l2:.3e}, largest entry error / max {worst:.3e} (bound {bound:.3e}, d {d:.3e})")
    assert l2 <= bound and worst <= bound


def neumann_on_w(host, fs):
    bc = host.BoundaryCondition()
    bc.create_neumann("open", [1])
    fs[2].set_boundary_condition(bc)


@pytest.mark.parametrize("w_open", [False, True], ids=["dirichlet", "neumann-on-w"])
@pytest.mark.parametrize("mesh,lo,hi", MESHES)
def test_residual_fused_composed_restated(env, mesh, lo, hi, w_open):
    """r = b - A x on Inner | NeumannBoundary.  neumann-on-w: the third component alone has a free boundary, so the components' SHELL
    class masks differ on every cell and the result still agrees.  The interior of a macro-cell stays Inner for every component there
    (comps = 7): a component whose inner points are excluded is test_a_component_fixed_everywhere_stays_out_of_the_fused_launches"""
    torch, host, hu = env
    dev = device(env, mesh, lo, hi)
    L = dev.h.levels[hi]
    free = np.concatenate([L.base.free, L.base.free, np.ones(L.n, dtype=bool)]) if w_open else None
    a, w = egu.smoother_call(mesh, lo, hi, 1, free=free), egu.smoother_call(mesh, lo, hi, 1, gm.LD, free=free)
    x0, b, want = a[0], a[1], a[2]
    sel = L.free if free is None else free
    prior = np.random.default_rng(5).standard_normal(3 * L.n)
    op = dev.operator()
    x, rhs = dev.vector("x", x0), dev.vector("b", b)
    out = {}
    for fused in (True, False):
        op.set_fused(fused)
        r = dev.vector("r", prior)
        if w_open:
            neumann_on_w(host, r)
        op.residual(x, rhs, r, hi, host.Inner | host.NeumannBoundary)
        out[fused] = dev.read(r)
        assert np.array_equal(out[fused][~sel], prior[~sel]), "a point the flag excludes was written"
    assert gm.rel(out[True], out[False]) <= FUSED_TOL
    close_enough(out[True][sel], want[sel], gm.rel(a[2], w[2]), f"{mesh} residual")
    dev.close()


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("mesh,lo,hi", MESHES)
def test_chebyshev_call_fused_composed_restated(env, mesh, lo, hi, order):
    """one ChebyshevSmoother call on the top level: the fused steps against set_fused( False ) and against the restatement"""
    torch, host, hu = env
    dev = device(env, mesh, lo, hi)
    a, w = egu.smoother_call(mesh, lo, hi, order), egu.smoother_call(mesh, lo, hi, order, gm.LD)
    op = dev.operator()
    smoother = host.EpsilonSolver.chebyshev(dev.st, lo, hi, order, dev.radii())
    rhs = dev.vector("b", a[1])
    out = {}
    for fused in (True, False):
        op.set_fused(fused)
        x = dev.vector("x", a[0])
        smoother.solve(op, x, rhs, hi)
        out[fused] = dev.read(x)
    assert gm.rel(out[True], out[False]) <= FUSED_TOL
    close_enough(out[True], a[3], gm.rel(a[3], w[3]), f"{mesh} Chebyshev({order})")
    smoother.close()
    dev.close()


def test_chebyshev_call_with_a_neumann_condition_on_w_alone(env):
    """cube_6el level 3, Chebyshev( 2 ): w is free on the mesh boundary, u and v are not"""
    torch, host, hu = env
    mesh, lo, hi, order = "cube_6el", 1, 3, 2
    dev = device(env, mesh, lo, hi)
    L = dev.h.levels[hi]
    free = np.concatenate([L.base.free, L.base.free, np.ones(L.n, dtype=bool)])
    a, w = egu.smoother_call(mesh, lo, hi, order, free=free), egu.smoother_call(mesh, lo, hi, order, gm.LD, free=free)
    op = dev.operator()
    smoother = host.EpsilonSolver.chebyshev(dev.st, lo, hi, order, dev.radii())
    rhs = dev.vector("b", a[1])
    out = {}
    for fused in (True, False):
        op.set_fused(fused)
        x = dev.vector("x", a[0])
        neumann_on_w(host, x)
        smoother.solve(op, x, rhs, hi)
        out[fused] = dev.read(x)
    assert gm.rel(out[True], out[False]) <= FUSED_TOL
    assert gm.rel(out[True][2 * L.n:][~L.base.free], a[0][2 * L.n:][~L.base.free]) > 1e-3, "the boundary values of w were smoothed"
    close_enough(out[True], a[3], gm.rel(a[3], w[3]), "Chebyshev(2), Neumann on w")
    smoother.close()
    dev.close()


def test_a_component_fixed_everywhere_stays_out_of_the_fused_launches(env):
    """cube_6el level 3: w under a condition that makes every mesh flag ( 0: the interior primitives, 1: the boundary ) a Dirichlet
    boundary, u and v under the default one.  The components' INNER masks then disagree on every cell: the fused launches run with
    comps = 0b011 and must leave w untouched (both store streams of the step); residual and one Chebyshev( 2 ) call, fused against
    set_fused( False ) and against the restatement with w fixed"""
    torch, host, hu = env
    mesh, lo, hi, order = "cube_6el", 1, 3, 2
    dev = device(env, mesh, lo, hi)
    L = dev.h.levels[hi]
    free = np.concatenate([L.base.free, L.base.free, np.zeros(L.n, dtype=bool)])
    a, w = egu.smoother_call(mesh, lo, hi, order, free=free), egu.smoother_call(mesh, lo, hi, order, gm.LD, free=free)
    w_fixed = np.random.default_rng(7).standard_normal(L.n)  # nonzero Dirichlet data in w: it enters u and v through the coupling
    x0 = np.concatenate([a[0][:2 * L.n], w_fixed])
    prior = np.random.default_rng(8).standard_normal(3 * L.n)

    def fix_w(fs):
        bc = host.BoundaryCondition()
        bc.create_dirichlet("everywhere", [0, 1])
        fs[2].set_boundary_condition(bc)

    def restated(dtype):
        keep, L.free = L.free, free
        try:
            xs, b = x0.astype(dtype), a[1].astype(dtype)
            return np.where(free, b - L.apply(xs), 0), gm.chebyshev_smoother(dev.h, order, egu.case_radii(mesh, lo, hi))(xs, b, hi)
        finally:
            L.free = keep

    (r_want, x_want), (r_wide, x_wide) = restated(np.float64), restated(gm.LD)
    op = dev.operator()
    smoother = host.EpsilonSolver.chebyshev(dev.st, lo, hi, order, dev.radii())
    rhs = dev.vector("b", a[1])
    res, out = {}, {}
    for fused in (True, False):
        op.set_fused(fused)
        x, r = dev.vector("x", x0), dev.vector("r", prior)
        fix_w(x), fix_w(r)
        op.residual(x, rhs, r, hi, host.Inner | host.NeumannBoundary)
        res[fused] = dev.read(r)
        smoother.solve(op, x, rhs, hi)
        out[fused] = dev.read(x)
        assert np.array_equal(res[fused][~free], prior[~free]) and np.array_equal(out[fused][~free], x0[~free]), "a fixed point was written"
    assert gm.rel(res[True], res[False]) <= FUSED_TOL and gm.rel(out[True], out[False]) <= FUSED_TOL
    close_enough(res[True][free], r_want[free], gm.rel(r_want, r_wide), "residual, w fixed")
    close_enough(out[True], x_want, gm.rel(x_want, x_wide), "Chebyshev(2), w fixed")
    smoother.close()
    dev.close()


def test_residual_in_place_is_refused_by_the_host_layer(env):
    """r = x given as the same handles: every argument becomes a view of its own, so the operator compares components, composes, and
    its apply refuses the aliased destination with an exception of the host layer (no launch, x unchanged)"""
    torch, host, hu = env
    mesh, lo, hi = "tet_1el", 2, 4
    dev = device(env, mesh, lo, hi)
    x0, b = egu.top_inputs(mesh, lo, hi)
    op = dev.operator()
    x, rhs = dev.vector("x", x0), dev.vector("b", b)
    with pytest.raises(host.HytegHostError, match="dst must differ"):
        op.residual(x, rhs, x, hi, host.Inner | host.NeumannBoundary)
    with pytest.raises(host.HytegHostError, match="dst must differ"):
        op.residual(x, rhs, [rhs[0], x[1], rhs[2]], hi, host.Inner | host.NeumannBoundary)
    assert np.array_equal(dev.read(x), x0)
    dev.close()


@pytest.mark.parametrize("c", egu.CYCLE_CASES, ids=egu.cycle_id)
def test_cycle_iterates_and_residual_reduction(env, c):
    """the iterates after cycles 1, 2 and 3 against the restated cycle, and the residual reduction of every cycle (evaluated on the
    dense matrix from the GPU's iterates) against the restated cycle's, within the bound measured for it"""
    torch, host, hu = env
    dev = device(env, c.mesh, c.lo, c.hi)
    want = egu.restated_cycles(c)
    x0, b = egu.top_inputs(c.mesh, c.lo, c.hi)
    op = dev.operator()
    if c.smoother == "chebyshev":
        solver = host.EpsilonSolver.gmg_chebyshev(dev.st, c.lo, c.hi, c.param, dev.radii(), pre=c.pre, post=c.post)
    else:
        solver = host.EpsilonSolver.gmg(dev.st, c.lo, c.hi, relax=c.param, pre=c.pre, post=c.post)
    x, rhs = dev.vector("x", x0), dev.vector("b", b)
    L = dev.h.levels[c.hi]

    def residual_norm(v):
        return float(np.linalg.norm(np.where(L.free, b - L.apply(v), 0.0)))

    # the reduction of a cycle within gmgutil.tolerance of the restated one, d measured on the reductions themselves (float64
    # against 80-bit) and on the iterates, whichever is larger
    bound = gm.tolerance(max(want.d, want.d_rate))
    res = [residual_norm(x0)]
    for k in range(egu.CYCLES):
        solver.solve(op, x, rhs, c.hi)
        got = dev.read(x)
        close_enough(got, want.iterates[k], want.d, f"{egu.cycle_id(c)} cycle {k + 1}")
        res.append(residual_norm(got))
        rate = res[-1] / res[-2]
        print(f"   residual reduction {rate:.6f} (restated {want.rates[k]:.6f}): relative difference {abs(rate / want.rates[k] - 1.0):.3e} (bound {bound:.3e})")
        assert abs(rate / want.rates[k] - 1.0) <= bound
    solver.close()
    dev.close()


def test_cg_preconditioned_with_the_cycle_needs_fewer_iterations(env):
    """cube_6el 1-3: CG to 1e-10 with the V( 1, 1 ) Chebyshev( 2 ) cycle as preconditioner against plain CG, both counted here"""
    torch, host, hu = env
    mesh, lo, hi = "cube_6el", 1, 3
    dev = device(env, mesh, lo, hi)
    L = dev.h.levels[hi]
    x0, b = egu.top_inputs(mesh, lo, hi)
    op = dev.operator()
    cycle = host.EpsilonSolver.gmg_chebyshev(dev.st, lo, hi, 2, dev.radii(), pre=1, post=1)
    counts = {}
    for name, pre in (("plain", None), ("cycle", cycle)):
        cg = host.EpsilonSolver.cg(dev.st, lo, hi, max_iter=2000, tol=1e-10, preconditioner=pre)
        x, rhs = dev.vector("x", x0), dev.vector("b", b)
        cg.solve(op, x, rhs, hi)
        counts[name] = cg.iterations
        got = dev.read(x)
        ratio = np.linalg.norm(np.where(L.free, b - L.apply(got), 0.0)) / np.linalg.norm(np.where(L.free, b - L.apply(x0), 0.0))
        print(f"{name} CG: {counts[name]} iterations, residual ratio on the dense matrix {ratio:.3e}")
        assert ratio <= 1e-9
        cg.close()
    assert 0 < counts["cycle"] < counts["plain"] < 2000
    cycle.close()
    dev.close()


def test_estimate_radius_against_the_restated_power_iteration(env):
    """estimate_radius( level, 20 ): chebyshev::estimateRadius statement by statement on the dense matrix, from the same start vector
    (three incommensurate waves, on ALL points as the reference's flag has it)"""
    torch, host, hu = env
    mesh, lo, hi, iterations = "cube_6el", 1, 3, 20
    dev = device(env, mesh, lo, hi)
    op = dev.operator()
    L = dev.h.levels[hi]
    q = L.base.coords

    def restated(dtype):
        A, dinv = L.matrix(dtype), (1.0 / L.D).astype(dtype)
        x = np.concatenate([np.sin(7.3 * q[:, 0] + 3.1 * q[:, 1] + 1.7 * q[:, 2] + 0.4), np.cos(2.9 * q[:, 0] - 6.1 * q[:, 1] + 4.3 * q[:, 2]),
                            np.sin(5.3 * q[:, 0] * q[:, 1] - 3.7 * q[:, 2] + 1.1)]).astype(dtype)
        x = x / np.sqrt(x @ x)
        t = dinv * (A @ x)
        for _ in range(iterations):
            x = t / np.sqrt(t @ t)
            t = dinv * (A @ x)
            radius = x @ t
        return float(radius)

    want, wide = restated(np.float64), restated(gm.LD)
    rho = op.estimate_radius(hi, iterations)
    bound = gm.tolerance(abs(want - wide) / wide)
    print(f"estimate_radius {rho:.12f}, restated {want:.12f} (bound {bound:.3e}); on the free points {egu.case_radii(mesh, lo, hi)[hi]:.6f}")
    assert abs(rho - want) <= bound * want
    dev.close()


# ---- the same two checks for div-k-grad: residual and smoother calls, fused against composed ----
@pytest.mark.parametrize("mesh,lo,hi", MESHES)
def test_divkgrad_residual_and_chebyshev_fused_against_composed(env, mesh, lo, hi):
    torch, host, hu = env
    h = gm.divkgrad_hierarchy(mesh, lo, hi)
    L = h.levels[hi]
    st = host.Storage.from_gmsh(hu.MESHES / f"{mesh}.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    idx = [L.glob.gidx[st.local_cell(i)[0]] for i in range(st.n_local_cells)]
    rng = np.random.default_rng(6)
    x0, b = (np.where(L.free, rng.standard_normal(L.glob.ndof), 0.0) for _ in range(2))
    prior = rng.standard_normal(L.glob.ndof)

    def function(name, vec, levels=(hi, hi)):
        f = host.P1Function(st, name, *levels)
        hu.upload(f, [np.ascontiguousarray(vec[ix]) for ix in idx], hi)
        return f

    def read(f):
        out = np.zeros(L.glob.ndof)
        for a, ix in zip(hu.download(f, hi), idx):
            out[ix] = a
        return out

    k = host.P1Function(st, "k", lo, hi)
    for l in range(lo, hi + 1):
        gl = h.levels[l].glob.gidx
        hu.upload(k, [np.ascontiguousarray(h.levels[l].k[gl[st.local_cell(i)[0]]]) for i in range(st.n_local_cells)], l)
    op = host.P1ElementwiseDivKGrad(st, lo, hi, k)
    op.compute_inverse_diagonal_operator_values()
    radii = [gm.spectral_radius(h.levels[l]) for l in range(lo, hi + 1)]
    x, rhs = function("x", x0), function("b", b)
    out = {}
    for fused in (True, False):
        op.set_fused(fused)
        r = function("r", prior)
        op.residual(x, rhs, r, hi, host.Inner | host.NeumannBoundary)
        out[fused] = read(r)
        assert np.array_equal(out[fused][~L.free], prior[~L.free])
        r.close()
    want = np.where(L.free, b - L.apply(x0), 0.0)
    assert gm.rel(out[True], out[False]) <= FUSED_TOL
    assert gm.rel(out[True][L.free], want[L.free]) <= 1e-12
    for order in (1, 2, 3):
        smoother = host.DivKGradSolver.chebyshev(st, lo, hi, order, radii)
        want = gm.chebyshev_smoother(h, order, dict(zip(range(lo, hi + 1), radii)))(x0, b, hi)
        for fused in (True, False):
            op.set_fused(fused)
            y = function("y", x0)
            smoother.solve(op, y, rhs, hi)
            out[fused] = read(y)
            y.close()
        print(f"{mesh} div-k-grad Chebyshev({order}): fused against composed {gm.rel(out[True], out[False]):.3e}, "
              f"against the restatement {gm.rel(out[True], want):.3e}")
        assert gm.rel(out[True], out[False]) <= FUSED_TOL
        assert gm.rel(out[True], want) <= 1e-12
        smoother.close()
    # one V( 1, 1 ) Chebyshev( 2 ) cycle of DivKGradSolver.gmg_chebyshev: the fused residual and the fused steps together against
    # set_fused( False ).  Bound 1e-12, not the 1e-13 of a single call: the cycle contains a coarse-grid CG that stops at a relative
    # residual of 1e-14, and two runs that differ in the last bits may stop one iteration apart
    cycle = host.DivKGradSolver.gmg_chebyshev(st, lo, hi, 2, radii, pre=1, post=1)

    def restated_cycle(dtype):
        xs = {l: np.zeros(h.levels[l].glob.ndof, dtype=dtype) for l in range(lo, hi + 1)}
        bs = {l: np.zeros(h.levels[l].glob.ndof, dtype=dtype) for l in range(lo, hi + 1)}
        xs[hi], bs[hi] = x0.astype(dtype), b.astype(dtype)
        gm.cycle(h, gm.chebyshev_smoother(h, 2, dict(zip(range(lo, hi + 1), radii))), xs, bs, hi, 1, 1)
        return xs[hi]

    want, wide = restated_cycle(np.float64), restated_cycle(gm.LD)
    for fused in (True, False):
        op.set_fused(fused)
        y, yb = function("y", x0, (lo, hi)), function("yb", b, (lo, hi))
        cycle.solve(op, y, yb, hi)
        out[fused] = read(y)
        y.close(), yb.close()
    print(f"{mesh} div-k-grad V(1,1) Chebyshev(2) cycle: fused against composed {gm.rel(out[True], out[False]):.3e}, "
          f"against the restated cycle {gm.rel(out[True], want):.3e} (bound {gm.tolerance(gm.rel(want, wide)):.3e})")
    assert gm.rel(out[True], out[False]) <= 1e-12
    assert gm.rel(out[True], want) <= gm.tolerance(gm.rel(want, wide))
    cycle.close()
    op.set_fused(True)
    for o in (x, rhs, op, k, st):
        o.close()
