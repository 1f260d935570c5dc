#!/usr/bin/env python3
"""Solver evidence for DESIGN.md section 3.21: MINRES on the variable-viscosity Taylor-Hood Stokes operator (P2P1StokesEpsilonOperator)
to a relative residual of 1e-8 with the "pressure", "block" and "block_viscosity" preconditioners, iterations and wall time, all in one
run on one GPU.  The sibling of tools/epsilon_solver_evidence.py (P1-P1, section 3.18).
  known:     the reference's known answer (tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp, P2 3-D case): the unit
             cube of six tetrahedra (meshCuboid), mu = 1
  contrast:  the same right-hand side and Dirichlet values on cube_6el with mu = exp( 3 x ) ( 1 + y ) (contrast 40)
The velocity cycle of the block preconditioners runs on the levels 1 .. level (V( 1, 1 ) Chebyshev( 2 ), radii estimated at construction).
Usage: python tools/p2_epsilon_solver_evidence.py [--levels 2 3 4] [--budget 60]
The mesh helpers and the known answer's functions are those of the tests (tests/epsilonutil.py, tests/p2divkgradutil.py)."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import epsilonutil as eu  # noqa: E402
import hostutil as hu  # noqa: E402
import p2divkgradutil as pu  # noqa: E402
from hyteg_amd import capi, host  # noqa: E402

KINDS = ("pressure", "block", "block_viscosity")
LO = 1


def solve(problem, level, kind, max_iter):
    if problem == "known":
        st = host.Storage.from_arrays(*eu.cuboid_mesh())
        st.set_mesh_boundary_flags_on_boundary(1, 0, True)
        viscosity = lambda x, y, z: np.ones_like(x)  # noqa: E731
    else:
        st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
        viscosity = lambda x, y, z: np.exp(3.0 * x) * (1.0 + y)  # noqa: E731
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    tets = [np.asarray(st.local_cell(i)[1], dtype=np.float64).reshape(4, 3) for i in range(st.n_local_cells)]

    def fill(f, fn, l, keep=None):
        """fn at the DoF points of level l into the P2Function f (keep: per cell a mask of the DoFs that take the value, the others 0)"""
        nv = pu.vertex_size(l)
        for c, t in enumerate(tets):
            a = np.ascontiguousarray(fn(*pu.dof_points(t, l).T))
            if keep is not None:
                a = np.where(keep[c], a, 0.0)
            f.upload(l, a[:nv], a[nv:], cell=c)

    mu = host.P2Function(st, "mu", LO, level)
    for l in range(LO, level + 1):
        fill(mu, viscosity, l)
    u, f = host.TaylorHoodFunction(st, "u", LO, level), host.TaylorHoodFunction(st, "f", LO, level)
    for g in (u, f):
        g.interpolate(0.0, level, host.All)
    mass = host.P2ElementwiseMassOperator(st, level, level)
    tmp = host.P2Function(st, "tmp", level, level)
    dirichlet = [pu.dof_mask(level, st.mask(i, host.DirichletBoundary)) for i in range(st.n_local_cells)]
    for k, (fn, ex) in enumerate(zip((eu.known_rhs_u, eu.known_rhs_v, eu.known_rhs_w), (eu.known_u, eu.known_v, eu.known_w))):
        fill(tmp, fn, level)
        mass.apply(tmp, f.velocity[k], level, host.All)
        fill(u.velocity[k], ex, level, dirichlet)
    op = host.TaylorHoodEpsilonStokesOperator(st, LO, level, mu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver = host.TaylorHoodEpsilonSolver.minres(st, LO, level, max_iter=max_iter, rel_tol=1e-8, preconditioner=kind, mu=mu)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    solver.solve(op, u, f, level)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    row = dict(problem=problem, level=level, preconditioner=kind, iterations=solver.minres_iterations, converged=solver.minres_iterations < max_iter,
               setup_s=t1 - t0, solve_s=t2 - t1)
    for o in (solver, op, mass, tmp, u, f, mu, st):
        o.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--max-iter", type=int, default=10000)
    ap.add_argument("--budget", type=float, default=60.0, help="after a solve that took longer than this, the problem's higher levels are not run")
    args = ap.parse_args()
    rows = []
    for problem in ("known", "contrast"):
        over = False
        for level in sorted(args.levels):
            if over:
                print(f"{problem:9s} level {level}  not run: a solve at a lower level was over the budget of {args.budget:.0f} s", flush=True)
                continue
            for kind in KINDS:
                row = solve(problem, level, kind, args.max_iter)
                rows.append(row)
                print(f"{problem:9s} level {level}  {kind:16s} {row['iterations']:6d} iterations{'' if row['converged'] else ' (NOT converged)'}  "
                      f"set-up {row['setup_s']:7.3f} s  solve {row['solve_s']:8.3f} s", flush=True)
                over = over or row["solve_s"] > args.budget
    print(json.dumps({"device": capi.device_name(), "rel_tol": 1e-8, "velocity_min_level": LO, "rows": rows}))


if __name__ == "__main__":
    main()
