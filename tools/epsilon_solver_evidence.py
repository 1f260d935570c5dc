#!/usr/bin/env python3
"""Solver evidence for DESIGN.md section 3.18: MINRES on the variable-viscosity Stokes operator to a relative residual of 1e-8 with
the "pressure", "block" and "block_viscosity" preconditioners, iterations and wall time, all in one run on one GPU.
  known:     the reference's known answer (tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp, 3-D case): the unit
             cube of six tetrahedra (meshCuboid), mu = 1, velocity hierarchy from level 2
  contrast:  the same right-hand side and Dirichlet values on cube_6el with mu = exp( 3 x ) ( 1 + y ) (contrast 40), velocity
             hierarchy from level 1
Usage: python tools/epsilon_solver_evidence.py [--levels 3 4 6] [--budget 60]
The mesh helpers and the known answer's functions are those of the tests (tests/epsilonutil.py, tests/hostutil.py)."""
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
from hyteg_amd import capi, host  # noqa: E402

KINDS = ("pressure", "block", "block_viscosity")


def solve(problem, level, kind, max_iter):
    lo = 2 if problem == "known" else 1
    if problem == "known":
        st = host.Storage.from_arrays(*eu.cuboid_mesh())
        st.set_mesh_boundary_flags_on_boundary(1, 0, True)
        viscosity = lambda x, y, z: np.ones_like(x)  # noqa: E731
    else:
        st = host.Storage.from_gmsh(hu.MESHES / "cube_6el.msh")
        viscosity = lambda x, y, z: np.exp(3.0 * x) * (1.0 + y)  # noqa: E731
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    orc = hu.MultiCellOracle(st)
    mu = host.P1Function(st, "mu", lo, level)
    for l in range(lo, level + 1):
        hu.upload(mu, orc.interpolate(viscosity, l), l)
    u, f = host.P1StokesFunction(st, "u", lo, level), host.P1StokesFunction(st, "f", lo, level)
    mass = host.P1ConstantOperator(st, level, level, form=1)
    tmp = host.P1Function(st, "tmp", level, level)
    for k, (fn, ex) in enumerate(zip((eu.known_rhs_u, eu.known_rhs_v, eu.known_rhs_w), (eu.known_u, eu.known_v, eu.known_w))):
        hu.upload(tmp, orc.interpolate(fn, level), level)
        mass.apply(tmp, f.components[k], level, host.All)
        exact = orc.interpolate(ex, level)
        hu.upload(u.components[k], [np.where(hu.point_mask(level, st.mask(i, host.DirichletBoundary)), e, 0.0) for i, e in enumerate(exact)], level)
    for g in (u.p, f.p):
        g.interpolate(0.0, level, host.All)
    op = host.P1P1EpsilonStokesOperator(st, lo, level, mu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver = host.EpsilonStokesSolver.minres(st, lo, level, max_iter=max_iter, rel_tol=1e-8, preconditioner=kind, mu=mu)
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
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--max-iter", type=int, default=10000)
    ap.add_argument("--budget", type=float, default=60.0, help="a (problem, level) whose first solve took longer than this is not continued")
    args = ap.parse_args()
    rows = []
    for problem in ("known", "contrast"):
        for level in args.levels:
            for kind in KINDS:
                row = solve(problem, level, kind, args.max_iter)
                rows.append(row)
                print(f"{problem:9s} level {level}  {kind:16s} {row['iterations']:6d} iterations{'' if row['converged'] else ' (NOT converged)'}  "
                      f"set-up {row['setup_s']:7.3f} s  solve {row['solve_s']:8.3f} s", flush=True)
                if row["solve_s"] > args.budget:
                    print(f"   over the budget of {args.budget:.0f} s: the other preconditioners at this level are not run", flush=True)
                    break
    print(json.dumps({"device": capi.device_name(), "rel_tol": 1e-8, "rows": rows}))


if __name__ == "__main__":
    main()
