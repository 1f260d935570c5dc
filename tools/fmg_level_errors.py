#!/usr/bin/env python3
"""L2 error per FMG level on cube_6el, levels 2-5, one V(2,2) Jacobi cycle per level, linear against quadratic FMG prolongation
(informational; profiles/p1p2_conversion.txt).  -laplace u = f, u = sin(pi x) sin(pi y) sin(pi z) on the unit cube,
u = 0 on the boundary.  Usage: python tools/fmg_level_errors.py"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import hostutil as hu  # noqa: E402
from hyteg_amd import host  # noqa: E402

LO, HI = 2, 5
exact = lambda x, y, z: np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)  # noqa: E731


def run(prolongation):
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/cube_6el.msh")
    st.set_stream(torch.cuda.current_stream().cuda_stream)
    orc = hu.MultiCellOracle(st)
    A, M = host.P1ConstantOperator(st, LO, HI), host.P1ConstantOperator(st, LO, HI, form=1)
    A.compute_inverse_diagonal()
    x, b, ue, f, err, tmp = (host.P1Function(st, n, LO, HI) for n in ("x", "b", "ue", "f", "err", "tmp"))
    for level in range(LO, HI + 1):
        u = orc.interpolate(exact, level)
        hu.upload(ue, u, level)
        hu.upload(f, [3.0 * np.pi**2 * a for a in u], level)
        M.apply(f, b, level, host.Inner)

    def l2(level):
        err.assign([1.0, -1.0], [x, ue], level, host.All)
        tmp.interpolate(0.0, level)
        M.apply(err, tmp, level, host.All)
        return float(np.sqrt(err.dot(tmp, level, host.All)))

    errors = {}
    gmg = host.Solver.gmg(st, LO, HI, smoother=host.JACOBI, relax=2.0 / 3.0, pre=2, post=2, cg_max_iter=500, cg_tol=1e-14)
    fmg = host.Solver.fmg(st, gmg, LO, HI, cycles_per_level=1, prolongation=prolongation,
                          post_cycle=lambda level: errors.__setitem__(level, l2(level)))
    fmg.solve(A, x, b, HI)
    for _ in range(15):
        gmg.solve(A, x, b, HI)
    return errors, l2(HI)


for kind in ("linear", "quadratic"):
    errors, converged = run(kind)
    print(f"FMG prolongation {kind}: L2 error after the cycle of each level: " + ", ".join(f"L{k}: {v:.4e}" for k, v in sorted(errors.items()))
          + f"; level {HI} after 15 more cycles (discretisation error): {converged:.4e}", flush=True)
