#!/usr/bin/env python3
"""Per-kernel timings of the whole P1 hot path on one GPU (level 8 by default) with algorithmic GB/s, plus V-cycle
timings through the host layer.  Not the headline bench (that is bench.py); this is the evidence table for
DESIGN.md section 3.  Usage: python tools/bench_kernels.py [--level 8] [--reps 200]
--only epsilon: the rows of the epsilon operator alone, levels 6..level, with the fused residual and Chebyshev steps
against the composed sequences they replace; --only divkgrad: the same pairs for div-k-grad; --only p2-divkgrad: the two
forms of the P2 div-k-grad apply, the constant P2 apply and a copy, levels 4..7; --only p2-epsilon: the fused P2 epsilon
apply in its forms against three P2 div-k-grad applies on the same arrays, levels 4..7; --only p2-epsilon-modes /
p2-divkgrad-modes: the fused residual, Jacobi and Chebyshev steps of the P2 operators against the composed sequences, levels 2..7
(DESIGN 3.21)."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hyteg_amd import capi, host  # noqa: E402


def cpu_rows(L, w, rows):
    """CPU baseline beside the GPU rows: the oracle's restatement of the reference's generated kernels, built with the flags of a
    HyTeG Release build (oracle/Makefile: -O3 -march=native), one thread as one MPI rank runs them; protocol of
    apps/benchmarks/KernelBench/3DKernelBench.cpp:59-82 (double the sweeps until a block lasts 0.5 s), bounded to ~2 s per row."""
    from oracle import p1_oracle as po

    n, nc, inner = po.cell_size(L), po.cell_size(L - 1), po.cell_inner_size(L)
    rng = np.random.default_rng(1)
    a, b, c, co = rng.random(n), rng.random(n), rng.random(n), rng.random(nc)
    ones = np.ones(14)
    fast = po.lib(fast=True)

    def protocol(fn, budget=2.0):
        fn()
        sweeps, total = 1, 0.0
        while True:
            t0 = time.perf_counter()
            for _ in range(sweeps):
                fn()
            dt = time.perf_counter() - t0
            total += dt
            if dt > 0.5 or total > budget:
                return dt / sweeps
            sweeps *= 2

    table = [
        ("apply Replace", lambda: po.apply_cell(b, a, L, w, fast=True), 16 * inner, inner),
        ("SOR forward sweep", lambda: po.sor_cell(b, a, L, w, 1.0, False, fast=True), 24 * inner, inner),
        ("Jacobi composition (apply + 3 vector passes)", lambda: po.jacobi_cell(b, c, a, L, w, 0.66, None, fast=True), 104 * inner, inner),
        ("restrict (fine L -> coarse L-1)", lambda: fast.ho_restrict_cell(po._p(co), po._p(a), L - 1, po._p(ones)), 8 * (n + nc), nc),
        ("prolongate (coarse L-1 -> fine L, incl. zeroing)",
         lambda: (fast.ho_prolongate_prepare(po._p(b), L, 0), fast.ho_prolongate_cell(po._p(co), po._p(b), L - 1, po._p(ones))), 8 * (n + nc), n),
    ]
    for name, fn, nbytes, updates in table:
        s_ = protocol(fn)
        us = s_ * 1e6
        rows.append(dict(kernel="CPU 1 core: " + name, us=us, GBps=nbytes / us * 1e-3, GDoFps=updates / us * 1e-3, algorithmic_bytes=nbytes))
        print(f"{'CPU 1 core: ' + name:58s} {us:12.1f} us  {nbytes / us * 1e-3:8.2f} GB/s  {updates / us * 1e-3:8.3f} GDoF/s", flush=True)


def epsilon_rows(top_level, reps, from_level=6):
    """--only epsilon: one macro-cell, inner points, levels 6..top_level.  Per level, in the same run: the fused epsilon
    apply and Jacobi step (z-march), every compiled brick shape, the one-thread-per-point form, NINE div-k-grad applies (what a
    block-composed epsilon operator costs at the least) and a copy of the same seven arrays.  Every operand class is a ring of its
    own, each 2.2 x the Infinity Cache, as for the div-k-grad rows."""
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
    rows = []
    for L in range(from_level, top_level + 1):
        n, inner = capi.cell_size(L), capi.cell_inner_size(L)
        nbuf = min(2049, max(6, -(-int(2.2 * 256 * 2**20) // (n * 8))))  # the cap binds below level 6 only: launch-bound there
        nbuf += -nbuf % 3  # three consecutive arrays per call
        S, D, X = ([torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)] for _ in range(3))
        M = [0.5 + 49.5 * torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf // 3)]  # the viscosity ring
        p3 = lambda t, k, o=0: [t[(3 * k + o + c) % nbuf].data_ptr() for c in range(3)]  # noqa: E731
        pm = lambda k: M[k % len(M)].data_ptr()  # noqa: E731

        def timeit(name, fn, nbytes, r=reps):
            for k in range(5):
                fn(k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(r):
                fn(k)
            e1.record(stream)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / r
            rows.append(dict(kernel=name, level=L, us=us, GBps=nbytes / us * 1e-3, GDoFps=3 * inner / us * 1e-3, algorithmic_bytes=nbytes))
            print(f"level {L}  {name:62s} {us:10.2f} us  {nbytes / us * 1e-3:8.1f} GB/s  {3 * inner / us * 1e-3:8.2f} GDoF/s", flush=True)

        apply_ = lambda k: capi.p1_elementwise_epsilon_apply_macro_3d_masked(p3(D, k), p3(S, k), pm(k), tet, 1 << L, 1 << 14, 0, sh)  # noqa: E731
        timeit("epsilon apply Replace, inner points (z-march, default shape)", apply_, 56 * inner)
        for ny, lz in capi.EPSILON_SHAPES:
            capi.p1_elementwise_epsilon_set_shape(ny, lz)
            timeit(f"epsilon apply Replace, inner points (z-march, shape {ny} x {lz})", apply_, 56 * inner)
        capi.p1_elementwise_epsilon_set_shape(0, 0)
        timeit("epsilon apply Add, inner points (z-march)",
               lambda k: capi.p1_elementwise_epsilon_apply_macro_3d_masked(p3(D, k), p3(S, k), pm(k), tet, 1 << L, 1 << 14, 1, sh), 80 * inner)
        timeit("epsilon Jacobi fused (z-march)",
               lambda k: capi.p1_elementwise_epsilon_jacobi_macro_3d(p3(D, k), p3(S, k), p3(X, 2 * k), p3(X, 2 * k, 3), pm(k), tet, 1 << L, 0.66, sh),
               104 * inner)
        capi.p1_elementwise_epsilon_set_inner_by_points(True)
        timeit("epsilon apply Replace, inner points (one thread per point)", apply_, 56 * inner, r=max(3, reps // 10))
        capi.p1_elementwise_epsilon_set_inner_by_points(False)

        def nine_divkgrad(k):
            d, s_ = p3(D, k), p3(S, k)
            for i in range(3):
                for j in range(3):
                    capi.p1_elementwise_divkgrad_apply_macro_3d_masked(d[i], s_[j], pm(k), tet, 1 << L, 1 << 14, 0 if j == 0 else 1, sh)

        timeit("epsilon yardstick: nine div-k-grad applies (3 Replace, 6 Add)", nine_divkgrad, (3 * 24 + 6 * 32) * inner)

        def copy7(k):
            d, s_ = p3(D, k), p3(S, k)
            capi.p1_assign_cell(d[0], [2.0, -1.0], [s_[0], pm(k)], L, sh)
            capi.p1_assign_cell(d[1], [2.0], [s_[1]], L, sh)
            capi.p1_assign_cell(d[2], [2.0], [s_[2]], L, sh)

        timeit("epsilon copy floor (assign: four arrays read, three written)", copy7, 56 * inner)

        # the fused residual and Chebyshev steps, and on the same arrays the composed sequences they replace, built from
        # the kernels that were there before: apply + assign, apply + assign + multElementwise, apply + multElementwise + assign per
        # component.  Bytes: what the fused launch has to move (the composed sequences move more; their GB/s column is on that scale too)
        inv = lambda k: p3(X, 2 * k, 3)  # noqa: E731
        rhs = lambda k: p3(X, 2 * k)  # noqa: E731
        timeit("epsilon residual fused (z-march)",
               lambda k: capi.p1_elementwise_epsilon_residual_macro_3d(p3(D, k), p3(S, k), rhs(k), pm(k), tet, 1 << L, 7, sh), 80 * inner)

        def residual_composed(k):
            d, r = p3(D, k), rhs(k)
            apply_(k)
            for c in range(3):
                capi.p1_assign_cell(d[c], [1.0, -1.0], [r[c], d[c]], L, sh)

        timeit("epsilon residual composed (apply + 3 assign)", residual_composed, 80 * inner)
        timeit("epsilon Chebyshev start fused (z-march)",
               lambda k: capi.p1_elementwise_epsilon_chebyshev_start_macro_3d(p3(D, k), rhs(k), p3(S, k), inv(k), pm(k), tet, 1 << L, 7, sh),
               104 * inner)

        def start_composed(k):
            d, r, i = p3(D, k), rhs(k), inv(k)
            apply_(k)
            for c in range(3):
                capi.p1_assign_cell(d[c], [1.0, -1.0], [r[c], d[c]], L, sh)
                capi.p1_mult_cell(d[c], [i[c], d[c]], L, sh)

        timeit("epsilon Chebyshev start composed (apply + 3 assign + 3 mult)", start_composed, 104 * inner)
        # x is the rhs ring here: read and rewritten at the inner points
        timeit("epsilon Chebyshev step fused (z-march)",
               lambda k: capi.p1_elementwise_epsilon_chebyshev_step_macro_3d(p3(D, k), rhs(k), p3(S, k), inv(k), pm(k), tet, 1 << L, 0.37, -0.21, 1, 7,
                                                                             sh), 128 * inner)

        step = lambda k: capi.p1_elementwise_epsilon_chebyshev_step_macro_3d(p3(D, k), rhs(k), p3(S, k), inv(k), pm(k), tet, 1 << L, 0.37, -0.21, 1,  # noqa: E731
                                                                             7, sh)
        for ny, lz in ((1, 4), (1, 8)):  # the step is not compiled at 2 x 4 (it would need scratch)
            capi.p1_elementwise_epsilon_set_shape(ny, lz)
            timeit(f"epsilon Chebyshev step fused (z-march, shape {ny} x {lz})", step, 128 * inner)
        capi.p1_elementwise_epsilon_set_shape(0, 0)

        def step_composed(k):
            d, x, i = p3(D, k), rhs(k), inv(k)
            apply_(k)
            for c in range(3):
                capi.p1_mult_cell(d[c], [i[c], d[c]], L, sh)
                capi.p1_assign_cell(x[c], [1.0, -0.21], [x[c], d[c]], L, sh)

        timeit("epsilon Chebyshev step composed (apply + 3 mult + 3 assign)", step_composed, 128 * inner)
        del S, D, X, M
    print(json.dumps({"levels": list(range(from_level, top_level + 1)), "device": capi.device_name(), "kernels": rows}))


def divkgrad_mode_rows(top_level, reps, from_level=6):
    """--only divkgrad: one macro-cell, inner points, levels 6..top_level.  Per level, in the same run: the fused residual
    and Chebyshev steps of div-k-grad, the composed sequences they replace on the same arrays (apply + assign, apply + assign +
    multElementwise, apply + multElementwise + assign), the apply alone and a copy floor.  Rings as for the epsilon rows."""
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
    rows = []
    for L in range(from_level, top_level + 1):
        n, inner = capi.cell_size(L), capi.cell_inner_size(L)
        nbuf = min(2048, max(4, -(-int(2.2 * 256 * 2**20) // (n * 8))))  # the cap binds below level 6 only: launch-bound there
        S, D, R, I = ([torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)] for _ in range(4))
        K = [1.0 + 0.5 * torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
        p = lambda t, k: t[k % nbuf].data_ptr()  # noqa: E731

        def timeit(name, fn, nbytes, r=reps):
            for k in range(5):
                fn(k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(r):
                fn(k)
            e1.record(stream)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / r
            rows.append(dict(kernel=name, level=L, us=us, GBps=nbytes / us * 1e-3, GDoFps=inner / us * 1e-3, algorithmic_bytes=nbytes))
            print(f"level {L}  {name:62s} {us:10.2f} us  {nbytes / us * 1e-3:8.1f} GB/s  {inner / us * 1e-3:8.2f} GDoF/s", flush=True)

        apply_ = lambda k: capi.p1_elementwise_divkgrad_apply_macro_3d_masked(p(D, k), p(S, k), p(K, k), tet, 1 << L, 1 << 14, 0, sh)  # noqa: E731
        timeit("div-k-grad apply Replace, inner points (z-march)", apply_, 24 * inner)
        timeit("div-k-grad residual fused (z-march)",
               lambda k: capi.p1_elementwise_divkgrad_residual_macro_3d(p(D, k), p(S, k), p(R, k), p(K, k), tet, 1 << L, sh), 32 * inner)

        def residual_composed(k):
            apply_(k)
            capi.p1_assign_cell(p(D, k), [1.0, -1.0], [p(R, k), p(D, k)], L, sh)

        timeit("div-k-grad residual composed (apply + assign)", residual_composed, 32 * inner)
        timeit("div-k-grad Chebyshev start fused (z-march)",
               lambda k: capi.p1_elementwise_divkgrad_chebyshev_start_macro_3d(p(D, k), p(R, k), p(S, k), p(I, k), p(K, k), tet, 1 << L, sh), 40 * inner)

        def start_composed(k):
            residual_composed(k)
            capi.p1_mult_cell(p(D, k), [p(I, k), p(D, k)], L, sh)

        timeit("div-k-grad Chebyshev start composed (apply + assign + mult)", start_composed, 40 * inner)
        timeit("div-k-grad Chebyshev step fused (z-march)",
               lambda k: capi.p1_elementwise_divkgrad_chebyshev_step_macro_3d(p(D, k), p(R, k), p(S, k), p(I, k), p(K, k), tet, 1 << L, 0.37, -0.21, 1,
                                                                              sh), 48 * inner)

        def step_composed(k):
            apply_(k)
            capi.p1_mult_cell(p(D, k), [p(I, k), p(D, k)], L, sh)
            capi.p1_assign_cell(p(R, k), [1.0, -0.21], [p(R, k), p(D, k)], L, sh)

        timeit("div-k-grad Chebyshev step composed (apply + mult + assign)", step_composed, 48 * inner)
        timeit("div-k-grad copy floor (assign 2 sources: two arrays read, one written)",
               lambda k: capi.p1_assign_cell(p(D, k), [2.0, -1.0], [p(S, k), p(K, k)], L, sh), 24 * inner)
        del S, D, R, I, K
    print(json.dumps({"levels": list(range(from_level, top_level + 1)), "device": capi.device_name(), "kernels": rows}))


def p2_divkgrad_rows(top_level, reps, from_level=4, repeats=5):
    """--only p2-divkgrad: the macro-cell of tet_1el, all DoFs, levels from_level..top_level.  Per level, in the same run and
    alternating in every one of `repeats` rounds: the P2 div-k-grad apply with the inner form on the inner DoFs, the same through the gather
    form on every DoF, the constant-coefficient P2 apply on the same cell, and a device copy that moves the bytes of the six arrays (four
    read, two written).  Reported: the median of the rounds and their spread (min .. max); a form is faster only beyond that spread.
    Rings: every array class exceeds the Infinity Cache 2.2 times, capped at 256 buffers (the small levels are launch-bound anyway)."""
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
    rows = []
    before = capi.p2_elementwise_divkgrad_set_inner_min_level(2)
    for L in range(from_level, top_level + 1):
        nv, ne = capi.cell_size(L), capi.p2_edge_array_size(L)
        dofs = nv + ne
        nbuf = min(256, max(4, -(-int(2.2 * 256 * 2**20) // (ne * 8))))
        rnd = lambda n, lo=0.0: [lo + torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]  # noqa: E731
        DV, DE, SV, SE, KV, KE = rnd(nv), rnd(ne), rnd(nv), rnd(ne), rnd(nv, 0.5), rnd(ne, 0.5)
        half = (3 * dofs) // 2
        CA, CB = rnd(half), rnd(half)
        geometry = capi.p2_elementwise_divkgrad_geometry(tet, L)
        table = torch.from_numpy(np.asarray(capi.p2_build_operator_table(capi.p2_elementwise_diffusion_element_matrices(tet, 1 << L)))).to("cuda")
        p = lambda t, k: t[k % nbuf].data_ptr()  # noqa: E731

        def divkgrad(gather):
            return lambda k: capi.p2_elementwise_divkgrad_apply_cell(p(DV, k), p(DE, k), p(SV, k), p(SE, k), p(KV, k), p(KE, k), L, geometry, 1.0, 0,
                                                                     0x7FFF, 0xFF, sh, gather=gather)

        table_rows = [
            ("P2 div-k-grad apply: inner form (+ gather form on the boundary DoFs)", divkgrad(False), 48 * dofs),
            ("P2 div-k-grad apply: gather form on every DoF", divkgrad(True), 48 * dofs),
            ("constant-coefficient P2 apply on the same cell", lambda k: capi.p2_elementwise_apply_cell(p(DV, k), p(DE, k), p(SV, k), p(SE, k), L,
                                                                                                     table.data_ptr(), 1.0, 0, 0x7FFF, sh), 16 * dofs),
            ("device copy moving the bytes of the six arrays", lambda k: CA[k % nbuf].copy_(CB[k % nbuf]), 24 * dofs),
        ]
        for name, fn, nbytes in table_rows:  # warm every shape
            for k in range(3):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in table_rows}
        for _ in range(repeats):
            for name, fn, nbytes in table_rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for k in range(reps):
                    fn(k)
                e1.record(stream)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
        for name, fn, nbytes in table_rows:
            t = sorted(times[name])
            us = t[len(t) // 2]
            rows.append(dict(kernel=name, level=L, us=us, us_min=t[0], us_max=t[-1], GBps=nbytes / us * 1e-3, GDoFps=dofs / us * 1e-3,
                             algorithmic_bytes=nbytes, dofs=dofs))
            print(f"level {L}  {name:70s} {us:10.2f} us  ({t[0]:.2f} .. {t[-1]:.2f})  {nbytes / us * 1e-3:8.1f} GB/s  {dofs / us * 1e-3:8.3f} GDoF/s",
                  flush=True)
        del DV, DE, SV, SE, KV, KE, CA, CB
    capi.p2_elementwise_divkgrad_set_inner_min_level(before)
    print(json.dumps({"levels": list(range(from_level, top_level + 1)), "device": capi.device_name(), "repeats": repeats, "kernels": rows}))


def p2_epsilon_rows(top_level, reps, from_level=4, repeats=5):
    """--only p2-epsilon: the macro-cell of tet_1el, all DoFs of the three components, levels from_level..top_level.  Per level,
    in the same run and alternating in every one of `repeats` rounds: the fused P2 epsilon apply with the inner form on the inner DoFs, the
    same through the gather form on every DoF, the apply as shipped (the default inner_min_level), and the yardstick: three
    P2ElementwiseDivKGrad applies (as shipped) on the same arrays -- the three diagonal blocks alone, a lower bound of any block
    composition.  Reported: the median of the rounds and their spread (min .. max); a form is faster only beyond that spread.
    Rings as for p2-divkgrad: every array class exceeds the Infinity Cache 2.2 times, capped at 256 buffers."""
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
    rows = []
    shipped = capi.p2_elementwise_epsilon_set_inner_min_level(2)
    capi.p2_elementwise_epsilon_set_inner_min_level(shipped)
    for L in range(from_level, top_level + 1):
        nv, ne = capi.cell_size(L), capi.p2_edge_array_size(L)
        dofs = 3 * (nv + ne)
        nbuf = min(256, max(4, -(-int(2.2 * 256 * 2**20) // (ne * 8))))
        rnd = lambda n, lo=0.0: [lo + torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]  # noqa: E731
        DV, DE, SV, SE = ([rnd(n) for _ in range(3)] for n in (nv, ne, nv, ne))
        MV, ME = rnd(nv, 0.5), rnd(ne, 0.5)
        geometry = capi.p2_elementwise_epsilon_geometry(tet, L)
        geometry_dk = capi.p2_elementwise_divkgrad_geometry(tet, L)
        p = lambda t, k: t[k % nbuf].data_ptr()  # noqa: E731
        p3 = lambda ts, k: [t[k % nbuf].data_ptr() for t in ts]  # noqa: E731

        def epsilon(gather, inner_min_level):
            def fn(k):
                capi.p2_elementwise_epsilon_apply_cell(p3(DV, k), p3(DE, k), p3(SV, k), p3(SE, k), p(MV, k), p(ME, k), L, geometry, 1.0, 0, 0x7FFF,
                                                       0xFF, sh, gather=gather)
            return fn, inner_min_level

        def three_divkgrad(k):
            for c in range(3):
                capi.p2_elementwise_divkgrad_apply_cell(p(DV[c], k), p(DE[c], k), p(SV[c], k), p(SE[c], k), p(MV, k), p(ME, k), L, geometry_dk, 1.0, 0,
                                                        0x7FFF, 0xFF, sh)

        nbytes = 8 * (2 * dofs + nv + ne)  # three components read, three written, the viscosity read
        table_rows = [
            ("P2 epsilon apply: inner form (+ gather form on the boundary DoFs)", *epsilon(False, 2)),
            ("P2 epsilon apply: gather form on every DoF", *epsilon(True, shipped)),
            ("P2 epsilon apply as shipped", *epsilon(False, shipped)),
            ("yardstick: three P2 div-k-grad applies on the same arrays", three_divkgrad, shipped),
        ]

        for name, fn, sw in table_rows:  # warm every shape
            capi.p2_elementwise_epsilon_set_inner_min_level(sw)
            for k in range(3):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in table_rows}
        for _ in range(repeats):
            for name, fn, sw in table_rows:
                capi.p2_elementwise_epsilon_set_inner_min_level(sw)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for k in range(reps):
                    fn(k)
                e1.record(stream)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
        for name, fn, sw in table_rows:
            t = sorted(times[name])
            us = t[len(t) // 2]
            rows.append(dict(kernel=name, level=L, us=us, us_min=t[0], us_max=t[-1], GBps=nbytes / us * 1e-3, GDoFps=dofs / us * 1e-3,
                             algorithmic_bytes=nbytes, dofs=dofs))
            print(f"level {L}  {name:70s} {us:10.2f} us  ({t[0]:.2f} .. {t[-1]:.2f})  {nbytes / us * 1e-3:8.1f} GB/s  {dofs / us * 1e-3:8.3f} GDoF/s",
                  flush=True)
        del DV, DE, SV, SE, MV, ME
    capi.p2_elementwise_epsilon_set_inner_min_level(shipped)
    print(json.dumps({"levels": list(range(from_level, top_level + 1)), "device": capi.device_name(), "repeats": repeats,
                      "shipped_inner_min_level": shipped, "kernels": rows}))


def p2_varcoef_mode_rows(op, top_level, reps, from_level=2, repeats=5):
    """--only p2-epsilon-modes / p2-divkgrad-modes: the fused residual, Jacobi step, Chebyshev start and Chebyshev step of a P2
    variable-coefficient operator on the macro-cell of tet_1el, all DoFs, as shipped (the default inner_min_level), each against the
    composed sequence on the same arrays in the same run: the apply as shipped plus the vector passes the host layer ran before the fused
    steps (per component a vertex launch and an edge launch per pass).  Rows alternate in every one of `repeats` rounds; reported: the
    median and the spread (min .. max).  Rings as for p2-divkgrad."""
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
    nc = 3 if op == "epsilon" else 1
    rows = []
    for L in range(from_level, top_level + 1):
        nv, ne = capi.cell_size(L), capi.p2_edge_array_size(L)
        dofs = nc * (nv + ne)
        nbuf = min(256, max(4, -(-int(2.2 * 256 * 2**20) // (ne * 8))))
        rnd = lambda n, lo=0.0: [lo + torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]  # noqa: E731
        ring = lambda lo=0.0: ([rnd(nv, lo) for _ in range(nc)], [rnd(ne, lo) for _ in range(nc)])  # noqa: E731
        D, S, R, I, X = ring(), ring(), ring(), ring(0.5), ring()
        KV, KE = rnd(nv, 0.5), rnd(ne, 0.5)
        geometry = getattr(capi, f"p2_elementwise_{op}_geometry")(tet, L)
        ptr = lambda t, k: t[k % nbuf].data_ptr()  # noqa: E731
        arg = lambda F, k: [[ptr(t, k) for t in half] if nc == 3 else ptr(half[0], k) for half in F]  # noqa: E731
        coef = lambda k: [ptr(KV, k), ptr(KE, k)]  # noqa: E731

        def apply_(k):
            getattr(capi, f"p2_elementwise_{op}_apply_cell")(*arg(D, k), *arg(S, k), *coef(k), L, geometry, 1.0, 0, 0x7FFF, 0xFF, sh)

        def passes(k, *ops):
            """( what, dst ring, scalars or None, source rings ): per component a vertex launch and an edge launch"""
            for what, dst, scalars, srcs in ops:
                for c in range(nc):
                    sv, se = [ptr(s[0][c], k) for s in srcs], [ptr(s[1][c], k) for s in srcs]
                    if what == "assign":
                        capi.p1_assign_cell(ptr(dst[0][c], k), scalars, sv, L, sh)
                    else:
                        capi.p1_mult_cell(ptr(dst[0][c], k), sv, L, sh)
                    capi.p2_edge_vector_cell_masked(0 if what == "assign" else 2, ptr(dst[1][c], k), se, scalars, L, 0x7FFF, sh)

        def composed(*ops):
            def fn(k):
                apply_(k)
                passes(k, *ops)
            return fn

        table_rows = [
            ("residual fused", lambda k: capi.p2_varcoef_residual_cell(op, arg(D, k), arg(S, k), arg(R, k), coef(k), L, geometry, stream=sh)),
            ("residual composed (apply + assign)", composed(("assign", D, [1.0, -1.0], [R, D]))),
            ("Jacobi step fused",
             lambda k: capi.p2_varcoef_jacobi_cell(op, arg(D, k), arg(S, k), arg(R, k), arg(I, k), coef(k), L, geometry, 0.6, stream=sh)),
            ("Jacobi step composed (apply + assign + mult + assign)",
             composed(("assign", D, [1.0, -1.0], [R, D]), ("mult", D, None, [I, D]), ("assign", D, [1.0, 0.6], [S, D]))),
            ("Chebyshev start fused",
             lambda k: capi.p2_varcoef_chebyshev_start_cell(op, arg(D, k), arg(S, k), arg(R, k), arg(I, k), coef(k), L, geometry, stream=sh)),
            ("Chebyshev start composed (apply + assign + mult)", composed(("assign", D, [1.0, -1.0], [R, D]), ("mult", D, None, [I, D]))),
            ("Chebyshev step fused", lambda k: capi.p2_varcoef_chebyshev_step_cell(op, arg(D, k), arg(X, k), arg(S, k), arg(I, k), coef(k), L, geometry,
                                                                                     0.37, -0.21, 1, stream=sh)),
            ("Chebyshev step composed (apply + mult + assign)", composed(("mult", D, None, [I, D]), ("assign", X, [1.0, -0.21], [X, D]))),
            ("apply as shipped", apply_),
        ]
        for name, fn in table_rows:  # warm every shape
            for k in range(3):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name, _ in table_rows}
        for _ in range(repeats):
            for name, fn in table_rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for k in range(reps):
                    fn(k)
                e1.record(stream)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
        for name, fn in table_rows:
            t = sorted(times[name])
            us = t[len(t) // 2]
            rows.append(dict(kernel=f"P2 {op} {name}", level=L, us=us, us_min=t[0], us_max=t[-1], dofs=dofs))
            print(f"level {L}  P2 {op:9s} {name:56s} {us:10.2f} us  ({t[0]:.2f} .. {t[-1]:.2f})", flush=True)
        del D, S, R, I, X, KV, KE
    print(json.dumps({"levels": list(range(from_level, top_level + 1)), "device": capi.device_name(), "repeats": repeats, "kernels": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--from-level", type=int, default=6, help="--only epsilon / divkgrad: the lowest level timed (2..level)")
    ap.add_argument("--only", default=None, help="time only the kernel rows whose name contains this text (skips the cycles)")
    ap.add_argument("--cpu", action="store_true",
                    help="also time the CPU restatement of the reference kernels (oracle/, gcc -O3 -march=native, 1 thread) for apply, "
                         "SOR, the Jacobi composition, restriction and prolongation (BASELINE.md section 2) -- a reported baseline")
    args = ap.parse_args()
    L, reps = args.level, args.reps
    if args.only == "epsilon":
        epsilon_rows(min(L, 8), reps, max(2, args.from_level))
        return
    if args.only == "divkgrad":
        divkgrad_mode_rows(min(L, 8), reps, max(2, args.from_level))
        return
    if args.only == "p2-divkgrad":
        p2_divkgrad_rows(min(L, 7), reps, min(4, max(0, args.from_level)))
        return
    if args.only == "p2-epsilon":
        p2_epsilon_rows(min(L, 7), reps, min(4, max(0, args.from_level)))
        return
    if args.only in ("p2-epsilon-modes", "p2-divkgrad-modes"):
        p2_varcoef_mode_rows(args.only.split("-")[1], min(L, 7), reps, min(7, max(2, args.from_level)))
        return
    n, inner = capi.cell_size(L), capi.cell_inner_size(L)
    nc = capi.cell_size(L - 1)
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    # every array class (sources, destinations, third operands) alone exceeds the 256 MiB Infinity Cache 2.2 times: a ring that only
    # exceeds it in total is READ from that cache when the destination is written with nontemporal stores (round 3)
    nbuf = max(2, -(-int(2.2 * 256 * 2**20) // (n * 8)))
    A = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    B = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    Cc = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    Co = [torch.rand(nc, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    st = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/tet_1el.msh")
    st.set_stream(sh)
    op = host.P1ConstantOperator(st, 2, L)
    w = list(op.stencils(0, L)[0])
    ones = [1.0] * 14
    res = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(capi.dot_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    rows = []

    def timeit(name, fn, bytes_per_call, updates, r=reps):
        if args.only and args.only not in name:
            return
        for k in range(5):
            fn(k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(r):
            fn(k)
        e1.record(stream)
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / r
        rows.append(dict(kernel=name, us=us, GBps=bytes_per_call / us * 1e-3, GDoFps=updates / us * 1e-3,
                         algorithmic_bytes=bytes_per_call))
        print(f"{name:44s} {us:10.2f} us  {bytes_per_call / us * 1e-3:8.1f} GB/s  {updates / us * 1e-3:8.1f} GDoF/s", flush=True)

    if args.cpu:
        cpu_rows(L, w, rows)
    p = lambda t, k: t[k % nbuf].data_ptr()  # noqa: E731
    timeit("apply Replace", lambda k: capi.p1_apply_cell(p(B, k), p(A, k), L, w, 0, sh), 16 * inner, inner)
    timeit("apply Add", lambda k: capi.p1_apply_cell(p(B, k), p(A, k), L, w, 1, sh), 24 * inner, inner)
    timeit("Jacobi fused (scalar inverse diagonal)", lambda k: capi.p1_jacobi_cell(p(B, k), p(Cc, k), p(A, k), L, w, 0.66, None, sh),
           24 * inner, inner)
    timeit("Jacobi fused (inverse-diagonal function)",
           lambda k: capi.p1_jacobi_cell(p(B, k), p(Cc, k), p(A, k), L, w, 0.66, p(Cc, k + 1), sh), 32 * inner, inner)
    # variable-coefficient diffusion -div( k grad u ) (levels <= 8): the inner points by the z-march and by the
    # one-thread-per-point kernel, the fused Jacobi step, and in the same run the constant-coefficient apply and a copy floor that moves
    # the same three arrays (two read, one written).  182 fp64 instructions (254 flop) per point; --only div-k-grad times these rows alone
    if L <= 8:
        tet = [list(map(float, v)) for v in st.local_cell(0)[1]]
        K = [1.0 + 0.5 * t for t in Cc]  # the coefficient ring: k in [1, 1.5]
        dkg_flop = 254 * inner
        before = len(rows)
        timeit("div-k-grad apply Replace, inner points (z-march)",
               lambda k: capi.p1_elementwise_divkgrad_apply_macro_3d_masked(p(B, k), p(A, k), p(K, k), tet, 1 << L, 1 << 14, 0, sh), 24 * inner, inner)
        capi.p1_elementwise_divkgrad_set_inner_by_points(True)
        timeit("div-k-grad apply Replace, inner points (one thread per point)",
               lambda k: capi.p1_elementwise_divkgrad_apply_macro_3d_masked(p(B, k), p(A, k), p(K, k), tet, 1 << L, 1 << 14, 0, sh), 24 * inner, inner)
        capi.p1_elementwise_divkgrad_set_inner_by_points(False)
        timeit("div-k-grad Jacobi fused (z-march)",
               lambda k: capi.p1_elementwise_divkgrad_jacobi_macro_3d(p(B, k), p(A, k), p(Cc, k), p(Cc, k + 1), p(K, k), tet, 1 << L, 0.66, sh),
               40 * inner, inner)
        for r_ in rows[before:]:
            r_["fp64_TFLOPs"] = dkg_flop / r_["us"] * 1e-6
            print(f"    {r_['kernel']}: {r_['fp64_TFLOPs']:.2f} TFLOP/s fp64")
        # set-up work (one thread per point, all points): diag += the element diagonals; k read, diag read and written
        timeit("div-k-grad diagonal (set-up, one thread per point)",
               lambda k: capi.p1_elementwise_divkgrad_diagonal_macro_3d(p(B, k), p(K, k), tet, 1 << L, sh), 24 * n, n, r=max(3, reps // 10))
        timeit("div-k-grad yardstick: constant-coefficient apply Replace", lambda k: capi.p1_apply_cell(p(B, k), p(A, k), L, w, 0, sh), 16 * inner, inner)
        timeit("div-k-grad copy floor (assign 2 sources: two arrays read, one written)",
               lambda k: capi.p1_assign_cell(p(B, k), [2.0, -1.0], [p(A, k), p(K, k)], L, sh), 24 * inner, inner)
        del K
    # one step of the Chebyshev smoother: t_out = invDiag .* (A t_in), x += c_prev t_in + c_cur t_out -- fused into one launch,
    # and composed from the kernels of the smoother's generic path (apply, multElementwise, assign) on rings of their own
    X = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    timeit("Chebyshev step, fused (scalar inverse diagonal)",
           lambda k: capi.p1_chebyshev_step_cell(p(B, k), p(X, k), p(A, k), L, w, 0.5, -0.1, True, None, sh), 32 * inner, inner)
    timeit("Chebyshev step, fused (inverse-diagonal function)",
           lambda k: capi.p1_chebyshev_step_cell(p(B, k), p(X, k), p(A, k), L, w, 0.5, -0.1, True, p(Cc, k), sh), 40 * inner, inner)
    timeit("Chebyshev start, fused (inverse-diagonal function)",
           lambda k: capi.p1_chebyshev_start_cell(p(B, k), p(X, k), p(A, k), L, w, p(Cc, k), sh), 32 * inner, inner)

    def chebyshev_step_composed(k):
        capi.p1_apply_cell(p(B, k), p(A, k), L, w, 0, sh)
        capi.p1_mult_cell(p(B, k), [p(Cc, k), p(B, k)], L, sh)
        capi.p1_assign_cell(p(X, k), [1.0, -0.1], [p(X, k), p(B, k)], L, sh)

    timeit("Chebyshev step, composed (apply + multElementwise + assign)", chebyshev_step_composed, 64 * inner, inner)
    del X
    timeit("assign 1 source", lambda k: capi.p1_assign_cell(p(B, k), [2.0], [p(A, k)], L, sh), 16 * inner, inner)
    timeit("assign 2 sources", lambda k: capi.p1_assign_cell(p(B, k), [2.0, -1.0], [p(A, k), p(Cc, k)], L, sh), 24 * inner, inner)
    timeit("add 1 source", lambda k: capi.p1_add_cell(p(B, k), [2.0], [p(A, k)], L, sh), 24 * inner, inner)
    timeit("multElementwise 2 sources", lambda k: capi.p1_mult_cell(p(B, k), [p(A, k), p(Cc, k)], L, sh), 24 * inner, inner)
    timeit("dot", lambda k: capi.p1_dot_cell(p(A, k), p(B, k), L, res.data_ptr(), ws.data_ptr(), sh), 16 * inner, inner)
    # the vector body of a CG iteration: x += alpha p, r -= alpha ap and <r,r> in one pass, beside the three calls the host
    # layer composes it from on one macro-cell (the inner points); information, no threshold is attached
    D4 = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(nbuf)]
    timeit("CG update, fused (x += a p, r -= a Ap, <r,r>)",
           lambda k: capi.p1_cg_update_cells([p(A, k)], [p(B, k)], [p(Cc, k)], [p(D4, k)], 1e-3, L, [0x4000], [0x4000], res.data_ptr(), ws.data_ptr(), sh),
           48 * inner, inner)

    def cg_update_composed(k):
        capi.p1_vector_cell_masked(1, p(A, k), [1e-3], [p(Cc, k)], L, 0x4000, sh)
        capi.p1_vector_cell_masked(1, p(B, k), [-1e-3], [p(D4, k)], L, 0x4000, sh)
        capi.p1_dot_cell_masked(p(B, k), p(B, k), L, 0x4000, res.data_ptr(), ws.data_ptr(), sh)

    timeit("CG update, composed (add, add, dot)", cg_update_composed, 56 * inner, inner)
    del D4
    # the statistics reduction of the function classes (sum, sum of magnitudes, min, max, max magnitude in one pass over the
    # array, all point classes) beside the dot product of the same array with itself through the batched entry, which decodes the same
    # point classes; a diagnostic kernel: the figures are information, no threshold is attached
    rws = torch.zeros(capi.reduce_workspace_bytes() // 8, dtype=torch.float64, device="cuda")
    res5 = torch.zeros(capi.REDUCE_COUNT, dtype=torch.float64, device="cuda")
    timeit("statistics reduction (5 numbers, 1 cell, full mask)",
           lambda k: capi.p1_reduce_cells([p(A, k)], L, [0x7FFF], res5.data_ptr(), rws.data_ptr(), sh), 8 * n, n)
    timeit("dot a.a beside the statistics reduction (batched entry, 1 cell, full mask)",
           lambda k: capi.p1_dot_cells([p(A, k)], [p(A, k)], L, [0x7FFF], res.data_ptr(), ws.data_ptr(), sh), 8 * n, n)
    timeit("restrict (fine L -> coarse L-1)", lambda k: capi.p1_restrict_cell(p(Co, k), p(A, k), L - 1, ones, sh), 8 * (n + nc), nc)
    timeit("prolongate Replace (coarse L-1 -> fine L)", lambda k: capi.p1_prolongate_cell(p(Co, k), p(B, k), L - 1, ones, 0, sh),
           8 * (n + nc), n)
    # float32 instantiations: algorithmic bytes halve
    Af = [t.to(torch.float32) for t in A] + [torch.rand(n, dtype=torch.float32, device="cuda") for _ in range(nbuf)]  # 2 nbuf: half the bytes
    Bf = [t.to(torch.float32) for t in B] + [torch.rand(n, dtype=torch.float32, device="cuda") for _ in range(nbuf)]
    Cf = [t.to(torch.float32) for t in Cc] + [torch.rand(n, dtype=torch.float32, device="cuda") for _ in range(nbuf)]
    pf = lambda t, k: t[k % len(t)].data_ptr()  # noqa: E731
    timeit("apply Replace, float32", lambda k: capi.p1_apply_cell_f32(pf(Bf, k), pf(Af, k), L, w, 0, sh), 8 * inner, inner)
    timeit("Jacobi fused, float32 (scalar inverse diagonal)",
           lambda k: capi.p1_jacobi_cell_f32(pf(Bf, k), pf(Cf, k), pf(Af, k), L, w, 0.66, None, sh), 12 * inner, inner)
    for name, alg in (("dataflow, one launch", capi.SOR_DATAFLOW), ("16^3 blocks, one launch per block wavefront", capi.SOR_BLOCKS)):
        capi.set_sor_algorithm(alg)
        timeit(f"SOR forward sweep ({name})", lambda k: capi.p1_sor_cell(p(B, k), p(A, k), L, w, 1.0, False, sh), 24 * inner, inner,
               r=max(3, reps // 40))
        timeit(f"SOR backward sweep ({name})", lambda k: capi.p1_sor_cell(p(B, k), p(A, k), L, w, 1.0, True, sh), 24 * inner, inner,
               r=max(3, reps // 40))
    capi.set_sor_algorithm(capi.SOR_AUTO)
    # the sweeps of a smoothing phase as one pipeline of block wavefronts (bytes / DoFs of ALL the sweeps of a call)
    for ns in (2, 3, 4):
        timeit(f"SOR {ns} forward sweeps, pipelined (per call)", lambda k: capi.p1_sor_cell_sweeps(p(B, k), p(A, k), L, w, 1.0, ns, False, sh),
               ns * 24 * inner, ns * inner, r=max(3, reps // 40))
    # Gauss-Seidel on the cell's macro-vertices/-edges/-faces (what a multi-cell sweep adds per cell); octahedron weights
    sys.path.insert(0, str(ROOT / "tests"))
    import hostutil as hu  # noqa: E402

    mv, mc = hu.read_msh(ROOT / "hyteg_amd/data/meshes/regular_octahedron_8el.msh")
    T = hu.sor_tables(mv, mc, L)[0]
    shell_pts = 4 * ((1 << L) + 1) * ((1 << L) + 2) // 2
    timeit("SOR shell forward (4 faces, 6 edges, 4 vertices)",
           lambda k: capi.p1_sor_shell_cell(p(B, k), p(A, k), p(Cc, k), L, T["edge_verts"], T["edge_w"], T["face_verts"], T["face_w"],
                                            T["vertex_w"], 1.0, 0x3FFF, False, sh), 40 * shell_pts, shell_pts, r=max(3, reps // 10))
    timeit("SOR shell backward", lambda k: capi.p1_sor_shell_cell(p(B, k), p(A, k), p(Cc, k), L, T["edge_verts"], T["edge_w"], T["face_verts"],
                                                                  T["face_w"], T["vertex_w"], 1.0, 0x3FFF, True, sh),
           40 * shell_pts, shell_pts, r=max(3, reps // 10))
    # the normal projection of the strong free-slip condition on tet_1el with all four faces selected: one launch for the
    # three components, beside three launches of the masked shell vector kernel (one add per component) that touch the same points
    ntab = torch.rand(3 * shell_pts, dtype=torch.float64, device="cuda") / 2  # | n | < 1: repeated projections do not grow
    timeit("project normal (u, v, w; 4 faces selected)",
           lambda k: capi.p1_project_normal_cells([p(A, k)], [p(B, k)], [p(Cc, k)], [ntab.data_ptr()], L, [0x3FFF], sh),
           72 * shell_pts, 3 * shell_pts)

    def project_yardstick(k):
        capi.p1_vector_cell_masked(1, p(A, k), [1e-3], [p(B, k)], L, 0x3FFF, sh)
        capi.p1_vector_cell_masked(1, p(B, k), [1e-3], [p(Cc, k)], L, 0x3FFF, sh)
        capi.p1_vector_cell_masked(1, p(Cc, k), [1e-3], [p(A, k)], L, 0x3FFF, sh)

    timeit("project yardstick: 3 masked shell vector launches", project_yardstick, 72 * shell_pts, 3 * shell_pts)
    del ntab
    # P2 elementwise Laplace apply on one macro-cell, level 7 as in BASELINE config 4
    L2 = min(L, 7)
    nv2, ne2 = capi.cell_size(L2), capi.p2_edge_array_size(L2)
    p2op = host.P2ElementwiseLaplaceOperator(st, L2, L2)  # element matrices (kernel input) from the host layer's P2LaplaceForm
    em = torch.from_numpy(capi.p2_build_operator_table(p2op.element_matrices(L2))).to("cuda")
    nb2 = max(2, -(-int(2.2 * 256 * 2**20) // ((nv2 + ne2) * 8)))  # the sources alone 2.2 x the Infinity Cache
    SV = [torch.rand(nv2, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    SE = [torch.rand(ne2, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    DV = [torch.zeros(nv2, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    DE = [torch.zeros(ne2, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    timeit(f"P2 elementwise Laplace apply, level {L2} ({nv2 + ne2} DoFs)",
           lambda k: capi.p2_elementwise_apply_cell(DV[k % nb2].data_ptr(), DE[k % nb2].data_ptr(), SV[k % nb2].data_ptr(),
                                                    SE[k % nb2].data_ptr(), L2, em.data_ptr(), 1.0, 0, 0x7FFF, sh),
           16 * (nv2 + ne2), nv2 + ne2, r=max(3, reps // 10))
    # P2 quadratic grid transfer between level L2 - 1 and L2
    nvc, nec = capi.cell_size(L2 - 1), capi.p2_edge_array_size(L2 - 1)
    CV = [torch.rand(nvc, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    CE = [torch.rand(nec, dtype=torch.float64, device="cuda") for _ in range(nb2)]
    timeit(f"P2 prolongate level {L2 - 1} -> {L2}",
           lambda k: capi.p2_prolongate_cell(DV[k % nb2].data_ptr(), DE[k % nb2].data_ptr(), CV[k % nb2].data_ptr(), CE[k % nb2].data_ptr(),
                                             L2 - 1, 0, 0x7FFF, sh), 8 * (nv2 + ne2 + nvc + nec), nv2 + ne2, r=max(3, reps // 10))
    timeit(f"P2 restrict level {L2} -> {L2 - 1}",
           lambda k: capi.p2_restrict_cell(CV[k % nb2].data_ptr(), CE[k % nb2].data_ptr(), SV[k % nb2].data_ptr(), SE[k % nb2].data_ptr(),
                                           L2 - 1, ones, 0x7FFF, sh), 8 * (nv2 + ne2 + nvc + nec), nvc + nec, r=max(3, reps // 10))
    # the same transfer on the small levels of a cycle, for the 24 macro-cells of cube_24el: the per-cell loop (24 launches) against one
    # batched launch; time, bytes and DoFs are those of all 24 cells
    ncell = 24
    inv24 = torch.ones(14 * ncell, dtype=torch.float64, device="cuda")
    for fine in (3, 6):
        nvf, nef, nvk, nek = capi.cell_size(fine), capi.p2_edge_array_size(fine), capi.cell_size(fine - 1), capi.p2_edge_array_size(fine - 1)
        FV, FE, KV, KE = ([torch.rand(m, dtype=torch.float64, device="cuda") for _ in range(ncell)] for m in (nvf, nef, nvk, nek))
        fv, fe, kv, ke = ([t.data_ptr() for t in ts] for ts in (FV, FE, KV, KE))
        masks24, nbytes = [0x7FFF] * ncell, 8 * ncell * (nvf + nef + nvk + nek)

        def restrict_loop(k):
            for c in range(ncell):
                capi.p2_restrict_cell(kv[c], ke[c], fv[c], fe[c], fine - 1, ones, 0x7FFF, sh)

        def prolongate_loop(k):
            for c in range(ncell):
                capi.p2_prolongate_cell(fv[c], fe[c], kv[c], ke[c], fine - 1, 0, 0x7FFF, sh)

        r24 = max(3, reps // 10)
        timeit(f"P2 restrict level {fine} -> {fine - 1}, 24 cells, per-cell loop", restrict_loop, nbytes, ncell * (nvk + nek), r=r24)
        timeit(f"P2 restrict level {fine} -> {fine - 1}, 24 cells, one batched launch",
               lambda k: capi.p2_restrict_cells(kv, ke, fv, fe, fine - 1, inv24.data_ptr(), masks24, sh), nbytes, ncell * (nvk + nek), r=r24)
        timeit(f"P2 prolongate level {fine - 1} -> {fine}, 24 cells, per-cell loop", prolongate_loop, nbytes, ncell * (nvf + nef), r=r24)
        timeit(f"P2 prolongate level {fine - 1} -> {fine}, 24 cells, one batched launch",
               lambda k: capi.p2_prolongate_cells(fv, fe, kv, ke, fine - 1, masks24, 0, sh), nbytes, ncell * (nvf + nef), r=r24)
    # P1 <-> P2 conversion at P2 level 7 (P1 level 8), both directions, beside hyteg_hip_copy of the same number of bytes in the same
    # run: a permutation, 8 bytes read and 8 written per DoF; information, no threshold is attached
    Lc = 7
    nvc7, nec7, np1 = capi.cell_size(Lc), capi.p2_edge_array_size(Lc), capi.cell_size(Lc + 1)
    assert nvc7 + nec7 == np1
    nbc = max(2, -(-int(2.2 * 256 * 2**20) // (np1 * 8)))
    P1s = [torch.rand(np1, dtype=torch.float64, device="cuda") for _ in range(nbc)]
    P2s = [torch.rand(np1, dtype=torch.float64, device="cuda") for _ in range(nbc)]  # vertex array, then the edge array, in one allocation
    pv = lambda k: P2s[k % nbc].data_ptr()  # noqa: E731
    pe = lambda k: P2s[k % nbc].data_ptr() + 8 * nvc7  # noqa: E731
    timeit(f"P1 -> P2 conversion, P2 level {Lc} ({np1} DoFs)", lambda k: capi.p1_to_p2_cell(pv(k), pe(k), P1s[k % nbc].data_ptr(), Lc, 0x7FFF, sh),
           16 * np1, np1)
    timeit(f"P2 -> P1 conversion, P2 level {Lc} ({np1} DoFs)", lambda k: capi.p2_to_p1_cell(P1s[k % nbc].data_ptr(), pv(k), pe(k), Lc, 0x7FFF, sh),
           16 * np1, np1)
    timeit(f"hyteg_hip_copy of the bytes of the conversion ({8 * np1} bytes)",
           lambda k: capi.check(capi.lib().hyteg_hip_copy(P2s[k % nbc].data_ptr(), P1s[k % nbc].data_ptr(), 8 * np1, sh), "copy"), 16 * np1, np1)
    del P1s, P2s
    if args.only:
        print(json.dumps({"level": L, "kernels": rows}))
        return
    # BASELINE config 4 shape on one GPU: P2 Laplace, level 7, the 6 macro-cells one GPU holds (cube_6el = the unit cube)
    if L >= 7:
        s6 = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/cube_6el.msh")
        s6.set_stream(sh)
        A6 = host.P2ElementwiseLaplaceOperator(s6, 7, 7)
        u6, r6 = host.P2Function(s6, "u", 7, 7), host.P2Function(s6, "r", 7, 7)
        u6.interpolate(1.0, 7)
        for _ in range(3):
            A6.apply(u6, r6, 7, host.Inner)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n6 = 10
        for _ in range(n6):
            A6.apply(u6, r6, 7, host.Inner)
        torch.cuda.synchronize()
        us6 = (time.perf_counter() - t0) / n6 * 1e6
        dofs6 = 6 * (nv2 + ne2)
        rows.append(dict(kernel="P2 elementwise apply, cube_6el, level 7, host layer (6 cells + exchange)", us=us6, GDoFps=dofs6 / us6 * 1e-3))
        print(f"P2 elementwise apply, cube_6el (6 macro-cells), level 7, host layer: {us6:9.1f} us  {dofs6 / us6 * 1e-3:7.1f} GDoF/s "
              f"({dofs6} DoFs incl. copies of shared ones)", flush=True)
        for o in (u6, r6, A6, s6):
            o.close()
    # V-cycles through the host layer
    # Chebyshev rows: ( order, fused ) instead of a smoother code; V(1,1), spectral radius 1.97 on every level (the time per cycle
    # does not depend on the bounds)
    for mesh, lo, hi, smoother, name in (("tet_1el", 2, L, host.JACOBI, "Jacobi(2/3)"), ("tet_1el", 2, L, host.JACOBI_FP32, "Jacobi fp32"),
                                          ("tet_1el", 2, min(L, 7), host.GAUSS_SEIDEL, "GS"),
                                          ("tet_1el", 2, L, (3, True), "Chebyshev(3)"), ("tet_1el", 2, L, (2, True), "Chebyshev(2)"),
                                          ("tet_1el", 2, L, (3, False), "Chebyshev(3) composed"),
                                          ("tet_1el", 2, min(L, 7), (3, True), "Chebyshev(3)"),
                                          ("regular_octahedron_8el", 2, min(L, 6), host.JACOBI, "Jacobi(2/3)"),
                                          ("regular_octahedron_8el", 0, min(L, 6), host.GAUSS_SEIDEL, "GS"),
                                          ("regular_octahedron_8el", 2, min(L, 6), (3, True), "Chebyshev(3)"),
                                          ("regular_octahedron_8el", 2, min(L, 6), (2, True), "Chebyshev(2)")):
        s2 = host.Storage.from_gmsh(ROOT / f"hyteg_amd/data/meshes/{mesh}.msh")
        s2.set_stream(sh)
        A2 = host.P1ConstantOperator(s2, lo, hi)
        A2.compute_inverse_diagonal()
        x, b, one = (host.P1Function(s2, nm, lo, hi) for nm in ("x", "b", "one"))
        one.interpolate(1.0, hi, host.All)
        dofs = one.dot(one, hi, host.Inner)
        rng = np.random.default_rng(0)
        for c in range(s2.n_local_cells):
            x.upload_cell(c, hi, rng.random(capi.cell_size(hi)))
        x.sync_shared(hi, host.All)
        x.interpolate(0.0, hi, host.DirichletBoundary)
        if isinstance(smoother, tuple):
            gmg = host.Solver.gmg_chebyshev(s2, lo, hi, smoother[0], 1.97, pre=1, post=1, cg_max_iter=50, cg_tol=1e-10)
            gmg.set_fused(smoother[1])
        else:
            gmg = host.Solver.gmg(s2, lo, hi, smoother=smoother, relax=2.0 / 3.0, pre=3, post=3, cg_max_iter=50, cg_tol=1e-10)
        vnu = "V(1,1)" if isinstance(smoother, tuple) else "V(3,3)"
        for _ in range(3):
            gmg.solve(A2, x, b, hi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ncyc = 5
        for _ in range(ncyc):
            gmg.solve(A2, x, b, hi)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / ncyc
        rows.append(dict(kernel=f"{vnu} {name} {mesh} L{lo}-{hi}", ms=ms, inner_dofs=dofs))
        print(f"{vnu} {name:21s} {mesh:24s} levels {lo}-{hi}: {ms:9.2f} ms/cycle, {dofs:.0f} inner DoFs "
              f"({dofs / ms * 1e-6:.2f} GDoF/s per cycle)", flush=True)
    # P1-P1 Stokes: the reference's P1P1Stokes3DUzawaConvergenceTest configuration (cube_24el, levels 2-5, V(3,3) increment 2, Uzawa)
    s3 = host.Storage.from_gmsh(ROOT / "hyteg_amd/data/meshes/cube_24el.msh")
    s3.set_stream(sh)
    Ls = host.P1P1StokesOperator(s3, 2, 5)
    us_, fs_ = host.P1StokesFunction(s3, "u", 2, 5), host.P1StokesFunction(s3, "f", 2, 5)
    for fn_ in (us_, fs_):
        for comp in fn_.components:
            comp.interpolate(0.0, 5, host.All)
    us_.u.interpolate(1.0, 5, host.DirichletBoundary)
    uz = host.StokesSolver.uzawa(s3, 2, 5, 0.3, velocity_iterations=2, velocity_smoother=host.GAUSS_SEIDEL)
    sg = host.StokesSolver.gmg(s3, uz, 2, 5, pre=3, post=3, increment=2)
    sg.solve(Ls, us_, fs_, 5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        sg.solve(Ls, us_, fs_, 5)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / 3
    rows.append(dict(kernel="Stokes V(3,3)+2 Uzawa/GS cube_24el L2-5", ms=ms))
    print(f"P1-P1 Stokes V(3,3) increment 2, Uzawa(0.3) over GS, cube_24el levels 2-5: {ms:9.2f} ms/cycle", flush=True)
    t0 = time.perf_counter()
    for _ in range(20):
        Ls.apply(us_, fs_, 5, host.Inner | host.NeumannBoundary)
    torch.cuda.synchronize()
    us1 = (time.perf_counter() - t0) * 1e6 / 20
    rows.append(dict(kernel="P1P1StokesOperator::apply cube_24el L5", us=us1))
    print(f"P1P1StokesOperator::apply, cube_24el level 5 (24 cells, 10 scalar applies): {us1:9.1f} us", flush=True)
    # P2-P1 Taylor-Hood (config 5's literal wording): the reference's P2P1Stokes3DUzawaConvergenceTest configuration (cube_24el, levels 2-3,
    # V(3,3), Uzawa(0.4) over Gauss-Seidel, MINRES on the coarsest level) and one level more; operator apply; one P2 Gauss-Seidel sweep
    for lo_t, hi_t in ((2, 3), (2, 4)):
        Lt = host.TaylorHoodStokesOperator(s3, lo_t, hi_t)
        ut, ft = host.TaylorHoodFunction(s3, "u", lo_t, hi_t), host.TaylorHoodFunction(s3, "f", lo_t, hi_t)
        ut.interpolate(0.0, hi_t, host.All)
        ft.interpolate(1.0, hi_t, host.Inner)
        th = host.TaylorHoodSolver.gmg(s3, lo_t, hi_t, uzawa_relax=0.4, pre=3, post=3, increment=0, coarse_max_iter=60, coarse_rel_tol=1e-16)
        th.solve(Lt, ut, ft, hi_t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            th.solve(Lt, ut, ft, hi_t)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 2 * 1e3
        rows.append(dict(kernel=f"Taylor-Hood V(3,3) Uzawa/GS cube_24el L{lo_t}-{hi_t}, MINRES(60) coarse", ms=ms))
        print(f"P2-P1 Taylor-Hood V(3,3), Uzawa(0.4) over GS, cube_24el levels {lo_t}-{hi_t}, MINRES(60) on the coarsest level: {ms:9.2f} ms/cycle", flush=True)
        t0 = time.perf_counter()
        for _ in range(10):
            Lt.apply(ut, ft, hi_t, host.Inner | host.NeumannBoundary)
        torch.cuda.synchronize()
        us1 = (time.perf_counter() - t0) * 1e6 / 10
        rows.append(dict(kernel=f"P2P1TaylorHoodStokesOperator::apply cube_24el L{hi_t}", us=us1))
        print(f"P2P1TaylorHoodStokesOperator::apply, cube_24el level {hi_t} (24 cells: 3 P2 Laplace + 3 divT + 3 div): {us1:9.1f} us", flush=True)
        for o in (th, ut, ft, Lt):
            o.close()
    A2g = host.P2ConstantLaplaceOperator(s3, 4, 4)
    A2g.compute_inverse_diagonal()
    xg, bg = host.P2Function(s3, "x", 4, 4), host.P2Function(s3, "b", 4, 4)
    xg.interpolate(0.0, 4, host.All)
    bg.interpolate(1.0, 4, host.Inner)
    A2g.smooth_sor(xg, bg, 1.0, 4, host.Inner)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        A2g.smooth_sor(xg, bg, 1.0, 4, host.Inner)
    torch.cuda.synchronize()
    usg = (time.perf_counter() - t0) * 1e6 / 5
    rows.append(dict(kernel="P2 Gauss-Seidel sweep (reference order on shared primitives) cube_24el L4", us=usg))
    print(f"P2 Gauss-Seidel sweep in the reference's order, cube_24el level 4 (24 cells): {usg:9.1f} us", flush=True)
    print(json.dumps({"level": L, "device": capi.device_name(), "rows": rows}))


if __name__ == "__main__":
    main()
