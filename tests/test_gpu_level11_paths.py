"""The code that level 11 (11.5 GB per array, beyond 32-bit buffer addressing) runs instead of the z-march and brick kernels, entry by
entry against the CPU oracle at levels 2..7, where a whole array can be compared:
  p1_apply_tiled_kernel (kernels_apply.hpp)       the LDS-tiled apply / fused Jacobi, both staging forms (VEC = true / false)
  the composed branches of hyteg_hip_p1_chebyshev_start_cell / _step_cell (p1_apply.hip)
  p1_prolongate_kernel (p1_transfer.hip)          the tile prolongation, several tiles per slice
HYTEG_HIP_APPLY_LDS_TILED=1 and HYTEG_HIP_TRANSFER_TILES=1 select them at every level; the library reads both once, at first use, so
this file is its own child program: the parent starts it twice, with neither variable (the z-march and brick kernels, the same calls: the
baseline) and with both.  Each child compares what it computes with oracle/p1_oracle.py itself, prints every figure, writes the arrays
as .npy and leaves with a non-zero status if a comparison failed; the parent compares the two children.

Bounds: relative L2 <= 1e-13 over the entries a kernel owns for apply, Jacobi and prolongation (TOL of test_gpu_parity.py), <= 1e-12
for the Chebyshev steps (test_gpu_chebyshev.py); every entry a kernel does not own keeps its bits.

Source and destination arrays sit inside larger device buffers, GUARD entries on each side.  The source's bands hold NaN, so whatever
a kernel stages from beyond either end of the array and then uses shows in the result.  The destination's bands hold a sentinel and
are compared afterwards.  Replace and Jacobi must not read dst: its interior entries are NaN before those calls.
(Every cell array has an odd number of entries, and stage_span has a branch for a last 16-byte pair that straddles the end of the array.
With the tiles of the interior that branch is never taken: the last entry any tile stages -- the stencil's top neighbours of the
interior point below the tip, rounded up to an odd index -- lies 5 entries before the end of the array at every level.  So removing
the `lo + k < total` guard or the `lds[k + 1] = 0.0` line changes no result here or at level 11, and no test of results can notice.)

Composed Chebyshev steps: besides chebyshevutil.kernel_case, the switched child repeats each step as the explicit sequence of C-ABI
calls in the order of the fallback's code (p1_apply_cell, p1_assign_cell, p1_mult_cell, p1_add_cell).  The fallback IS that sequence, so
the arrays are equal bit for bit.  Each child prints whether its result has the bits of that sequence, the parent in how many arrays
the two children differ.  Recorded on the MI355X: the baseline child's fused z-march kernel ALSO has the bits of its own sequence
(z-march apply, then the vector kernels) in all 36 arrays, so equality inside one process does not tell fused from composed; what
tells them apart is the apply kernel underneath -- the tiled and the z-march apply sum in different orders, and the two children's
Chebyshev arrays differ in bits at levels 4 and 6 (24 of 36 arrays, relative L2 1e-17 .. 7e-17; level 2 has the same bits).  A
switched child whose Chebyshev entry points ignored the switch would compare the fused z-march result with a sequence built on the
tiled apply, and fail there."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SWITCHES = {"HYTEG_HIP_APPLY_LDS_TILED": "1", "HYTEG_HIP_TRANSFER_TILES": "1"}
TOL, TOL_CHEB = 1e-13, 1e-12
GUARD = 64  # entries on each side of a banded array
SENTINEL = -77.25
NAME_LEVELS = (2, 5, 8)
APPLY_LEVELS = (2, 3, 4, 5, 6, 7)  # 6: the first level with more than one tile per slice; 7: tiles of ~8 rows that start and end mid-row
RANDOM_WEIGHT_LEVELS = (3, 6)
APPLY_MODES = ("replace", "add", "jacobi", "jacobi_invdiag")
CHEB_LEVELS = (2, 4, 6)
FINE_LEVELS = (4, 5, 6, 7)  # the fine levels whose default prolongation is the brick kernel
NNC_MIXED = [3, 4, 5, 6, 7, 8, 2, 1, 2, 2, 9, 10, 11, 12]
MASKS = (0x7FFF, (1 << 14) | 0x03C0, 0x3FFF)
RELAX = 0.6


class _Checks:
    """every figure is printed before it is judged; the child goes on after a failure and reports all of them at the end"""

    def __init__(self):
        self.failed = []

    def rel(self, what, got, want, tol):
        nw = float(np.linalg.norm(want))
        err = float(np.linalg.norm(got - want)) / (nw if nw > 0 else 1.0)
        print(f"{what}: relative L2 error {err:.3e} (bound {tol:.0e})")
        if not (np.isfinite(got).all() and err <= tol):
            self.failed.append(f"{what}: relative L2 error {err!r} > {tol!r}, or a non-finite entry")

    def same(self, what, got, want):
        if not np.array_equal(got, want):
            self.failed.append(f"{what}: {int(np.count_nonzero(got != want))} entries differ in bits")

    def true(self, what, cond):
        if not cond:
            self.failed.append(what)


def _child(mode, outdir):
    """everything one process computes; whichever switches the environment carries are read by the library at its first use here"""
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import torch

    import chebyshevutil as cu
    from conftest import SKEW_TET
    from hyteg_amd import capi
    from oracle import p1_oracle as po

    switched = mode == "switched"
    assert switched == all(os.environ.get(k) == v for k, v in SWITCHES.items())
    assert switched or not any(k in os.environ for k in SWITCHES)
    capi.lib()
    ck = _Checks()
    out = {}
    t0 = time.perf_counter()

    def banded(values, fill, offset=GUARD):
        """device buffer [fill x offset | values | fill x GUARD]; returns (buffer, view of the values)"""
        n = values.size
        host = np.full(offset + n + GUARD, fill)
        host[offset:offset + n] = values
        buf = torch.from_numpy(host).cuda()
        return buf, buf[offset:offset + n]

    def bands_intact(what, buf, n, fill, offset=GUARD):
        h = buf.cpu().numpy()
        ck.same(f"{what}: band in front of the array", h[:offset], np.full(offset, fill))
        ck.same(f"{what}: band behind the array", h[offset + n:], np.full(GUARD, fill))

    # ---- a. which kernel the apply dispatch names
    names = {level: capi.p1_apply_kernel_name(level) for level in NAME_LEVELS}
    names[f"{NAME_LEVELS[1]} add"] = capi.p1_apply_kernel_name(NAME_LEVELS[1], capi.ADD)
    prefix = "p1_apply_tiled_kernel" if switched else "p1_apply_zmarch_preload_kernel"
    for key, name in names.items():
        print(f"apply kernel at level {key}: {name}")
        ck.true(f"level {key} reports {name}, expected {prefix}*", name.startswith(prefix))
    (Path(outdir) / "names.json").write_text(json.dumps({str(k): v for k, v in names.items()}))

    # ---- b. apply (Replace, Add) and fused Jacobi (centre weight / inverse-diagonal array), 16-byte and 8-byte aligned source
    def apply_case(level, wname, w, amode, aligned, save=True):
        key = f"apply l{level} {wname} {amode} {'vec' if aligned else 'scalar'}"
        n = po.cell_size(level)
        m = po.inner_mask(level)
        rng = np.random.default_rng([level, len(wname), APPLY_MODES.index(amode), int(aligned)])
        src_h, rhs_h, dst0_h = rng.random(n), rng.random(n), rng.random(n)
        inv_h = (0.5 + rng.random(n)) / abs(w[7])
        if amode != "add":
            dst0_h[m] = np.nan  # Replace and Jacobi do not read dst
        offset = GUARD if aligned else GUARD + 1
        sbuf, src = banded(src_h, np.nan, offset)
        assert src.data_ptr() % 16 == (0 if aligned else 8)
        dbuf, dst = banded(dst0_h, SENTINEL)
        rhs, inv = torch.from_numpy(rhs_h).cuda(), torch.from_numpy(inv_h).cuda()
        ref = np.where(m, 0.0, dst0_h) if amode != "add" else dst0_h.copy()
        if amode in ("replace", "add"):
            update = capi.REPLACE if amode == "replace" else capi.ADD
            capi.p1_apply_cell(dst.data_ptr(), src.data_ptr(), level, w, update)
            po.apply_cell(ref, src_h, level, w, update)
        else:
            invdiag = amode == "jacobi_invdiag"
            capi.p1_jacobi_cell(dst.data_ptr(), rhs.data_ptr(), src.data_ptr(), level, w, RELAX, inv.data_ptr() if invdiag else None)
            po.jacobi_cell(ref, rhs_h, src_h, level, w, RELAX, inv_h if invdiag else None)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        ck.rel(key, got[m], ref[m], TOL)
        ck.same(f"{key}: entries outside the cell interior", got[~m], dst0_h[~m])
        bands_intact(key, dbuf, n, SENTINEL)
        sh = sbuf.cpu().numpy()
        ck.true(f"{key}: the source changed", np.array_equal(sh[offset:offset + n], src_h) and np.isnan(sh[:offset]).all() and np.isnan(sh[offset + n:]).all())
        if save:
            out[key] = got
        return got

    for level in APPLY_LEVELS:
        weights = [("skew", po.assemble_cell_stencil(SKEW_TET, level))]
        if level in RANDOM_WEIGHT_LEVELS:
            weights.append(("random", np.random.default_rng(50 + level).standard_normal(15)))  # non-symmetric: a swapped slot shows
        for wname, w in weights:
            for amode in APPLY_MODES:
                for aligned in (True, False):
                    apply_case(level, wname, w, amode, aligned)
    # e. the brick shape is a knob of the z-march: the tiled path ignores it
    if switched:
        capi.set_apply_shape(4, 8, 2)
        try:
            again = apply_case(6, "skew", po.assemble_cell_stencil(SKEW_TET, 6), "replace", True, save=False)
        finally:
            capi.set_apply_shape(0, 0, 0)
        ck.same("tiled Replace at level 6 under set_apply_shape(4, 8, 2)", again, out["apply l6 skew replace vec"])
    print(f"apply and Jacobi: {time.perf_counter() - t0:.1f} s")

    # ---- c. the Chebyshev steps: against the oracle (kernel_case), and against the explicit sequence of C-ABI calls
    t1 = time.perf_counter()
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    for level in CHEB_LEVELS:
        for function_inverse in (False, True):
            for has_prev in (False, True):
                key = f"chebyshev l{level} function_inverse={function_inverse} has_prev={has_prev}"
                keep = {}
                try:
                    errs = cu.kernel_case(torch, capi, SKEW_TET, level, function_inverse, has_prev, seed=level, keep=keep)
                except AssertionError as e:
                    ck.failed.append(f"{key}: {e}")
                    continue
                print(f"{key}: {errs}")
                for what, e in errs.items():
                    ck.true(f"{key} {what}: relative L2 error {e!r} > {TOL_CHEB!r}", e <= TOL_CHEB)
                w, x0, rhs, t_in, junk, inv = cu.kernel_inputs(SKEW_TET, level, function_inverse, level)
                inv_d = dev(inv)
                x_d, rhs_d, t_d = dev(x0), dev(rhs), dev(junk)
                capi.p1_apply_cell(t_d.data_ptr(), x_d.data_ptr(), level, w, capi.REPLACE)
                capi.p1_assign_cell(t_d.data_ptr(), [1.0, -1.0], [rhs_d.data_ptr(), t_d.data_ptr()], level)
                if function_inverse:
                    capi.p1_mult_cell(t_d.data_ptr(), [inv_d.data_ptr(), t_d.data_ptr()], level)
                else:
                    capi.p1_assign_cell(t_d.data_ptr(), [1.0 / w[7]], [t_d.data_ptr()], level)
                torch.cuda.synchronize()
                composed = {"start t_out": t_d.cpu().numpy()}
                x_d, tin_d, t_d = dev(x0), dev(t_in), dev(junk)
                capi.p1_apply_cell(t_d.data_ptr(), tin_d.data_ptr(), level, w, capi.REPLACE)
                if function_inverse:
                    capi.p1_mult_cell(t_d.data_ptr(), [inv_d.data_ptr(), t_d.data_ptr()], level)
                else:
                    capi.p1_assign_cell(t_d.data_ptr(), [1.0 / w[7]], [t_d.data_ptr()], level)
                if has_prev:
                    capi.p1_add_cell(x_d.data_ptr(), [cu.C_PREV], [tin_d.data_ptr()], level)
                capi.p1_add_cell(x_d.data_ptr(), [cu.C_CUR], [t_d.data_ptr()], level)
                torch.cuda.synchronize()
                composed["step t_out"], composed["step x"] = t_d.cpu().numpy(), x_d.cpu().numpy()
                for what in sorted(composed):
                    equal = np.array_equal(keep[what], composed[what])
                    print(f"{key} {what}: {'the same bits as' if equal else 'differs in bits from'} the explicit sequence of C-ABI calls")
                    if switched:
                        ck.true(f"{key} {what}: the composed branch is not the sequence of its C-ABI calls", equal)
                    out[f"{key} {what}"] = keep[what]
    print(f"Chebyshev steps: {time.perf_counter() - t1:.1f} s")

    # ---- d. prolongation onto fine levels 4..7
    t1 = time.perf_counter()
    for fine_level in FINE_LEVELS:
        lc = fine_level - 1
        nf = po.cell_size(fine_level)
        rng = np.random.default_rng(70 + fine_level)
        coarse_h, fine0_h = rng.random(po.cell_size(lc)), rng.random(nf)
        coarse = torch.from_numpy(coarse_h).cuda()
        slots = po.slot_of_points(fine_level)
        for nname, nnc in (("ones", [1] * 14), ("mixed", NNC_MIXED)):
            for uname, update in (("replace", capi.REPLACE), ("add", capi.ADD)):
                key = f"prolongate l{fine_level} nnc={nname} {uname}"
                fbuf, fine = banded(fine0_h, SENTINEL)
                capi.p1_prolongate_cell(coarse.data_ptr(), fine.data_ptr(), lc, nnc, update)
                torch.cuda.synchronize()
                ref = fine0_h.copy()
                po.prolongate_prepare(ref, fine_level, update)
                po.prolongate_cell(coarse_h, ref, lc, np.array(nnc, dtype=np.float64))
                got = fine.cpu().numpy()
                ck.rel(key, got, ref, TOL)
                bands_intact(key, fbuf, nf, SENTINEL)
                out[key] = got
        full = np.zeros(nf)
        po.prolongate_cell(coarse_h, full, lc, np.array(NNC_MIXED, dtype=np.float64))
        for mask in MASKS:
            key = f"prolongate l{fine_level} mask={mask:#06x}"
            sel = ((mask >> slots) & 1).astype(bool)
            fbuf, fine = banded(fine0_h, SENTINEL)
            capi.p1_prolongate_cell_masked(coarse.data_ptr(), fine.data_ptr(), lc, NNC_MIXED, mask)
            torch.cuda.synchronize()
            got = fine.cpu().numpy()
            ck.rel(key, got[sel], full[sel], TOL)
            ck.same(f"{key}: entries the mask does not select", got[~sel], fine0_h[~sel])
            bands_intact(key, fbuf, nf, SENTINEL)
            out[key] = got
        ck.same(f"prolongate l{fine_level}: the coarse array changed", coarse.cpu().numpy(), coarse_h)
    print(f"prolongation: {time.perf_counter() - t1:.1f} s")

    for k, key in enumerate(sorted(out)):
        np.save(Path(outdir) / f"{k:03d}.npy", out[key])
    (Path(outdir) / "keys.json").write_text(json.dumps(sorted(out)))
    print(f"{mode} child: {len(out)} arrays, {time.perf_counter() - t0:.1f} s, {len(ck.failed)} failed comparisons")
    for f in ck.failed:
        print("FAILED", f)
    return 1 if ck.failed else 0


def _run_child(mode, outdir):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if mode == "switched":
        env.update(SWITCHES)
    outdir.mkdir()
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), mode, str(outdir)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(f"{mode} child: {time.perf_counter() - t0:.1f} s wall")
    assert r.returncode == 0, r.stdout + r.stderr
    keys = json.loads((outdir / "keys.json").read_text())
    return {key: np.load(outdir / f"{k:03d}.npy") for k, key in enumerate(keys)}, json.loads((outdir / "names.json").read_text())


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    return _run_child("baseline", tmp_path_factory.mktemp("level11_paths") / "baseline")


@pytest.fixture(scope="module")
def switched(tmp_path_factory):
    return _run_child("switched", tmp_path_factory.mktemp("level11_paths") / "switched")


@pytest.mark.gpu
def test_default_kernels_pass_the_same_calls(baseline):
    """the z-march and brick kernels on the banded arrays of this file: the child's own comparisons with the oracle"""
    arrays, names = baseline
    assert all(n.startswith("p1_apply_zmarch_preload_kernel") for n in names.values()), names


@pytest.mark.gpu
def test_level_11_paths_match_the_oracle_at_small_levels(switched):
    """tiled apply and Jacobi, the composed Chebyshev steps and the tile prolongation: the child's own comparisons with the oracle"""
    arrays, names = switched
    assert all(n.startswith("p1_apply_tiled_kernel") for n in names.values()), names
    assert names[str(NAME_LEVELS[1])] != names[f"{NAME_LEVELS[1]} add"]


@pytest.mark.gpu
def test_both_children_made_the_same_calls_and_agree(baseline, switched):
    base, _ = baseline
    sw, _ = switched
    assert sorted(base) == sorted(sw)
    assert len([k for k in base if k.startswith("apply")]) == (len(APPLY_LEVELS) + len(RANDOM_WEIGHT_LEVELS)) * len(APPLY_MODES) * 2
    assert len([k for k in base if k.startswith("chebyshev")]) == len(CHEB_LEVELS) * 4 * 3
    assert len([k for k in base if k.startswith("prolongate")]) == len(FINE_LEVELS) * (4 + len(MASKS))
    worst, identical = {}, {}
    for key in sorted(base):
        a, b = sw[key], base[key]
        assert a.shape == b.shape
        # the oracle's arrays are finite wherever a kernel writes; what is left of dst's NaN interior is a failure of the child already
        assert np.isfinite(b).all() and np.isfinite(a).all(), key
        d = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        group = key.split()[0]
        worst[group] = max(worst.get(group, 0.0), d)
        same, total = identical.get(group, (0, 0))
        identical[group] = (same + int(np.array_equal(a, b)), total + 1)
        print(f"{key}: switched against baseline, relative L2 difference {d:.3e}{' (the same bits)' if np.array_equal(a, b) else ''}")
    for group in sorted(worst):
        print(f"{group}: largest relative L2 difference {worst[group]:.3e}, {identical[group][0]} of {identical[group][1]} arrays bit-identical")
    cheb = [k for k in base if k.startswith("chebyshev")]
    print("the fused Chebyshev kernels differ in bits from the composed steps in", sum(not np.array_equal(sw[k], base[k]) for k in cheb), "of", len(cheb),
          "arrays")
    for key in sorted(base):
        if key.startswith("prolongate"):
            assert np.linalg.norm(sw[key] - base[key]) <= TOL * np.linalg.norm(base[key]), key


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1], sys.argv[2]))
