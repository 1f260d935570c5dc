"""The three branches of the P2 apply dispatch that only a variable read at first use reaches, each in a fresh child process that
sets one of them, against the same calls in a child that sets none:
  HYTEG_HIP_P2_INNER_THREADS=1  thread-per-DoF inner kernel + boundary kernel instead of the row kernels
  HYTEG_HIP_P2_ROWS_DPP=0       p2_rows_body (every source loaded) instead of p2_rows_body_dpp (every source row loaded once)
  HYTEG_HIP_P2_XCD_ROWS=0       row blocks in launch order instead of one chunk of the cell per XCD
One macro-cell (the vertices of hyteg_amd/data/meshes/tet_1el.msh, in node order), levels 3 (the first with row kernels) and 5 (the first whose row grid
reaches 64 blocks, so the XCD-chunk branch is taken), hyteg_hip_p2_set_class_rows_min_level( 99 ) so that the row branch is reached;
the full apply with Replace and with Add, then one apply restricted to the kind XY (kind_mask = 1 << 4).

HYTEG_HIP_P2_ROWS_DPP=0 and HYTEG_HIP_P2_XCD_ROWS=0 give bit-identical arrays for every call (the two row forms read the same sources
and sum them in the same order, the XCD chunks only reorder the blocks), and so does HYTEG_HIP_P2_INNER_THREADS=1 for the two Replace
calls (the row kernels sum each DoF's entries in the order and with the FMAs of the thread-per-DoF kernel): those assert equality.
The Add call under HYTEG_HIP_P2_INNER_THREADS=1 differs in the last bit (relative L2 3e-17 .. 5e-17: the thread-per-DoF kernel
contracts dst + alpha * sum into one FMA, the row kernel rounds alpha * sum first) and is held to the project's fp64 parity bound,
relative L2 <= 1e-12.  The relative L2 difference of every array is printed before the assertions."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SWITCHES = {"HYTEG_HIP_P2_INNER_THREADS": "1", "HYTEG_HIP_P2_ROWS_DPP": "0", "HYTEG_HIP_P2_XCD_ROWS": "0"}
LEVELS = (3, 5)
CALLS = (("full_replace", 0, 0xFF), ("full_add", 1, 0xFF), ("kind_xy", 0, 1 << 4))
ROUNDED = {("HYTEG_HIP_P2_INNER_THREADS", "full_add")}  # every other (variable, call) is bit-identical to the default branch


def _child(outdir):
    """the applies of one process; whatever switch the environment carries is read by the library at its first use here"""
    sys.path.insert(0, str(ROOT))
    import torch

    from hyteg_amd import capi
    from oracle import p1_oracle as po

    sys.path.insert(0, str(ROOT / "tests"))
    import hostutil as hu

    tet = hu.read_msh(hu.MESHES / "tet_1el.msh")[0]
    assert tet.shape == (4, 3)
    capi.lib()
    capi.p2_set_class_rows_min_level(99)
    for level in LEVELS:
        nv, ne = capi.cell_size(level), capi.p2_edge_array_size(level)
        em = po.p2_cell_element_matrices(np.asarray(tet, dtype=np.float64).reshape(12), level)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        table = dev(capi.p2_build_operator_table(em))
        rng = np.random.default_rng(500 + level)
        sv, se, dv0, de0 = (dev(rng.standard_normal(n)) for n in (nv, ne, nv, ne))
        for name, update, kinds in CALLS:
            dv, de = dv0.clone(), de0.clone()
            capi.p2_elementwise_apply_cell(dv.data_ptr(), de.data_ptr(), sv.data_ptr(), se.data_ptr(), level, table.data_ptr(), 1.25, update, 0x7FFF,
                                           kinds=kinds)
            torch.cuda.synchronize()
            np.save(Path(outdir) / f"l{level}_{name}_v.npy", dv.cpu().numpy())
            np.save(Path(outdir) / f"l{level}_{name}_e.npy", de.cpu().numpy())


def _run_child(outdir, extra_env):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra_env)
    outdir.mkdir()
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outdir)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return {(level, name, a): np.load(outdir / f"l{level}_{name}_{a}.npy") for level in LEVELS for name, _, _ in CALLS for a in "ve"}


@pytest.fixture(scope="module")
def unswitched(tmp_path_factory):
    return _run_child(tmp_path_factory.mktemp("p2_switches") / "default", {})


@pytest.mark.gpu
@pytest.mark.parametrize("variable", sorted(SWITCHES))
def test_p2_apply_switch_branch_equals_the_default_branch(unswitched, tmp_path, variable):
    got = _run_child(tmp_path / "switched", {variable: SWITCHES[variable]})
    assert sorted(got) == sorted(unswitched)
    for key in sorted(got):
        a, b = got[key], unswitched[key]
        print(variable, key, "relative L2 difference", np.linalg.norm(a - b) / np.linalg.norm(b))
    for key in sorted(got):
        a, b = got[key], unswitched[key]
        assert np.isfinite(b).all() and np.linalg.norm(b) > 0.0
        if (variable, key[1]) in ROUNDED:
            assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), (variable, key)
        else:
            assert np.array_equal(a, b), (variable, key)


if __name__ == "__main__":
    _child(sys.argv[1])
