"""CPU-only: the fused residual, Jacobi and Chebyshev entry points of the two P2 variable-coefficient operators (the epsilon operator and
div-k-grad, include/hyteg_hip.h sections b-4 (P2) and b-4 (P2 epsilon)) are declared with the reference lines they stand for, exported by
the cross-compiled library, bound, and reject bad arguments on the host with EINVAL before any GPU work (made-up addresses: nothing is
dereferenced on the host)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
OPS = ("epsilon", "divkgrad")
MODES = ("residual", "jacobi", "chebyshev_start", "chebyshev_step")
ENTRY_POINTS = tuple(f"hyteg_hip_p2_elementwise_{op}_{mode}_cell{form}" for op in OPS for mode in MODES for form in ("", "_gather"))
# made-up device addresses, a ( vertex, edge ) pair of three components each: dst / t_out, x, src / t_in, rhs, inverse diagonal
D = ((4096, 8192, 12288), (16384, 20480, 24576))
X = ((28672, 32768, 36864), (40960, 45056, 49152))
S = ((53248, 57344, 61440), (65536, 69632, 73728))
R = ((77824, 81920, 86016), (90112, 94208, 98304))
I = ((102400, 106496, 110592), (114688, 118784, 122880))
COEF = (126976, 131072)
GEOMETRY = {"epsilon": [1.0] * 72, "divkgrad": [1.0] * 60}
USED = {"residual": (0, 2, 3), "jacobi": (0, 2, 3, 4), "chebyshev_start": (0, 2, 3, 4), "chebyshev_step": (0, 1, 2, 4)}  # positions in GOOD
WRITTEN = {"residual": (0,), "jacobi": (0,), "chebyshev_start": (0,), "chebyshev_step": (0, 1)}
GOOD = (D, X, S, R, I)


def test_entry_points_are_declared_exported_and_bound():
    from hyteg_amd import capi

    assert len(ENTRY_POINTS) == 16
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert hasattr(raw, name), f"{name} not exported by the library"
        assert hasattr(capi.lib(), name)
    for mode in MODES:
        assert hasattr(capi, f"p2_varcoef_{mode}_cell")


def test_header_comments_cite_the_reference_lines_and_integration_shows_the_entries():
    text = (ROOT / "include" / "hyteg_hip.h").read_text()
    for start, end in (("b-4 (P2), fused modes", "b-4 (P2 epsilon):"), ("b-4 (P2 epsilon), fused modes", "b-5:")):
        section = text[text.index(start):text.index(end)]
        for cited in ("GeometricMultigridSolver.hpp:240-246", "P2ElementwiseOperator.cpp:344-374", "ChebyshevSmoother.hpp:165-212",
                      "hyteg_hip_p1_chebyshev_step_cell"):
            assert cited in section, (start, cited)
    integration = (ROOT / "INTEGRATION.md").read_text()
    for op in OPS:
        for mode in MODES:
            assert f"hyteg_hip_p2_elementwise_{op}_{mode}_cell" in integration


def replaced(t, k, v):
    return tuple(v if i == k else x for i, x in enumerate(t))


def call(capi, op, mode, gather, d, x, s, r, i, coef=COEF, level=3, geometry="default", mask=0x7FFF):
    """the entry of ( op, mode ) on ( dst / t_out, x, src / t_in, rhs, inv_diag ), each a ( vertex, edge ) pair of three addresses
    (div-k-grad takes the first of each)"""
    if op == "divkgrad":
        d, x, s, r, i = (tuple(None if a is None else a[0] for a in pair) for pair in (d, x, s, r, i))
    geometry = GEOMETRY[op] if geometry == "default" else geometry
    kw = dict(mask=mask, gather=gather)
    if mode == "residual":
        capi.p2_varcoef_residual_cell(op, d, s, r, coef, level, geometry, **kw)
    elif mode == "jacobi":
        capi.p2_varcoef_jacobi_cell(op, d, s, r, i, coef, level, geometry, 0.6, **kw)
    elif mode == "chebyshev_start":
        capi.p2_varcoef_chebyshev_start_cell(op, d, s, r, i, coef, level, geometry, **kw)
    else:
        capi.p2_varcoef_chebyshev_step_cell(op, d, x, s, i, coef, level, geometry, 0.5, -0.25, 1, **kw)


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
def test_bad_arguments_are_rejected_on_the_host(op, mode, gather):
    from hyteg_amd import capi

    def refused(match, *args, **kw):
        with pytest.raises(capi.HytegHipError, match=r"code 1\).*" + match):
            call(capi, op, mode, gather, *args, **kw)

    # null pointers: a whole operand, one array of a pair, one component of an array, the coefficient, the geometry, the masks
    for pos in USED[mode]:
        for half in (0, 1):
            refused("null pointer", *replaced(GOOD, pos, replaced(GOOD[pos], half, None)))
            if op == "epsilon":
                for k in range(3):
                    refused("null pointer", *replaced(GOOD, pos, replaced(GOOD[pos], half, replaced(GOOD[pos][half], k, None))))
    for half in (0, 1):
        refused("null pointer", *GOOD, coef=replaced(COEF, half, None))
    refused("null pointer", *GOOD, geometry=None)
    if op == "epsilon":
        refused("null pointer", *GOOD, mask=None)
    for level in (-1, 9, 12):
        refused("level out of range", *GOOD, level=level)
    # a written array against every other array of the call and against the coefficient, in every component
    ncomp = 3 if op == "epsilon" else 1
    for w in WRITTEN[mode]:
        for half in (0, 1):
            for k in range(ncomp):
                others = [COEF[0], COEF[1]]
                for pos in USED[mode]:
                    for h in (0, 1):
                        others += [a for kk, a in enumerate(GOOD[pos][h][:ncomp]) if (pos, h, kk) != (w, half, k)]
                for other in others:
                    refused("alias", *replaced(GOOD, w, replaced(GOOD[w], half, replaced(GOOD[w][half], k, other))))
    # an input that is the coefficient
    for pos in USED[mode]:
        if pos in WRITTEN[mode]:
            continue
        for half in (0, 1):
            for k in range(ncomp):
                refused("alias", *replaced(GOOD, pos, replaced(GOOD[pos], half, replaced(GOOD[pos][half], k, COEF[half]))))


@pytest.mark.parametrize("op", OPS)
def test_empty_masks_return_ok_without_a_launch(op):
    """nothing is launched (there is no GPU here, and the addresses are made up): the call returns OK"""
    from hyteg_amd import capi

    for mode in MODES:
        for gather in (False, True):
            call(capi, op, mode, gather, *GOOD, mask=0)
            if op == "epsilon":
                call(capi, op, mode, gather, *GOOD, mask=[0, 0, 0])
    capi.p2_varcoef_residual_cell(op, *(tuple(a if op == "epsilon" else a[0] for a in pair) for pair in (D, S, R)), COEF, 3, GEOMETRY[op], kinds=0)
