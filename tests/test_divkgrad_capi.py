"""CPU-only: the C-ABI entry points of the variable-coefficient operator -div( k grad u ) are declared, bound, and reject bad
arguments on the host with EINVAL before any GPU work (made-up addresses: nothing is dereferenced on the host)."""
import re
from pathlib import Path

import pytest

from conftest import SKEW_TET

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked", "hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d",
                "hyteg_hip_p1_elementwise_divkgrad_diagonal_macro_3d")
A, B, K, R, D = 4096, 8192, 12288, 16384, 20480  # made-up device addresses


def test_entry_points_are_declared_and_bound():
    from hyteg_amd import capi

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert hasattr(capi.lib(), name)


def test_apply_rejects_bad_arguments_on_the_host():
    from hyteg_amd import capi

    f = capi.p1_elementwise_divkgrad_apply_macro_3d_masked
    for dst, src, k in ((None, B, K), (A, None, K), (A, B, None)):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            f(dst, src, k, SKEW_TET, 16)
    lib = capi.lib()
    assert lib.hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked(A, B, K, None, 16, capi.MASK_ALL, capi.REPLACE, 0) == 1  # EINVAL
    with pytest.raises(capi.HytegHipError, match="power of two, at most 2\\^8"):
        f(A, B, K, SKEW_TET, 1 << 9)
    with pytest.raises(capi.HytegHipError, match="power of two"):
        f(A, B, K, SKEW_TET, 12)
    with pytest.raises(capi.HytegHipError, match="alias"):
        f(A, A, K, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="alias"):
        f(A, B, A, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="bad update"):
        f(A, B, K, SKEW_TET, 16, update=7)
    with pytest.raises(capi.HytegHipError, match="bad mask"):
        f(A, B, K, SKEW_TET, 16, mask=1 << 15)
    flat = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0))
    with pytest.raises(capi.HytegHipError, match="degenerate"):
        f(A, B, K, flat, 16)


def test_jacobi_and_diagonal_reject_bad_arguments_on_the_host():
    from hyteg_amd import capi

    j = capi.p1_elementwise_divkgrad_jacobi_macro_3d
    for args in ((None, B, R, D, K), (A, None, R, D, K), (A, B, None, D, K), (A, B, R, None, K), (A, B, R, D, None)):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            j(*args, SKEW_TET, 16, 0.6)
    for args in ((A, A, R, D, K), (A, B, A, D, K), (A, B, R, A, K), (A, B, R, D, A)):
        with pytest.raises(capi.HytegHipError, match="alias"):
            j(*args, SKEW_TET, 16, 0.6)
    with pytest.raises(capi.HytegHipError, match="at most 2\\^8"):
        j(A, B, R, D, K, SKEW_TET, 1 << 9, 0.6)
    d = capi.p1_elementwise_divkgrad_diagonal_macro_3d
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        d(None, K, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        d(A, None, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="alias"):
        d(A, A, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="at most 2\\^8"):
        d(A, K, SKEW_TET, 1 << 9)
    with pytest.raises(capi.HytegHipError, match="not compiled in"):
        capi.p1_elementwise_divkgrad_set_shape(3, 5)
    capi.p1_elementwise_divkgrad_set_shape(0, 0)
