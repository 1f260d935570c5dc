"""CPU-only: the C-ABI entry points of the epsilon operator -div( 2 mu eps(u) ) are declared, exported and bound, and reject bad
arguments on the host with EINVAL before any GPU work (made-up addresses: nothing is dereferenced on the host)."""
import ctypes
import re
from pathlib import Path

import pytest

from conftest import SKEW_TET

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_masked", "hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d",
                "hyteg_hip_p1_elementwise_epsilon_diagonal_macro_3d", "hyteg_hip_p1_elementwise_epsilon_set_shape",
                "hyteg_hip_p1_elementwise_epsilon_set_inner_by_points")
# made-up device addresses
D, S, R, I = (4096, 8192, 12288), (16384, 20480, 24576), (28672, 32768, 36864), (40960, 45056, 49152)
MU = 53248


def test_entry_points_are_declared_exported_and_bound():
    from hyteg_amd import capi

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for name in ENTRY_POINTS + ("hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_component_masks",):
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_hip.h"
        assert hasattr(raw, name), f"{name} not exported"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert hasattr(capi.lib(), name)


def replaced(t, k, v):
    return tuple(v if i == k else x for i, x in enumerate(t))


def test_apply_rejects_bad_arguments_on_the_host():
    from hyteg_amd import capi

    f = capi.p1_elementwise_epsilon_apply_macro_3d_masked
    for k in range(3):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            f(replaced(D, k, None), S, MU, SKEW_TET, 16)
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            f(D, replaced(S, k, None), MU, SKEW_TET, 16)
    for args in ((None, S, MU), (D, None, MU), (D, S, None)):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            f(*args, SKEW_TET, 16)
    lib = capi.lib()
    d3, s3 = (ctypes.c_void_p * 3)(*D), (ctypes.c_void_p * 3)(*S)
    assert lib.hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_masked(d3, s3, MU, None, 16, capi.MASK_ALL, capi.REPLACE, 0) == 1  # EINVAL
    with pytest.raises(capi.HytegHipError, match="power of two, at most 2\\^8"):
        f(D, S, MU, SKEW_TET, 1 << 9)
    with pytest.raises(capi.HytegHipError, match="power of two"):
        f(D, S, MU, SKEW_TET, 12)
    for i in range(3):
        for j in range(3):  # any dst with any src
            with pytest.raises(capi.HytegHipError, match="alias"):
                f(replaced(D, i, S[j]), S, MU, SKEW_TET, 16)
        with pytest.raises(capi.HytegHipError, match="alias"):
            f(replaced(D, i, MU), S, MU, SKEW_TET, 16)
        with pytest.raises(capi.HytegHipError, match="alias"):
            f(replaced(D, i, D[(i + 1) % 3]), S, MU, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="bad update"):
        f(D, S, MU, SKEW_TET, 16, update=7)
    with pytest.raises(capi.HytegHipError, match="bad mask"):
        f(D, S, MU, SKEW_TET, 16, mask=1 << 15)
    with pytest.raises(capi.HytegHipError, match="bad mask"):
        f(D, S, MU, SKEW_TET, 16, mask=(capi.MASK_ALL, 1 << 15, 0))
    flat = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0))
    with pytest.raises(capi.HytegHipError, match="degenerate"):
        f(D, S, MU, flat, 16)


def test_jacobi_and_diagonal_reject_bad_arguments_on_the_host():
    from hyteg_amd import capi

    j = capi.p1_elementwise_epsilon_jacobi_macro_3d
    good = (D, S, R, I, MU)
    for pos in range(5):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            j(*replaced(good, pos, None), SKEW_TET, 16, 2.0 / 3.0)
    for pos in range(4):
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            j(*replaced(good, pos, replaced(good[pos], 1, None)), SKEW_TET, 16, 2.0 / 3.0)
    for other in (S, R, I):
        for k in range(3):
            with pytest.raises(capi.HytegHipError, match="alias"):
                j(replaced(D, 2, other[k]), S, R, I, MU, SKEW_TET, 16, 2.0 / 3.0)
    with pytest.raises(capi.HytegHipError, match="alias"):
        j(replaced(D, 0, MU), S, R, I, MU, SKEW_TET, 16, 2.0 / 3.0)
    with pytest.raises(capi.HytegHipError, match="at most 2\\^8"):
        j(D, S, R, I, MU, SKEW_TET, 1 << 9, 2.0 / 3.0)
    d = capi.p1_elementwise_epsilon_diagonal_macro_3d
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        d(replaced(D, 1, None), MU, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        d(D, None, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="alias"):
        d(replaced(D, 1, MU), MU, SKEW_TET, 16)
    with pytest.raises(capi.HytegHipError, match="at most 2\\^8"):
        d(D, MU, SKEW_TET, 1 << 9)


def test_set_shape_rejects_a_shape_that_is_not_compiled_in():
    from hyteg_amd import capi

    with pytest.raises(capi.HytegHipError, match="not compiled in"):
        capi.p1_elementwise_epsilon_set_shape(3, 5)
    for ny, lz in capi.EPSILON_SHAPES:
        capi.p1_elementwise_epsilon_set_shape(ny, lz)
    capi.p1_elementwise_epsilon_set_shape(0, 0)
