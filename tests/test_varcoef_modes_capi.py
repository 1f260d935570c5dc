"""CPU-only: the fused residual and Chebyshev entry points of the epsilon operator and of div-k-grad are declared, exported and
bound, and reject bad arguments on the host with EINVAL before any GPU work (made-up addresses: nothing is dereferenced on the
host)."""
import ctypes
import re
from pathlib import Path

import pytest

from conftest import SKEW_TET

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = tuple(f"hyteg_hip_p1_elementwise_{op}_{what}_macro_3d" for op in ("epsilon", "divkgrad")
                     for what in ("residual", "chebyshev_start", "chebyshev_step"))
# made-up device addresses: t_out / dst, x, t_in / src, rhs, inverse diagonal, coefficient
D, X, S, R, I = (4096, 8192, 12288), (16384, 20480, 24576), (28672, 32768, 36864), (40960, 45056, 49152), (53248, 57344, 61440)
MU = 65536


def test_entry_points_are_declared_exported_and_bound():
    from hyteg_amd import capi

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_hip.h"
        assert hasattr(raw, name), f"{name} not exported"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"


def test_header_comments_cite_the_reference_lines():
    text = (ROOT / "include" / "hyteg_hip.h").read_text()
    assert text.count("GeometricMultigridSolver.hpp:240-246") >= 2
    assert text.count("ChebyshevSmoother.hpp:165-212") >= 3  # the constant-stencil steps and the two operators here


def replaced(t, k, v):
    return tuple(v if i == k else x for i, x in enumerate(t))


def calls(capi, name):
    """the three entries as functions of ( dst / t_out, x, src / t_in, rhs, inv_diag, coef, micro_edges ) with 3-tuples of addresses
    (div-k-grad takes the first of each)"""
    one = name == "divkgrad"
    a = (lambda t: None if t is None else t[0]) if one else (lambda t: t)
    f = lambda what: getattr(capi, f"p1_elementwise_{name}_{what}_macro_3d")  # noqa: E731
    return {
        "residual": lambda d, x, s, r, i, mu, me=16: f("residual")(a(d), a(s), a(r), mu, SKEW_TET, me),
        "start": lambda d, x, s, r, i, mu, me=16: f("chebyshev_start")(a(d), a(r), a(s), a(i), mu, SKEW_TET, me),
        "step": lambda d, x, s, r, i, mu, me=16: f("chebyshev_step")(a(d), a(x), a(s), a(i), mu, SKEW_TET, me, 0.5, -0.25, 1),
    }


USED = {"residual": (0, 2, 3, 5), "start": (0, 2, 3, 4, 5), "step": (0, 1, 2, 4, 5)}  # positions of the arguments an entry reads
WRITTEN = {"residual": (0,), "start": (0,), "step": (0, 1)}


@pytest.mark.parametrize("name", ["epsilon", "divkgrad"])
def test_bad_arguments_are_rejected_on_the_host(name):
    from hyteg_amd import capi

    good = (D, X, S, R, I, MU)
    for what, call in calls(capi, name).items():
        for pos in USED[what]:
            with pytest.raises(capi.HytegHipError, match=r"code 1\).*null pointer"):
                call(*replaced(good, pos, None))
            if pos < 5 and name == "epsilon":
                with pytest.raises(capi.HytegHipError, match="null pointer"):
                    call(*replaced(good, pos, replaced(good[pos], 1, None)))
        with pytest.raises(capi.HytegHipError, match="at most 2\\^8"):
            call(*good, 1 << 9)
        with pytest.raises(capi.HytegHipError, match="power of two"):
            call(*good, 12)
        # a written array against every other array of the call and against the coefficient
        for w in WRITTEN[what]:
            for pos in USED[what]:
                if pos == w:
                    continue
                other = (MU,) * 3 if pos == 5 else good[pos]
                with pytest.raises(capi.HytegHipError, match=r"code 1\).*alias"):
                    call(*replaced(good, w, replaced(good[w], 0, other[0])))
        # an input that is the coefficient
        for pos in USED[what]:
            if pos not in WRITTEN[what] and pos != 5:
                with pytest.raises(capi.HytegHipError, match="alias"):
                    call(*replaced(good, pos, replaced(good[pos], 0, MU)))
        if name == "epsilon":
            for w in WRITTEN[what]:  # two components of one written array
                with pytest.raises(capi.HytegHipError, match="alias"):
                    call(*replaced(good, w, replaced(good[w], 2, good[w][0])))
    if name == "epsilon":
        with pytest.raises(capi.HytegHipError, match="bad component bits"):
            capi.p1_elementwise_epsilon_residual_macro_3d(D, S, R, MU, SKEW_TET, 16, comps=8)
