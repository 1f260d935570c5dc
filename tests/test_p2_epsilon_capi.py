"""CPU-only: the C-ABI entry points of the P2 epsilon operator -div( 2 mu eps(u) ) with a P2 viscosity are declared with the reference
locations they replace, exported by the cross-compiled library, bound, and reject bad arguments on the host with EINVAL before any GPU
work (made-up addresses: nothing is dereferenced on the host); the geometry helper is host arithmetic and is checked against the
restatement."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import divkgradutil as dk
import p2divkgradutil as pu
from conftest import SKEW_TET

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("hyteg_hip_p2_elementwise_epsilon_geometry", "hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds",
                "hyteg_hip_p2_elementwise_epsilon_apply_cell_gather", "hyteg_hip_p2_elementwise_epsilon_diagonal_cell",
                "hyteg_hip_p2_elementwise_epsilon_set_inner_min_level", "hyteg_hip_p2_elementwise_epsilon_max_level")
HOST_ENTRY_POINTS = ("hyteg_host_p2epsilon_create", "hyteg_host_p2epsilon_apply", "hyteg_host_p2epsilon_gemv",
                     "hyteg_host_p2epsilon_compute_inverse_diagonal", "hyteg_host_p2epsilon_inverse_diagonal", "hyteg_host_p2epsilon_smooth_jac",
                     "hyteg_host_p2epsilon_cg_create", "hyteg_host_p2epsilon_chebyshev_create", "hyteg_host_p2epsilon_smoother_create",
                     "hyteg_host_p2epsilon_solver_solve", "hyteg_host_th_epsilon_create", "hyteg_host_th_epsilon_apply",
                     "hyteg_host_th_epsilon_minres_create", "hyteg_host_th_epsilon_minres_solve", "hyteg_host_th_epsilon_minres_precondition")
DV, DE, SV, SE = (4096, 8192, 12288), (16384, 20480, 24576), (28672, 32768, 36864), (40960, 45056, 49152)  # made-up device addresses
MV, ME = 53248, 57344
GEOMETRY = [1.0] * 72


def test_entry_points_are_declared_exported_and_bound():
    from hyteg_amd import capi, host

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_hip.h").read_text(), flags=re.S)
    raw = ctypes.CDLL(str(capi.lib_path()))
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_hip.h"
        assert name in capi.SIGNATURES, f"{name} not bound in capi.SIGNATURES"
        assert hasattr(raw, name), f"{name} not exported by the library"
        assert hasattr(capi.lib(), name)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hyteg_host.h").read_text(), flags=re.S)
    for name in HOST_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in include/hyteg_host.h"
        assert name in host.SIGNATURES and hasattr(host.lib(), name)
    for cls in ("P2ViscousBlockEpsilonOperator", "P2EpsilonSolver", "TaylorHoodEpsilonStokesOperator", "TaylorHoodEpsilonSolver"):
        assert hasattr(host, cls)
    for method in ("apply", "gemv", "inverse_diagonal", "smooth_jac"):
        assert hasattr(host.P2ViscousBlockEpsilonOperator, method)
    for method in ("cg", "chebyshev", "smoother"):
        assert hasattr(host.P2EpsilonSolver, method)
    assert hasattr(host.TaylorHoodEpsilonSolver, "minres")


def test_every_entry_cites_what_it_replaces():
    text = (ROOT / "include" / "hyteg_hip.h").read_text()
    section = text[text.index("b-4 (P2 epsilon)"):text.index("b-5:")]
    assert section.count("operatorgeneration::P2ViscousBlockEpsilonOperator::apply") >= 3
    assert "computeInverseDiagonalOperatorValues" in section and "ElementwiseEpsilonMinResConvergenceTest.cpp" in section
    assert "P2P1ElementwiseAffineEpsilonStokesOperator.hpp:61-70" in section


@pytest.mark.parametrize("gather", [False, True])
def test_apply_rejects_bad_arguments_on_the_host(gather):
    from hyteg_amd import capi

    f = capi.p2_elementwise_epsilon_apply_cell
    good = [DV, DE, SV, SE, MV, ME]
    for bad in range(6):
        args = list(good)
        args[bad] = None
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            f(*args, 3, GEOMETRY, gather=gather)
    for group in range(4):  # one of the three pointers of a group
        for k in range(3):
            args = [list(a) if isinstance(a, tuple) else a for a in good]
            args[group][k] = None
            with pytest.raises(capi.HytegHipError, match="null pointer"):
                f(*args, 3, GEOMETRY, gather=gather)
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        f(*good, 3, None, gather=gather)
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        f(*good, 3, GEOMETRY, mask=None, gather=gather)
    for level in (-1, capi.p2_elementwise_epsilon_max_level() + 1, 12):
        with pytest.raises(capi.HytegHipError, match="level out of range"):
            f(*good, level, GEOMETRY, gather=gather)
    # a written array that is a src array, a mu array or another written array
    for group in (0, 1):
        for k in range(3):
            for other in (SV[0], SV[2], SE[1], MV, ME, DV[(k + 1) % 3], DE[(k + 2) % 3]):
                args = [list(a) if isinstance(a, tuple) else a for a in good]
                if args[group][k] == other:
                    continue
                args[group][k] = other
                with pytest.raises(capi.HytegHipError, match="alias"):
                    f(*args, 3, GEOMETRY, gather=gather)
    with pytest.raises(capi.HytegHipError, match="bad update"):
        f(*good, 3, GEOMETRY, update=7, gather=gather)


def test_diagonal_and_geometry_reject_bad_arguments_on_the_host():
    from hyteg_amd import capi

    d = capi.p2_elementwise_epsilon_diagonal_cell
    good = [DV, DE, MV, ME]
    for bad in range(4):
        args = list(good)
        args[bad] = None
        with pytest.raises(capi.HytegHipError, match="null pointer"):
            d(*args, 3, GEOMETRY)
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        d(*good, 3, None)
    with pytest.raises(capi.HytegHipError, match="level out of range"):
        d(*good, 9, GEOMETRY)
    for group in (0, 1):
        for other in (MV, ME):
            args = [list(a) if isinstance(a, tuple) else a for a in good]
            args[group][1] = other
            with pytest.raises(capi.HytegHipError, match="alias"):
                d(*args, 3, GEOMETRY)
    with pytest.raises(capi.HytegHipError, match="level out of range"):
        capi.p2_elementwise_epsilon_geometry(SKEW_TET, 9)
    flat = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0))
    with pytest.raises(capi.HytegHipError, match="degenerate"):
        capi.p2_elementwise_epsilon_geometry(flat, 3)
    assert capi.lib().hyteg_hip_p2_elementwise_epsilon_geometry(None, 3, None) == 1  # EINVAL


@pytest.mark.parametrize("level", [0, 3, 8])
def test_geometry_table_is_the_scaled_gradients_of_the_six_micro_cell_types(level):
    """h[t][3 a + r] = sqrt( |e| / 840 ) d_r l_a"""
    from hyteg_amd import capi

    got = np.array(capi.p2_elementwise_epsilon_geometry(SKEW_TET, level)).reshape(6, 4, 3)
    cc = np.asarray(SKEW_TET, dtype=np.float64).reshape(4, 3)
    h = 1.0 / (1 << level)
    for t in range(6):
        v = dk.MICRO_CELL_VERTS[t] * h
        g, vol = pu.gradients(cc[0] + v[:, 0:1] * (cc[1] - cc[0]) + v[:, 1:2] * (cc[2] - cc[0]) + v[:, 2:3] * (cc[3] - cc[0]))
        want = np.sqrt(vol / 840.0) * g
        assert np.abs(got[t] - want).max() <= 1e-13 * np.abs(want).max()


def test_inner_min_level_switch_returns_the_previous_value():
    from hyteg_amd import capi

    before = capi.p2_elementwise_epsilon_set_inner_min_level(99)
    assert capi.p2_elementwise_epsilon_set_inner_min_level(before) == 99
    assert capi.p2_elementwise_epsilon_set_inner_min_level(0) == before  # clamped to 2: no inner form below
    assert capi.p2_elementwise_epsilon_set_inner_min_level(before) == 2
