"""CPU-only: the Chebyshev smoother's coefficients (chebyshev::coefficients in hyteg_amd/host/chebyshev.hpp, through the C facade)
against their definition, and the new symbols of both C interfaces.

Definition: c[0..n-1] are the monomial coefficients of p in
    1 - l p(l) = T_n((theta - l) / delta) / T_n(theta / delta),  theta = (upper + lower) / 2,  delta = (upper - lower) / 2.
The tolerances are not measurements: the definition is exact, and a recurrence in extended precision reproduces it to a few
units of the last place of the largest term."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb
from numpy.polynomial import polynomial as nppoly

ROOT = Path(__file__).resolve().parent.parent
BOUNDS = [(0.3 * 1.97, 1.2 * 1.97), (0.1, 1.0), (0.5, 4.0)]

NEW_HIP = ["hyteg_hip_p1_chebyshev_start_cell", "hyteg_hip_p1_chebyshev_step_cell"]
NEW_HOST = ["hyteg_host_chebyshev_coefficients", "hyteg_host_chebyshev_estimate_radius", "hyteg_host_chebyshev_create",
            "hyteg_host_chebyshev_set_fused", "hyteg_host_gmg_create_chebyshev", "hyteg_host_p2_chebyshev_estimate_radius",
            "hyteg_host_p2_chebyshev_create", "hyteg_host_p2_gmg_create_chebyshev", "hyteg_host_p2function_mult_elementwise"]


@pytest.fixture(scope="module")
def host():
    from hyteg_amd import host as h

    if not h.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    h.lib()
    return h


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_coefficients_reproduce_the_scaled_chebyshev_polynomial(host, order, lower, upper):
    theta, delta = 0.5 * (upper + lower), 0.5 * (upper - lower)
    c = host.chebyshev_coefficients(order, lower, upper)
    assert c.shape == (order,)
    lam = np.linspace(0.0, upper, 200)
    Tn = npcheb.Chebyshev.basis(order)
    want = Tn((theta - lam) / delta) / Tn(theta / delta)
    got = 1.0 - lam * nppoly.polyval(lam, c)
    err = np.abs(got - want).max()
    print(f"order {order} bounds ({lower}, {upper}): max |1 - l p(l) - T_n/T_n| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("lower,upper", BOUNDS)
def test_orders_one_and_two_have_their_closed_forms(host, lower, upper):
    theta, delta = 0.5 * (upper + lower), 0.5 * (upper - lower)
    c1 = host.chebyshev_coefficients(1, lower, upper)
    assert abs(c1[0] * theta - 1.0) <= 1e-15
    c2 = host.chebyshev_coefficients(2, lower, upper)
    want = np.array([4.0 * theta, -2.0]) / (2.0 * theta**2 - delta**2)
    assert np.abs(c2 / want - 1.0).max() <= 1e-15


def test_the_polynomial_damps_the_interval_it_was_built_for(host):
    """|1 - l p(l)| <= 1 / T_n(theta / delta) on [lower, upper] (the min-max property), and = 1 at l = 0"""
    lower, upper = BOUNDS[0]
    theta, delta = 0.5 * (upper + lower), 0.5 * (upper - lower)
    for order in range(1, 9):
        c = host.chebyshev_coefficients(order, lower, upper)
        lam = np.linspace(lower, upper, 400)
        bound = 1.0 / npcheb.Chebyshev.basis(order)(theta / delta)
        assert np.abs(1.0 - lam * nppoly.polyval(lam, c)).max() <= bound * (1.0 + 1e-9)


def test_orders_outside_the_accepted_range_are_rejected(host):
    with pytest.raises(ValueError):
        host.chebyshev_coefficients(0, 0.5, 2.0)
    with pytest.raises(host.HytegHostError, match="order"):
        host.chebyshev_coefficients(9, 0.5, 2.0)
    with pytest.raises(host.HytegHostError, match="lowerBound"):
        host.chebyshev_coefficients(3, 2.0, 0.5)


def _declared(header, prefix):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_new_symbols_are_declared_exported_and_bound(host):
    from hyteg_amd import capi

    if not capi.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    for header, prefix, names, mod in (("hyteg_hip.h", "hyteg_hip_", NEW_HIP, capi), ("hyteg_host.h", "hyteg_host_", NEW_HOST, host)):
        declared = _declared(header, prefix)
        raw = ctypes.CDLL(str(mod.lib_path()))
        for name in names:
            assert name in declared, f"{name} is not declared in include/{header}"
            assert hasattr(raw, name), f"{name} is declared but not exported"
            assert name in mod.SIGNATURES, f"{name} has no ctypes binding"
    assert host.CHEBYSHEV not in (host.JACOBI, host.GAUSS_SEIDEL, host.SOR, host.JACOBI_FP32)
    for attr in ("chebyshev", "gmg_chebyshev", "set_fused"):
        assert hasattr(host.Solver, attr)
    assert hasattr(host, "estimate_radius") and hasattr(host.P2Solver, "gmg_chebyshev")
    with pytest.raises(ValueError, match="gmg_chebyshev"):  # not a smoother code of hyteg_host_gmg_create: no silent other smoother
        host.Solver.gmg(None, 2, 4, smoother=host.CHEBYSHEV)


def test_kernel_arguments_are_checked_before_any_gpu_work():
    from hyteg_amd import capi

    w = [1.0] * 15
    a, b, c = 4096, 8192, 12288
    with pytest.raises(capi.HytegHipError, match="null pointer"):
        capi.p1_chebyshev_start_cell(None, b, c, 4, w)
    with pytest.raises(capi.HytegHipError, match="level out of range"):
        capi.p1_chebyshev_start_cell(a, b, c, 12, w)
    with pytest.raises(capi.HytegHipError, match="alias"):
        capi.p1_chebyshev_start_cell(a, b, a, 4, w)
    with pytest.raises(capi.HytegHipError, match="zero centre"):
        capi.p1_chebyshev_start_cell(a, b, c, 4, [0.0] * 15)
    for t_out, x, t_in in ((a, a, b), (a, b, a), (a, b, b)):
        with pytest.raises(capi.HytegHipError, match="three different"):
            capi.p1_chebyshev_step_cell(t_out, x, t_in, 4, w, 0.5, 0.25)
    with pytest.raises(capi.HytegHipError, match="level out of range"):
        capi.p1_chebyshev_step_cell(a, b, c, 1, w, 0.5, 0.25)
