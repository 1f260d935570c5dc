"""numpy restatements for the Chebyshev smoother tests, written from the smoother's definition: the coefficients from numpy's
Chebyshev class (not from the code under test), the smoother call, a power iteration and a V-cycle on one macro-cell built from
the single-cell CPU oracle; and kernel_case, the two C-ABI steps against the oracle's composition (test_gpu_chebyshev.py runs it on
the fused kernels, test_gpu_level11_paths.py on the composed fallbacks)."""
import numpy as np
from numpy.polynomial import chebyshev as npcheb

from oracle import p1_oracle as po


def coefficients(order, lower, upper):
    """monomial coefficients c[0..n-1] of p in 1 - l p(l) = T_n((theta - l)/delta) / T_n(theta/delta)"""
    theta, delta = 0.5 * (upper + lower), 0.5 * (upper - lower)
    # T_n(s) as a power series in s, then s = theta/delta - l/delta as a polynomial in l
    s = np.polynomial.Polynomial([theta / delta, -1.0 / delta])
    q = np.polynomial.Polynomial(npcheb.cheb2poly([0.0] * order + [1.0]))(s)
    u = q.coef
    return -u[1:order + 1] / u[0]


def smooth_cell(x, b, level, w, inv, c):
    """one smoother call on the interior of one macro-cell, the composition statement by statement; returns (x, t)"""
    x = x.copy()
    t2 = np.zeros_like(x)
    po.apply_cell(t2, x, level, w)
    po.assign(t2, [1.0, -1.0], [b, t2], level)
    t1 = np.zeros_like(x)
    po.mult_elementwise(t1, [inv, t2], level)
    po.assign(x, [1.0, c[0]], [x, t1], level)
    for k in range(1, len(c)):
        po.apply_cell(t2, t1, level, w)
        po.mult_elementwise(t1, [inv, t2], level)
        po.assign(x, [1.0, c[k]], [x, t1], level)
    return x


def radius_cell(level, w, iters=100, seed=0):
    """spectral radius of D^-1 A restricted to the interior points of one macro-cell: `iters` power iterations"""
    inner = po.inner_mask(level).astype(bool)
    v = np.zeros(po.cell_size(level))
    v[inner] = np.random.default_rng(seed).random(int(inner.sum()))
    y, rho = np.zeros_like(v), 0.0
    for _ in range(iters):
        v /= np.linalg.norm(v)
        po.apply_cell(y, v, level, w)
        y[~inner] = 0.0
        y /= w[7]
        rho = float(v @ y)
        v = y.copy()
    return rho


class CellCycle:
    """V(pre, post) cycle on one macro-cell with zero Dirichlet values, from apply_cell / restrict_cell / prolongate_cell;
    smoother: callable (x, b, level) -> x; the coarsest level is solved by conjugate gradients to 1e-10"""

    def __init__(self, coords, lo, hi, smoother, pre, post):
        self.lo, self.hi, self.smoother, self.pre, self.post = lo, hi, smoother, pre, post
        self.w = {l: po.assemble_cell_stencil(coords, l) for l in range(lo, hi + 1)}
        self.inner = {l: po.inner_mask(l).astype(bool) for l in range(lo, hi + 1)}
        self.nnc = np.ones(14)

    def A(self, v, level):
        y = np.zeros_like(v)
        po.apply_cell(y, v, level, self.w[level])
        y[~self.inner[level]] = 0.0
        return y

    def residual(self, x, b, level):
        r = np.zeros_like(x)
        m = self.inner[level]
        r[m] = (b - self.A(x, level))[m]
        return r

    def coarse_solve(self, b):
        l, m = self.lo, self.inner[self.lo]
        x = np.zeros_like(b)
        r = np.where(m, b, 0.0)
        p, rr, r0 = r.copy(), float(r @ r), float(np.sqrt(r @ r))
        for _ in range(1000):
            if np.sqrt(rr) <= 1e-10 * r0 or rr == 0.0:
                break
            ap = self.A(p, l)
            alpha = rr / float(p @ ap)
            x += alpha * p
            r -= alpha * ap
            rr_new = float(r @ r)
            p = r + (rr_new / rr) * p
            rr = rr_new
        return x

    def cycle(self, x, b, level=None):
        level = self.hi if level is None else level
        if level == self.lo:
            return self.coarse_solve(b)
        for _ in range(self.pre):
            x = self.smoother(x, b, level)
        r = self.residual(x, b, level)
        full = np.zeros(po.cell_size(level - 1))
        po.restrict_cell(full, r, level - 1, self.nnc)
        bc = np.where(self.inner[level - 1], full, 0.0)
        xc = self.cycle(np.zeros_like(bc), bc, level - 1)
        fine = np.zeros_like(x)
        po.prolongate_cell(xc, fine, level - 1, self.nnc)
        x = x.copy()
        x[self.inner[level]] += fine[self.inner[level]]
        for _ in range(self.post):
            x = self.smoother(x, b, level)
        return x


def multi_cell_smooth(orc, st, x, b, inv, c, level, flag, point_mask):
    """the smoother call on a storage of several macro-cells (orc: hostutil.MultiCellOracle); lists of cell arrays"""
    masks = [point_mask(level, st.mask(i, flag)) for i in range(len(x))]
    x = [a.copy() for a in x]

    def precondition(src):
        t2 = [np.zeros_like(a) for a in x]
        orc.apply(src, t2, level, flag)
        return t2

    t2 = precondition(x)
    t2 = [np.where(m, bb - tt, 0.0) for m, bb, tt in zip(masks, b, t2)]
    t1 = [np.where(m, iv * tt, 0.0) for m, iv, tt in zip(masks, inv, t2)]
    x = [np.where(m, xx + c[0] * tt, xx) for m, xx, tt in zip(masks, x, t1)]
    for k in range(1, len(c)):
        t2 = precondition(t1)
        t1 = [np.where(m, iv * tt, 0.0) for m, iv, tt in zip(masks, inv, t2)]
        x = [np.where(m, xx + c[k] * tt, xx) for m, xx, tt in zip(masks, x, t1)]
    return x


C_PREV, C_CUR = 0.8317, -0.2113


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def kernel_inputs(tet, level, function_inverse, seed):
    """(w, x0, rhs, t_in, junk, inv): the seeded arrays of one kernel_case"""
    w = po.assemble_cell_stencil(tet, level)
    n = po.cell_size(level)
    rng = np.random.default_rng(seed)
    x0, rhs, t_in, junk = (rng.standard_normal(n) for _ in range(4))
    inv = (1.0 / w[7]) * (0.5 + rng.random(n)) if function_inverse else np.full(n, 1.0 / w[7])
    return w, x0, rhs, t_in, junk, inv


def kernel_case(torch, capi, tet, level, function_inverse, has_prev, seed, keep=None):
    """hyteg_hip_p1_chebyshev_start_cell / _step_cell through the C-ABI against the composition apply_cell / assign / mult_elementwise
    of the oracle: returns the relative L2 errors over the cell interior; everything else is asserted bit for bit here.  `keep`, a
    dict, receives the three arrays the kernels computed."""
    w, x0, rhs, t_in, junk, inv = kernel_inputs(tet, level, function_inverse, seed)
    inner = po.inner_mask(level).astype(bool)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    inv_d = dev(inv)
    invp = inv_d.data_ptr() if function_inverse else None
    c_prev, c_cur = C_PREV, C_CUR
    out = {}
    # start: t_out = inv .* ( rhs - A x ), x untouched
    x_d, rhs_d, t_d = dev(x0), dev(rhs), dev(junk)
    capi.p1_chebyshev_start_cell(t_d.data_ptr(), rhs_d.data_ptr(), x_d.data_ptr(), level, w, invdiag=invp)
    torch.cuda.synchronize()
    ref = junk.copy()
    po.apply_cell(ref, x0, level, w)
    po.assign(ref, [1.0, -1.0], [rhs, ref], level)
    po.mult_elementwise(ref, [inv, ref], level)
    got = t_d.cpu().numpy()
    out["start t_out"] = _rel(got[inner], ref[inner])
    assert np.array_equal(got[~inner], junk[~inner]), "start: t_out changed outside the cell interior"
    assert np.array_equal(x_d.cpu().numpy(), x0), "start: x must not be updated by this launch"
    if keep is not None:
        keep["start t_out"] = got
    # step: t_out = inv .* ( A t_in ); x = ( x + c_prev t_in ) + c_cur t_out
    x_d, tin_d, t_d = dev(x0), dev(t_in), dev(junk)
    capi.p1_chebyshev_step_cell(t_d.data_ptr(), x_d.data_ptr(), tin_d.data_ptr(), level, w, c_prev, c_cur, has_prev=has_prev, invdiag=invp)
    torch.cuda.synchronize()
    ref_t, ref_x = junk.copy(), x0.copy()
    po.apply_cell(ref_t, t_in, level, w)
    po.mult_elementwise(ref_t, [inv, ref_t], level)
    if has_prev:
        po.assign(ref_x, [1.0, c_prev], [ref_x, t_in], level)
    po.assign(ref_x, [1.0, c_cur], [ref_x, ref_t], level)
    got_t, got_x = t_d.cpu().numpy(), x_d.cpu().numpy()
    out["step t_out"] = _rel(got_t[inner], ref_t[inner])
    out["step x"] = _rel(got_x[inner], ref_x[inner])
    assert np.array_equal(got_t[~inner], junk[~inner]), "step: t_out changed outside the cell interior"
    assert np.array_equal(got_x[~inner], x0[~inner]), "step: x changed outside the cell interior"
    assert np.array_equal(tin_d.cpu().numpy(), t_in), "step: t_in is read-only"
    if keep is not None:
        keep["step t_out"], keep["step x"] = got_t, got_x
    return out
