"""numpy restatements for the Chebyshev smoother tests, written from the smoother's definition: the coefficients from numpy's
Chebyshev class (not from the code under test), the smoother call, a power iteration and a V-cycle on one macro-cell built from
the single-cell CPU oracle."""
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
