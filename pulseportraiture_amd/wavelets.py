"""The db8 low-pass filter the wavelet smoothing kernels take, derived rather than tabulated.

Daubechies' construction: |H(w)|^2 = 2 cos^16(w / 2) P(sin^2(w / 2)) with P(y) = sum_{k<8} C(7 + k, k) y^k.
P has no real root; with y = (2 - z - 1/z) / 4 each of its seven roots gives a pair (z, 1/z), and the minimum-phase
factor keeps the z inside the unit circle: h(z) ~ (1 + z)^8 prod (z - z_i).  That is PyWavelets' rec_lo ordering (the
energy comes first); dec_lo is its reverse and the high-pass filters are the quadrature mirrors.  The roots come from
numpy.roots, good to ~1e-13 here; a few Newton steps (residuals in extended precision) on the defining equations -- orthonormality under even shifts
and eight vanishing moments of the mirror filter -- bring the taps to rounding.
"""
from math import comb

import numpy as np

NTAP = 16
NMOM = NTAP // 2


def _residual(h):
    # (in extended precision: the Newton step below is solved in f64, but what it drives to zero is this)
    h = np.asarray(h, dtype=np.longdouble)
    k = np.arange(NTAP, dtype=np.longdouble)
    sign = (-np.longdouble(1)) ** np.arange(NTAP)
    orth = [np.dot(h[:NTAP - 2 * m], h[2 * m:]) - (1 if m == 0 else 0) for m in range(NMOM)]
    # moments scaled by 15^-p so that every equation carries the same weight
    mom = [np.dot(sign * (k / (NTAP - 1)) ** p, h) for p in range(NMOM)]
    return np.array(orth + mom + [h.sum() - np.sqrt(np.longdouble(2))], dtype=np.longdouble)


def _jacobian(h):
    k = np.arange(NTAP, dtype=np.float64)
    sign = (-1.0) ** k
    J = np.zeros((2 * NMOM + 1, NTAP))
    for m in range(NMOM):
        J[m, :NTAP - 2 * m] += h[2 * m:]
        J[m, 2 * m:] += h[:NTAP - 2 * m]
    for p in range(NMOM):
        J[NMOM + p] = sign * (k / (NTAP - 1.0)) ** p
    J[2 * NMOM] = 1.0
    return J


def db8_rec_lo():
    """The 16 taps of db8's reconstruction low-pass filter (PyWavelets' Wavelet('db8').rec_lo)."""
    P = [comb(NMOM - 1 + k, k) for k in range(NMOM)]          # ascending powers of y
    ys = np.roots(P[::-1])
    zs = []
    for y in ys:
        b = 2.0 - 4.0 * y                                     # z + 1/z
        pair = np.roots([1.0, -b, 1.0])
        zs.append(pair[np.argmin(np.abs(pair))])
    poly = np.poly(np.concatenate([-np.ones(NMOM), np.array(zs)]))
    h = np.asarray(np.real(poly), dtype=np.longdouble)
    h *= np.sqrt(np.longdouble(2)) / h.sum()
    for _ in range(6):
        r = _residual(h)
        step = np.linalg.lstsq(_jacobian(np.asarray(h, dtype=np.float64)), np.asarray(r, dtype=np.float64), rcond=None)[0]
        h = h - step
        if np.max(np.abs(step)) < 1e-19:
            break
    return np.asarray(h, dtype=np.float64)


_REC_LO = None


def rec_lo():
    """db8_rec_lo(), computed once per process."""
    global _REC_LO
    if _REC_LO is None:
        _REC_LO = db8_rec_lo()
    return _REC_LO.copy()
