"""A plain NumPy stand-in for the three PyWavelets calls the reference's wavelet smoothing makes -- swt, iswt,
threshold -- for the db8 wavelet, written from PyWavelets' documented algorithm and independent of the package's
kernels: time-domain circular convolutions with zero-stuffed filters, and the inverse by averaging the even and the odd
decimated inverse per level (the device uses the adjoint form instead).

`PYWT` is an object usable in place of the `pywt` module (tests/golden/make_golden_ppsmooth.py puts it into
sys.modules['pywt'] before it imports the reference).  The filters are derived here, by a route of their own: the
roots of the Daubechies polynomial polished by Newton steps in extended precision.
"""
import types
from math import comb

import numpy as np

NTAP = 16


def db8_filters():
    """(dec_lo, dec_hi, rec_lo, rec_hi) of db8 in PyWavelets' conventions."""
    ld = np.longdouble
    cld = np.clongdouble
    N = NTAP // 2
    P = np.array([comb(N - 1 + k, k) for k in range(N)], dtype=ld)        # ascending in y
    dP = P[1:] * np.arange(1, N, dtype=ld)
    zs = []
    for y in np.roots(np.asarray(P[::-1], dtype=np.float64)):
        y = cld(y)
        for _ in range(4):
            pv = sum(P[k] * y ** k for k in range(N))
            dv = sum(dP[k] * y ** k for k in range(N - 1))
            y = y - pv / dv
        b = 2 - 4 * y                                   # z + 1/z
        disc = np.sqrt(b * b - 4)
        z1, z2 = (b + disc) / 2, (b - disc) / 2
        zs.append(z1 if abs(z1) < 1 else z2)
    poly = np.array([1], dtype=cld)
    for r in [cld(-1)] * N + zs:
        poly = np.convolve(poly, np.array([1, -r], dtype=cld))
    h = np.real(poly)
    h = h * (np.sqrt(ld(2)) / h.sum())
    rec_lo = np.asarray(h, dtype=np.float64)            # energy first (minimum phase)
    dec_lo = rec_lo[::-1].copy()
    k = np.arange(NTAP)
    rec_hi = (-1.0) ** k * dec_lo
    dec_hi = rec_hi[::-1].copy()
    return dec_lo, dec_hi, rec_lo, rec_hi


DEC_LO, DEC_HI, REC_LO, REC_HI = db8_filters()


def _check_wavelet(wavelet):
    name = getattr(wavelet, "name", wavelet)
    if name != "db8":
        raise ValueError("the stand-in knows db8 only, not %r" % (wavelet,))


def _dwt_per(x, filt):
    """One decimated analysis channel with periodic boundary: c[i] = sum_k filt[k] x[(2 i + NTAP / 2 - k) mod n]."""
    n = len(x)
    i = np.arange(n // 2)
    c = np.zeros(n // 2)
    for k in range(NTAP):
        c += filt[k] * x[(2 * i + NTAP // 2 - k) % n]
    return c


def _idwt_per(cA, cD):
    """The inverse of (_dwt_per(., DEC_LO), _dwt_per(., DEC_HI)): for orthonormal filters, its transpose."""
    n = 2 * len(cA)
    i = np.arange(len(cA))
    x = np.zeros(n)
    for k in range(NTAP):
        np.add.at(x, (2 * i + NTAP // 2 - k) % n, DEC_LO[k] * cA + DEC_HI[k] * cD)
    return x


def swt(data, wavelet="db8", level=None, start_level=0, axis=-1):
    """pywt.swt for a 1-D array: [(cA_L, cD_L), ..., (cA_1, cD_1)].  Level j convolves the running approximation
    circularly with the filters dilated by 2^(j-1)."""
    _check_wavelet(wavelet)
    x = np.asarray(data, dtype=np.float64)
    if x.ndim != 1 or start_level != 0:
        raise ValueError("the stand-in transforms one row from level 0")
    n = len(x)
    if level is None or level < 1 or n % (1 << level):
        raise ValueError("length %d is not a multiple of 2^%s" % (n, level))
    out = []
    a = x
    idx = np.arange(n)
    for j in range(1, level + 1):
        s = 1 << (j - 1)
        cA, cD = np.zeros(n), np.zeros(n)
        for k in range(NTAP):
            src = a[(idx + s * (NTAP // 2 - k)) % n]
            cA += DEC_LO[k] * src
            cD += DEC_HI[k] * src
        out.append((cA, cD))
        a = cA
    return out[::-1]


def iswt(coeffs, wavelet="db8"):
    """pywt.iswt: from the coarsest level down, every interleaved sub-sequence is inverted twice -- from its even and
    from its odd samples, the latter rolled by one -- and the two are averaged."""
    _check_wavelet(wavelet)
    coeffs = list(coeffs)
    output = np.array(coeffs[0][0], dtype=np.float64)
    num_levels = len(coeffs)
    for j in range(num_levels, 0, -1):
        step = 1 << (j - 1)
        cD = np.asarray(coeffs[num_levels - j][1], dtype=np.float64)
        for first in range(step):
            indices = np.arange(first, len(cD), step)
            even, odd = indices[0::2], indices[1::2]
            x1 = _idwt_per(output[even], cD[even])
            x2 = np.roll(_idwt_per(output[odd], cD[odd]), 1)
            output[indices] = (x1 + x2) / 2.0
    return output


def iswt_adjoint(coeffs):
    """The same inverse as the frame adjoint, r_{j-1} = (H_j^T r_j + G_j^T d_j) / 2 (what the device computes)."""
    coeffs = list(coeffs)
    r = np.array(coeffs[0][0], dtype=np.float64)
    n = len(r)
    idx = np.arange(n)
    L = len(coeffs)
    for j in range(L, 0, -1):
        s = 1 << (j - 1)
        d = np.asarray(coeffs[L - j][1], dtype=np.float64)
        new = np.zeros(n)
        for k in range(NTAP):
            np.add.at(new, (idx + s * (NTAP // 2 - k)) % n, DEC_LO[k] * r + DEC_HI[k] * d)
        r = 0.5 * new
    return r


def threshold(data, value, mode="soft", substitute=0):
    """pywt.threshold, modes 'hard' and 'soft'."""
    data = np.asarray(data)
    magnitude = np.absolute(data)
    if mode == "hard":
        return np.where(np.less(magnitude, value), substitute, data)
    if mode == "soft":
        with np.errstate(divide="ignore", invalid="ignore"):
            thresholded = 1 - value / magnitude
            thresholded.clip(min=0, max=None, out=thresholded)
            thresholded = data * thresholded
        if substitute == 0:
            return thresholded
        return np.where(np.less(magnitude, value), substitute, thresholded)
    raise ValueError("mode %r" % (mode,))


PYWT = types.SimpleNamespace(swt=swt, iswt=iswt, threshold=threshold, __name__="pywt")


# ---- the reference's smoothing, restated on the stand-in (pplib.py:1621-1761) ------------------------------------
def get_noise(x):
    F = np.fft.rfft(x)
    pows = np.real(F * np.conj(F)) / len(x)
    kc = int((1 - 4 ** -1) * len(pows))
    return np.sqrt(np.mean(pows[kc:]))


def smooth_parts(prof, nlevel, threshtype="hard", fact=1.0, inverse=iswt):
    """(smoothed profile, lopt, the coefficient array before thresholding)."""
    coeffs = np.array(swt(prof, "db8", level=nlevel))
    lopt = fact * (np.median(np.abs(coeffs[0])) / 0.6745) * np.sqrt(2 * np.log(len(prof)))
    th = threshold(coeffs, lopt, mode=threshtype, substitute=0.0)
    return inverse(list(map(tuple, th))), lopt, coeffs


def wavelet_smooth(prof, nlevel=5, threshtype="hard", fact=1.0, inverse=iswt):
    return smooth_parts(prof, nlevel, threshtype, fact, inverse)[0]


def objective(fact, prof, nlevel, threshtype="hard", rchi2_tol=0.1):
    s = wavelet_smooth(prof, nlevel, threshtype, fact)
    sig = np.sum(np.abs(np.fft.rfft(s)[1:]) ** 2)
    snr = 0.0
    if sig:
        noise = get_noise(s) * np.sqrt(len(s) / 2.0)
        snr = sig / noise if noise else np.inf
    rc = np.sum(((prof - s) / get_noise(prof)) ** 2.0) / len(prof)
    if abs(rc - 1.0) > rchi2_tol:
        snr = 0.0
    return -snr


def tie_margin(prof, nlevel, facts):
    """The smallest | |c| / lopt - 1 | over the coefficients of the nlevel-deep transform and the factors `facts`
    (inf where lopt is 0): how far the nearest coefficient is from a threshold, relative to the threshold."""
    coeffs = np.array(swt(prof, "db8", level=nlevel))
    mags = np.concatenate([np.abs(coeffs[0][0])] + [np.abs(c[1]) for c in coeffs])
    scale = (np.median(np.abs(coeffs[0])) / 0.6745) * np.sqrt(2 * np.log(len(prof)))
    worst = np.inf
    for f in np.atleast_1d(facts):
        lopt = f * scale
        if lopt > 0:
            worst = min(worst, np.min(np.abs(mags / lopt - 1.0)))
    return worst
