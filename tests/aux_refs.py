"""Plain references of what the ppzap and ppspline device kernels compute, written from the algorithms
(ppzap.get_zap_channels, pplib.get_noise_PS / get_SNR / normalize_portrait / count_crossings /
find_significant_eigvec / pca, FITPACK's splev): NumPy and np.longdouble only, no GPU.
tests/test_aux_refs_cpu.py pins each of them to the true reference's fixtures; tests/test_gpu_aux_kernels.py
holds the kernels against them at the sizes the fixtures do not reach."""
import numpy as np


# ---- ppzap: the median / sigma clip ---------------------------------------------------------------
def clip(noise_row, good_row, nstd):
    """get_zap_channels' loop over one subint: (zap mask uint8, rounds, min relative margin).  A round takes
    thr = median + nstd * std of the channels still alive, flags those above it and removes them; the last round
    flags none.  margin is the smallest |x - thr| / |thr| over the alive channels of every round: how close any
    decision came to going the other way (inf when no round ran, NaN when a threshold was NaN)."""
    x = np.asarray(noise_row, dtype=np.float64)
    alive = np.asarray(good_row) != 0
    zap = np.zeros(len(x), dtype=np.uint8)
    rounds, margin = 0, np.inf
    with np.errstate(all="ignore"):
        while alive.any():
            v = x[alive]
            thr = np.median(v) + nstd * np.std(v)
            rounds += 1
            m = np.min(np.abs(v - thr) / np.abs(thr))
            margin = m if np.isnan(m) or m < margin else margin
            bad = alive & (x > thr)
            if not bad.any():
                break
            zap[bad] = 1
            alive &= ~bad
    return zap, rounds, float(margin)


# ---- channel noise, norms and S/N -----------------------------------------------------------------
def _kc(nbin):
    return int(0.75 * (nbin // 2 + 1))


def noise_ps(row):
    """get_noise_PS(row, frac=4): sqrt of the mean power / nbin of the top quarter of the harmonics."""
    row = np.asarray(row, dtype=np.float64)
    nbin = len(row)
    with np.errstate(all="ignore"):
        pows = np.abs(np.fft.rfft(row)) ** 2 / nbin
        return float(np.sqrt(np.mean(pows[_kc(nbin):])))


def noise_ps_ld(row):
    """noise_ps from a direct DFT of the top-quarter harmonics in np.longdouble (angles reduced exactly in
    integers): what sizes the bar of a row length NumPy's own f64 transform cannot hold to 1e-12."""
    x = np.asarray(row, dtype=np.longdouble)
    nbin = len(x)
    k = np.arange(_kc(nbin), nbin // 2 + 1, dtype=np.int64)
    n = np.arange(nbin, dtype=np.int64)
    ang = (np.outer(k, n) % nbin).astype(np.longdouble) * _PI2_LD / nbin
    re, im = np.dot(np.cos(ang), x), np.dot(np.sin(ang), x)
    return np.sqrt(np.mean((re * re + im * im) / nbin))


_PI2_LD = 8 * np.arctan(np.longdouble(1))


def snr(row, fudge=3.25):
    """get_SNR(row, fudge): sum / (noise sqrt(Weq)) / fudge with Weq = sum / max; a Weq <= 0 is replaced by 1
    and zeroes the result; NaN propagates as NumPy's does."""
    row = np.asarray(row, dtype=np.float64)
    with np.errstate(all="ignore"):
        weq = row.sum() / row.max()
        mask = np.where(weq <= 0.0, 0.0, 1.0)
        weq = np.where(weq <= 0.0, 1.0, weq)
        return float((row.sum() / (noise_ps(row) * weq ** 0.5) * mask) / fudge)


def norm(row, method):
    """normalize_portrait's norm of one row (1 for a row without a non-zero sample, and for method None)."""
    row = np.asarray(row, dtype=np.float64)
    if method is None or not row.any():
        return 1.0
    if method == "mean":
        return float(row.mean())
    if method == "max":
        return float(row.max())
    if method == "rms":
        return noise_ps(row)
    if method == "abs":
        return float(np.sqrt((row ** 2).sum()))
    raise ValueError(method)


# ---- B-spline evaluation --------------------------------------------------------------------------
def deboor_ld(t, c, k, x):
    """The spline (t, c, k) at the points x by de Boor's recurrence in np.longdouble.  Outside [t[k], t[-k-1]]
    the boundary polynomial piece is used (splev's ext = 0); on a knot the piece to its right (the last piece at
    the end knot), as FITPACK's interval search chooses."""
    t = np.asarray(t, dtype=np.longdouble)
    c = np.asarray(c, dtype=np.longdouble)
    n = len(t)
    out = np.empty(np.shape(x), dtype=np.longdouble)
    for i, xv in enumerate(np.asarray(x, dtype=np.longdouble).ravel()):
        l = int(np.searchsorted(t, xv, side="right")) - 1
        l = min(max(l, k), n - k - 2)
        d = [c[j + l - k] for j in range(k + 1)]
        for r in range(1, k + 1):
            for j in range(k, r - 1, -1):
                lo, hi = t[j + l - k], t[j + 1 + l - r]
                a = (xv - lo) / (hi - lo)
                d[j] = (1 - a) * d[j - 1] + a * d[j]
        out.ravel()[i] = d[k]
    return out


# ---- PCA ------------------------------------------------------------------------------------------
def crossings(x, x0):
    """count_crossings: sign changes of x - x0 between neighbours, less the samples exactly on x0."""
    d = np.asarray(x, dtype=np.float64) - x0
    return int((np.diff(np.sign(d)) != 0).sum() - (d == 0).sum())


def ev_stats(ev):
    """find_significant_eigvec's numbers of one vector, unsmoothed: (sum_{k>=1} |rfft|^2, get_noise_PS(ev),
    max |ev|, count_crossings(|ev|, 0.1 max |ev|))."""
    ev = np.asarray(ev, dtype=np.float64)
    mx = float(np.abs(ev).max())
    return (float((np.abs(np.fft.rfft(ev)[1:]) ** 2).sum()), noise_ps(ev), mx, crossings(np.abs(ev), 0.1 * mx))


def pca_centre(port, w):
    """pplib.pca's centring: (mean_prof, delta = port - mean_prof, S, fact) with S = sqrt(w) (delta - its weighted
    average) -- np.cov(delta.T, aweights=w, ddof=1) is S.T S / fact and its dual is S S.T / fact."""
    port, w = np.asarray(port, dtype=np.float64), np.asarray(w, dtype=np.float64)
    mean_prof = (port * w[:, None]).sum(axis=0) / w.sum()
    delta = port - mean_prof
    avg = (delta * w[:, None]).sum(axis=0) / w.sum()
    fact = w.sum() - (w * w).sum() / w.sum()
    return mean_prof, delta, np.sqrt(w)[:, None] * (delta - avg), fact
