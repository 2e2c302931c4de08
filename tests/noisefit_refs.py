"""Plain NumPy restatement of the 'fit' noise method (find_kc, pplib.py:1465-1495, and get_noise_fit,
pplib.py:2255-2287): the 20 x 20 x 20 grid opt.brute(Ns=20, finish=None) builds, the chi-squared of every cell
summed as the reference sums it, NumPy's argmin, kc and the tail mean.  No SciPy.  test_noisefit_cpu.py pins it to
tests/golden/noisefit.npz (the true reference); the GPU tests compare the device against it at the row lengths the
fixture does not reach.

margin: how far the reference's own choice of the width index ia is from a toss-up -- the relative gap between the
minimum chi-squared and the smallest chi-squared at any cell with another ia (for a winner with b = 0, whose 20
widths tie exactly, only cells with b != 0 count; half triangles of the same floor(a) are one model and tie exactly
too).  Another summation order moves a chi-squared by ~1e-13 of itself;
an integer comparison is meaningful where the margin is well above that (MARGIN_MIN).
"""
import numpy as np

NS = 20
FNS = ("exp_dc", "half_tri")
MARGIN_MIN = 1e-9
LENGTHS_FIXTURE = (64, 100, 256, 1000)
SPECIAL = ("noise", "constant", "zeros", "zero_sum_int", "b0")


def mgrid_axis(lo, hi, n=NS):
    """np.mgrid[lo:hi:nj] along one axis: index * step + lo with step = (hi - lo) / (n - 1)."""
    step = (hi - lo) / float(n - 1)
    return np.arange(n, dtype=np.float64) * step + lo


def width_axis(H, fn):
    return mgrid_axis(float(H) ** -1, 1.0) if fn == "exp_dc" else mgrid_axis(1, H)


def kc_of_width(a, H, fn):
    if fn == "half_tri":
        return int(np.floor(a))
    hit = np.where(np.exp(-a * np.arange(H)) < 0.005)[0]
    return int(hit.min()) if len(hit) else H - 1


def width_table(H, fn):
    """(a20, kc20): what pp_noise_fit_grid returns."""
    a20 = width_axis(H, fn)
    return a20, np.array([kc_of_width(a, H, fn) for a in a20], dtype=np.int32)


def chi2_grid(data, fn):
    """J[ia, ib, idc] = sum((data - model)^2) and the three axes."""
    H = len(data)
    with np.errstate(all="ignore"):
        a20 = width_axis(H, fn)
        b20 = mgrid_axis(0, data.max() - data.min())
        dc20 = mgrid_axis(data.min(), data.max())
        J = np.empty((NS, NS, NS))
        k = np.arange(H)
        for ia, a in enumerate(a20):
            if fn == "exp_dc":
                model = b20[:, None, None] * np.exp(-a * k)[None, None, :] + dc20[None, :, None]
            else:
                ai = int(np.floor(a))
                model = np.zeros((NS, NS, H)) + dc20[None, :, None]
                model[:, :, :ai] += (-(b20 / ai)[:, None] * np.arange(ai)[None, :] + b20[:, None])[:, None, :]
            J[ia] = np.sum(((data[None, None, :] - model) / 1.0) ** 2.0, axis=-1)
    return J, a20, b20, dc20


def find_kc_full(pows, fn="exp_dc"):
    """dict(kc, cell, chi2_best, chi2_second, margin) of one power spectrum."""
    pows = np.asarray(pows, dtype=np.float64)
    H = len(pows)
    with np.errstate(all="ignore"):
        data = np.log10(pows)
        J, a20, b20, dc20 = chi2_grid(data, fn)
        flat = int(np.argmin(J.ravel()))
    ia, ib, idc = flat // (NS * NS), (flat // NS) % NS, flat % NS
    per_a = np.sort(J.reshape(NS, -1).min(axis=1))
    jmin = J[ia, ib, idc]
    if not np.isfinite(J).all():
        margin = np.inf                    # the all-NaN grid: cell 0 whatever the rounding
    else:
        # (half_tri: widths with the same floor(a) are the same model, the same bits, and no rivals either)
        width = np.floor(a20) if fn == "half_tri" else np.arange(NS)
        rivals = J[width != width[ia]]
        if b20[ib] == 0.0:
            rivals = rivals[:, b20 != 0.0]
        if rivals.size == 0:
            margin = np.inf
        else:
            gap = rivals.min() - jmin
            margin = gap / jmin if jmin > 0.0 else (np.inf if gap > 0.0 else 0.0)
    return dict(kc=kc_of_width(a20[ia], H, fn), cell=(ia, ib, idc), chi2_best=per_a[0], chi2_second=per_a[1],
                margin=margin)


def power_spectrum(row):
    F = np.fft.rfft(np.asarray(row, dtype=np.float64))
    return np.real(F * np.conj(F)) / len(row)


def tail_noise(pows, kc, fact=1.1):
    k = fact * kc
    if k >= len(pows):
        k = min(int(0.99 * len(pows)), k)
    return np.sqrt(np.mean(pows[int(k):]))


def noise_fit_row(row, fact=1.1, fn="exp_dc"):
    """dict(noise, kc, cell, margin, ...) of one profile: get_noise_fit(row, fact) with find_kc(pows, fn=fn)."""
    pows = power_spectrum(row)
    out = find_kc_full(pows, fn)
    out["noise"] = tail_noise(pows, out["kc"], fact)
    return out


def noise_fit_rows(rows, fact=1.1, fn="exp_dc"):
    """noise [n], kc [n], cell [n,3], margin [n] of every row."""
    res = [noise_fit_row(r, fact, fn) for r in rows]
    return (np.array([r["noise"] for r in res]), np.array([r["kc"] for r in res], dtype=np.int32),
            np.array([r["cell"] for r in res], dtype=np.int32), np.array([r["margin"] for r in res]))


def snr_row(row, noise, fudge=3.25):
    """get_SNR (pplib.py:2289-2308) with the given noise."""
    row = np.asarray(row, dtype=np.float64)
    Weq = row.sum() / row.max()
    mask = 0.0 if Weq <= 0.0 else 1.0
    Weq = 1.0 if Weq <= 0.0 else Weq
    return row.sum() / (noise * Weq ** 0.5) * mask / fudge


# ---- the rows the tests use -------------------------------------------------------
def f32_exact(x):
    """Rounded to float32 and back: one reference serves the f64 and the f32 input of the same values."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def pulse_rows(nbin, n, seed):
    """Gaussian pulses of width 0.02 - 0.15 rot and amplitude 1 - 100 sigma on unit noise."""
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    rows = np.empty((n, nbin))
    for i in range(n):
        amp, wid, at = 10.0 ** rng.uniform(0.0, 2.0), rng.uniform(0.02, 0.15), rng.uniform()
        rows[i] = amp * np.exp(-0.5 * ((ph - at) / (wid / 2.355)) ** 2) + rng.normal(0.0, 1.0, nbin)
    return f32_exact(rows)


def special_rows(nbin, seed):
    """SPECIAL, in that order: pure noise; a constant; zeros; integers that sum to zero (no power at DC, exactly);
    differenced noise, whose spectrum rises with k so that no decaying model beats b = 0."""
    rng = np.random.default_rng(seed)
    ints = rng.integers(-5, 6, nbin).astype(np.float64)
    ints[0] -= ints.sum()
    return f32_exact(np.array([rng.normal(0.0, 1.0, nbin), np.full(nbin, 3.25), np.zeros(nbin), ints,
                               np.diff(rng.normal(0.0, 1.0, nbin + 1))]))


# ---- the rows of tests/test_gpu_noisefit.py (here, so that the test without a GPU checks their margins first) ----
# every plan the row kernel instantiates up to 4096 bins (nbin 32 ... 4096), and both ends of the any-even path
TEST_LENGTHS = (8, 10, 32, 64, 100, 128, 256, 512, 1000, 1024, 2048, 4094, 4096)
TEST_NPULSE = 3
TEST_SPECTRA_H = (5, 6, 33, 51, 500, 2049)


def test_rows(nbin):
    """TEST_NPULSE pulses and the special rows, every value a float32.  Differenced noise does not make b = 0 win
    at every length and seed (at 32 bins the first seed's does not): the next seeds are tried until it does."""
    for j in range(20):
        special = special_rows(nbin, 5000 + nbin + 1000 * j)
        if find_kc_full(power_spectrum(special[SPECIAL.index("b0")]))["cell"][1] == 0:
            break
    else:
        raise AssertionError("no b = 0 row at nbin %d" % nbin)
    special[:SPECIAL.index("b0")] = special_rows(nbin, 5000 + nbin)[:SPECIAL.index("b0")]
    return np.concatenate([pulse_rows(nbin, TEST_NPULSE, 4000 + nbin), special])


def test_spectra(H):
    return np.array([power_spectrum(r) for r in pulse_rows(2 * (H - 1), 6, 7000 + H)])


test_rows.__test__ = test_spectra.__test__ = False          # (not tests: pytest collects by name)
