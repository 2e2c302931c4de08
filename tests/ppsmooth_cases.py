"""The wavelet-smoothing cases shared by tests/golden/make_golden_ppsmooth.py and the tests: two-Gaussian
profiles plus seeded white noise (samples rounded to multiples of 2^-20 so that the fixtures compress)."""
import numpy as np

# wavelet_smooth: (nbin, nlevel); every pair runs with both threshold types and every factor
WAVELET_CASES = ((16, 1), (16, 4), (64, 6), (100, 1), (256, 5), (2048, 11), (4096, 12))
THRESHTYPES = ("hard", "soft")
FACTS = (0.0, 0.7, 3.0, -0.1)

# smart_smooth: name -> (nbin, S/N of the taller component, seed, threshtype)
SMART_CASES = {
    "256_snr30": (256, 30.0, 4201, "hard"),
    "256_snr3": (256, 3.0, 4202, "hard"),
    "64_snr30": (64, 30.0, 4203, "hard"),
    "64_snr1": (64, 1.0, 4203, "hard"),         # no candidate passes the chi^2 test: the row comes back zero
    "100_snr30": (100, 30.0, 4204, "hard"),
    "256_snr30_soft": (256, 30.0, 4201, "soft"),    # a continuous objective: the simplex moves the factor off the grid
}
# spline models made with smoothing: cases of tests/ppspline_cases.py
MODEL_CASES = ("64x256", "48x1000")


def profile(nbin, snr, seed):
    """Two Gaussian components (heights 1 and 0.5) plus white noise of sigma 1 / snr."""
    rng = np.random.default_rng(seed)
    x = (np.arange(nbin) + 0.5) / nbin
    clean = np.exp(-0.5 * ((x - 0.4) / 0.03) ** 2) + 0.5 * np.exp(-0.5 * ((x - 0.55) / 0.06) ** 2)
    prof = clean + rng.standard_normal(nbin) / snr
    return np.rint(prof * 2.0 ** 20) / 2.0 ** 20


def wavelet_input(nbin):
    return profile(nbin, 10.0, 4100 + nbin)


def smart_input(name):
    return profile(*SMART_CASES[name][:3])
