"""The ppspline cases shared by tests/golden/make_golden_ppspline.py and the tests: the
synthetic aligned average portraits (the example pulsar's Gaussian-component portrait times
random channel gains, plus white noise, samples rounded to multiples of 2^-20 so that the
fixtures compress) and the make_spline_model arguments of each case."""
import hashlib

import numpy as np

# name: (nchan, nbin, sigma, channels zapped, descending band, make_spline_model arguments, seed)
CASES = {
    "64x256": (64, 256, 0.002, 0, False, {}, 7101),
    "128x512": (128, 512, 0.005, 9, False, {}, 7102),
    "48x1000": (48, 1000, 0.003, 0, True, {}, 7103),
    "300x128": (300, 128, 0.002, 20, False, {}, 7104),
    "64x256_nbreak3": (64, 256, 0.002, 0, False, {"max_nbreak": 3}, 7101),
    "64x256_sfac0": (64, 256, 0.002, 0, False, {"sfac": 0.0, "max_ncomp": 3}, 7101),
    "64x256_mean_only": (64, 256, 0.002, 0, False, {"snr_cutoff": np.inf}, 7101),
    "64x256_k5": (64, 256, 0.002, 0, False, {"k": 5, "max_ncomp": 2}, 7101),
    "512x2048": (512, 2048, 0.01, 0, False, {"max_ncomp": 4}, 7109),
}
# cases whose input is not stored but regenerated from the seed and checked by its SHA-256
REGENERATED = ("512x2048",)
# (the option cases of seed 7101 take their input from "64x256"'s fixture)
NSAMPLE_ROWS = 16      # rows of modelx and model a fixture stores


def make_input(name):
    """(port [nchan,nbin] with zapped rows zero, freqs [nchan], weights [nchan], bw) of a case."""
    from pulseportraiture_amd.gmodel import example_model
    nchan, nbin, sigma, nzap, descending, _, seed = CASES[name]
    rng = np.random.default_rng(seed)
    freqs, clean, _ = example_model(nchan, nbin)
    gains = rng.uniform(0.5, 1.5, nchan)
    port = gains[:, None] * clean + sigma * rng.standard_normal((nchan, nbin))
    port = np.rint(port * 2.0 ** 20) / 2.0 ** 20
    weights = np.ones(nchan)
    if nzap:
        weights[rng.choice(nchan, size=nzap, replace=False)] = 0.0
    port = port * weights[:, None]
    bw = 800.0
    if descending:
        freqs, port, weights, bw = freqs[::-1].copy(), port[::-1].copy(), weights[::-1].copy(), -bw
    return port, freqs, weights, bw


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def sample_rows(n):
    return np.unique(np.linspace(0, n - 1, min(n, NSAMPLE_ROWS)).round().astype(int))
