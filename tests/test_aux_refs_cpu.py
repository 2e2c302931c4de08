"""The plain references of tests/aux_refs.py against the true reference's fixtures (tests/golden/ppzap_noise.npz,
ppspline_*.npz) and SciPy, without a GPU: what tests/test_gpu_aux_kernels.py compares the kernels with is what the
reference computes."""
import os

import numpy as np
import pytest

from tests import aux_refs as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLDEN, "ppzap_noise.npz"))


def _g(name):
    return np.load(os.path.join(GOLDEN, "ppspline_%s.npz" % name))


@pytest.mark.parametrize("ia", [0, 1, 2])
@pytest.mark.parametrize("norm", ["none", "mean", "max", "prof", "abs"])
@pytest.mark.parametrize("nstd", [3, 5])
def test_clip_reproduces_the_references_zap_rows(ia, norm, nstd):
    noise = Z["a%d_noise_%s" % (ia, norm)]
    good = Z["a%d_weights" % ia][Z["a%d_ok_isubs" % ia]] > 0
    want = Z["a%d_zap_%s_%d" % (ia, norm, nstd)]
    for row, g, w in zip(noise, good, want):
        zap, rounds, margin = ar.clip(row, g, nstd)
        assert zap.dtype == np.uint8 and zap.tobytes() == w.tobytes()
        assert rounds >= 1 and margin >= 0.0 and not zap[~g].any()


def test_clip_edges():
    # one channel: thr == x, nothing flagged, margin 0; no channel: no round
    zap, rounds, margin = ar.clip([2.0], [1], 3)
    assert not zap.any() and rounds == 1 and margin == 0.0
    zap, rounds, margin = ar.clip([2.0, 3.0], [0, 0], 3)
    assert not zap.any() and rounds == 0 and margin == np.inf
    # a NaN threshold flags nothing
    for bad in (np.nan, np.inf):
        zap, rounds, margin = ar.clip([1.0, 1.0, 50.0, bad, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.ones(12), 3)
        assert not zap.any() and rounds == 1 and np.isnan(margin)


@pytest.mark.parametrize("name", ["64x256", "128x512", "48x1000", "300x128"])
def test_noise_and_snr_reproduce_the_references(name):
    from tests import ppspline_cases as pc
    g = _g(name)
    ok = g["weights"] > 0           # (the fixture's S/N of a zero-weight channel is not get_SNR's)
    port = (pc.make_input(name)[0] if name in pc.REGENERATED else g["port"])[ok]
    np.testing.assert_allclose([ar.noise_ps(r) for r in port], g["noise_stds"][ok], rtol=1e-12, atol=0)
    np.testing.assert_allclose([ar.snr(r) for r in port], g["SNRs"][ok], rtol=1e-12, atol=0)
    np.testing.assert_allclose([ar.snr(r, 1.0) for r in port[:3]], 3.25 * g["SNRs"][ok][:3], rtol=1e-12, atol=0)
    # the long-double DFT of the top quarter is the same number
    for r in port[:2]:
        assert abs(float(ar.noise_ps_ld(r)) / ar.noise_ps(r) - 1.0) < 1e-12


def test_snr_and_norm_special_rows():
    assert np.isnan(ar.snr(np.zeros(64))) and ar.noise_ps(np.zeros(64)) == 0.0
    x = -np.abs(np.random.default_rng(1).standard_normal(64)) - 0.1
    assert ar.snr(x) < 0
    x[5] = 0.0
    x = np.minimum(x, 0.0)
    assert x.max() == 0.0 and ar.snr(x) == 0.0
    y = x.copy()
    y[3] = np.nan
    assert np.isnan(ar.snr(y)) and np.isnan(ar.noise_ps(y))
    for m in (None, "mean", "max", "rms", "abs"):
        assert ar.norm(np.zeros(64), m) == 1.0
    assert ar.norm(x, "rms") == ar.noise_ps(x) and ar.norm(x, "abs") == np.sqrt((x * x).sum())


@pytest.mark.parametrize("name", ["64x256", "64x256_k5", "64x256_nbreak3"])
def test_deboor_agrees_with_splev(name):
    import scipy.interpolate as si
    g = _g(name)
    t, c, k = g["t"], g["c"], int(g["k"])
    f = g["freqs"]
    x = np.concatenate([f, 0.5 * (f[1:] + f[:-1]), np.unique(t), [t[0] - 30.0, t[-1] + 30.0]])
    for cj in c:
        want = si.splev(x, (t, cj, k), der=0, ext=0)
        got = ar.deboor_ld(t, cj, k, x).astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * max(np.abs(want).max(), np.abs(cj).max()))
        # FITPACK's full length (the last k + 1 unused) is the same spline
        full = np.concatenate([cj, np.zeros(len(t) - len(cj))])
        assert np.array_equal(ar.deboor_ld(t, full, k, x), ar.deboor_ld(t, cj, k, x))


def test_deboor_on_repeated_knots_and_low_degrees():
    import scipy.interpolate as si
    rng = np.random.default_rng(3)
    for k in (1, 2, 3, 4, 5):
        inner = np.sort(rng.uniform(1100.0, 1900.0, 7))
        inner = np.sort(np.concatenate([inner, inner[2:3]] + ([inner[5:6], inner[5:6]] if k >= 3 else [])))
        t = np.concatenate([[1000.0] * (k + 1), inner, [2000.0] * (k + 1)])
        c = rng.standard_normal(len(t) - k - 1)
        x = np.concatenate([rng.uniform(1000.0, 2000.0, 40), inner, [1000.0, 2000.0, 950.0, 2050.0]])
        want = si.splev(x, (t, c, k), ext=0)
        np.testing.assert_allclose(ar.deboor_ld(t, c, k, x).astype(np.float64), want, rtol=0,
                                   atol=1e-13 * max(np.abs(want).max(), np.abs(c).max()))


def test_ev_stats_reproduce_the_references():
    g = _g("64x256")
    scat = g["scat_stats"]
    for v in g["ieig"]:
        got, want = ar.ev_stats(g["eigvec"][:, v]), g["stats"][v]
        for col in range(3):
            bar = max(10.0 * scat[col], 1e-13 * np.abs(g["stats"][:, col]).max())
            assert abs(got[col] - want[col]) <= bar, (v, col, got[col], want[col], bar)
        assert got[3] == want[3]


def test_crossings_counts_threshold_samples_as_the_reference():
    # |ev| - x0: - 0 + : two sign changes less one zero = 1; a zero at either end: one change less one zero = 0
    assert ar.crossings([0.0, 1.0, 2.0], 1.0) == 1
    assert ar.crossings([1.0, 2.0, 2.0], 1.0) == 0 and ar.crossings([2.0, 2.0, 1.0], 1.0) == 0
    assert ar.crossings([0.0, 2.0, 0.0, 2.0], 1.0) == 3
    ev = np.array([10.0, -1.0, 0.0, 1.0, 5.0])
    assert ar.ev_stats(ev)[2:] == (10.0, ar.crossings(np.abs(ev), 1.0)) and ar.crossings(np.abs(ev), 1.0) == 2


def test_pca_centre_is_np_covs():
    rng = np.random.default_rng(8)
    port, w = rng.standard_normal((40, 16)) + 3.0, rng.uniform(0.5, 2.0, 40)
    mean_prof, delta, S, fact = ar.pca_centre(port, w)
    cov = np.cov(delta.T, aweights=w, ddof=1)
    np.testing.assert_allclose(np.dot(S.T, S) / fact, cov, rtol=0, atol=1e-13 * np.abs(cov).max())
    np.testing.assert_allclose(mean_prof, np.average(port, axis=0, weights=w), rtol=1e-14)
