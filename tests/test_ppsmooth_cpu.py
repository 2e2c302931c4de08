"""Wavelet smoothing without a GPU: the derived db8 filters, the PyWavelets stand-in's identities, the host flow of
make_smooth_spline_model against the reference's goldens (a fake engine hands back the reference's smoothed vectors),
the new command's parser, and the two refusals that stay."""
import os

import numpy as np
import pytest

from tests import ppsmooth_cases as sc
from tests import ppspline_cases as pc
from tests import wavelet_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _g(name):
    return np.load(os.path.join(GOLDEN, "ppsmooth_model_%s.npz" % name))


def _filters():
    from pulseportraiture_amd import wavelets
    return {"package": wavelets.db8_rec_lo(), "stand-in": wr.REC_LO}


@pytest.mark.parametrize("which", ["package", "stand-in"])
def test_filter_algebra(which):
    h = _filters()[which]
    assert h.shape == (16,)
    assert abs(h.sum() - np.sqrt(2.0)) < 1e-13
    for m in range(8):
        assert abs(np.dot(h[:16 - 2 * m], h[2 * m:]) - (1.0 if m == 0 else 0.0)) < 1e-13, m
    k = np.arange(16.0)
    g = (-1.0) ** k * h[::-1]
    for p in range(8):          # eight vanishing moments of the mirror filter, relative to the moment's own scale
        assert abs(np.dot(k ** p, g)) < 1e-13 * np.dot(k ** p, np.abs(g)), p
    # PyWavelets' rec_lo ordering: the energy comes first
    assert abs(h[0] - 0.0544158422) < 1e-9 and abs(h[15] + 1.17476784e-4) < 1e-11


def test_the_two_derivations_agree():
    f = _filters()
    assert np.abs(f["package"] - f["stand-in"]).max() < 1e-15
    from pulseportraiture_amd import wavelets
    a = wavelets.rec_lo()
    a[0] = 0.0
    assert wavelets.rec_lo()[0] != 0.0          # (callers get a copy)
    np.testing.assert_array_equal(wr.DEC_LO, wr.REC_LO[::-1])
    np.testing.assert_array_equal(wr.DEC_HI, wr.REC_HI[::-1])


@pytest.mark.parametrize("nbin,nlevel", [c for c in sc.WAVELET_CASES if c[0] <= 2048])
def test_perfect_reconstruction_and_the_two_inverse_forms(nbin, nlevel):
    x = sc.wavelet_input(nbin)
    coeffs = wr.swt(x, "db8", level=nlevel)
    assert len(coeffs) == nlevel and coeffs[0][0].shape == (nbin,)
    scale = np.abs(x).max()
    for tt in sc.THRESHTYPES:
        assert np.abs(wr.wavelet_smooth(x, nlevel, tt, 0.0) - x).max() < 1e-14 * scale * nlevel       # fact = 0
    assert np.abs(wr.iswt_adjoint(coeffs) - x).max() < 1e-14 * scale * nlevel
    # on thresholded coefficients (no longer the transform of any signal) the time-domain even/odd average is the adjoint
    for tt in sc.THRESHTYPES:
        for fact in (0.7, 3.0, -0.1):
            a, lopt, c = wr.smooth_parts(x, nlevel, tt, fact)
            b = wr.wavelet_smooth(x, nlevel, tt, fact, inverse=wr.iswt_adjoint)
            assert np.abs(a - b).max() < 1e-14 * scale * nlevel
            if tt == "hard" and fact > 0:
                assert np.abs(a - x).max() > 1e-3 * scale          # (something was removed)


def test_threshold_is_pywts():
    c = np.array([-3.0, -1.0, 0.5, 2.0])
    np.testing.assert_array_equal(wr.threshold(c, 1.0, "hard", 0.0), [-3.0, -1.0, 0.0, 2.0])
    np.testing.assert_allclose(wr.threshold(c, 1.0, "soft", 0.0), [-2.0, 0.0, 0.0, 1.0])
    np.testing.assert_array_equal(wr.threshold(c, -0.1, "hard", 0.0), c)        # a negative threshold zeroes nothing
    assert np.all(np.abs(wr.threshold(c, -0.1, "soft", 0.0)) > np.abs(c))


def test_stand_in_against_pywavelets():
    pywt = pytest.importorskip("pywt")
    w = pywt.Wavelet("db8")
    np.testing.assert_allclose(wr.REC_LO, w.rec_lo, rtol=0, atol=1e-14)
    np.testing.assert_allclose(wr.DEC_HI, w.dec_hi, rtol=0, atol=1e-14)
    for nbin, nlevel in ((16, 4), (64, 6), (100, 1), (256, 5)):
        x = sc.wavelet_input(nbin)
        theirs = np.array(pywt.swt(x, "db8", level=nlevel, start_level=0))
        mine = np.array(wr.swt(x, "db8", level=nlevel))
        # (alignment conventions may shift a level's arrays circularly: compare what the smoothing reads)
        np.testing.assert_allclose(np.sort(np.abs(mine), axis=-1), np.sort(np.abs(theirs), axis=-1), rtol=0, atol=1e-12)
        for tt in sc.THRESHTYPES:
            lopt = 0.7 * np.median(np.abs(theirs[0])) / 0.6745 * np.sqrt(2 * np.log(nbin))
            t = pywt.threshold(theirs, lopt, mode=tt, substitute=0.0)
            want = pywt.iswt(list(map(tuple, t)), "db8")
            np.testing.assert_allclose(wr.wavelet_smooth(x, nlevel, tt, 0.7), want, rtol=0, atol=1e-12 * np.abs(x).max())


class GoldenEngine(object):
    """The device stages of make_smooth_spline_model from the reference's numbers."""

    def __init__(self, g, port):
        self.g, self.port, self.ok = g, port, g["weights"] > 0
        self.smooth_calls = []

    def channel_noise(self, port, norm=None, weights=None):
        return self.g["noise_stds"][self.ok], np.ones(self.ok.sum())

    def pca_gram(self, port, weights):
        return self.g["mean_prof"], np.diag(np.arange(12.0, 0.0, -1.0)), 1.0

    def pca_basis(self, vecs, eigval):
        return self.g["eigvec"], np.full((10, 4), np.nan)          # (the unsmoothed statistics must not be consulted)

    def pca_project(self, ieig):
        raise AssertionError("the smoothed model projects onto the smoothed basis")

    def smart_smooth(self, rows, try_nlevels, rchi2_tol=0.1, threshtype="hard"):
        g = self.g
        self.smooth_calls.append((len(rows), int(try_nlevels), rchi2_tol, threshtype))
        if len(rows) == 1:
            out, stats, noise = g["smooth_mean_prof"][None], np.zeros((1, 4)), np.zeros(1)
        else:
            # (the golden keeps the smoothed columns of the significant vectors; the decisions need the statistics only)
            out, stats, noise = np.ascontiguousarray(g["smooth_eigvec"].T), g["stats"][:, :4].copy(), g["stats"][:, 1].copy()
            stats[:, 1] = -1.0                                   # (find_significant_eigvec's noise is the RAW vector's)
        n = len(rows)
        return out, dict(level=np.zeros(n, int), fact=np.zeros(n), snr=np.zeros(n), red_chi2=np.zeros(n),
                         nfev=np.zeros(n, int), stats=stats, raw_noise=noise)

    def spline_portrait(self, mean_prof, eigvec, tck, freqs, nbin=None):
        from pulseportraiture_amd.splmodel import gen_spline_portrait
        return gen_spline_portrait(mean_prof, freqs, eigvec, tck)


def _portrait(name):
    from pulseportraiture_amd.ppspline import DataPortrait
    from pulseportraiture_amd.pptoas import data_from_arrays
    g = _g(name)
    port = pc.make_input(name)[0]
    assert pc.sha256(port) == str(g["input_sha256"])
    bunch = data_from_arrays(port[None, None], g["freqs"], [0.003], [55000.0], weights=g["weights"][None],
                             noise_stds=g["noise_stds"][None, None], SNRs=g["SNRs"][None, None], bw=float(g["bw"]),
                             source="fake", filename=name + ".npz")
    return DataPortrait(bunch, quiet=True), g, port


@pytest.mark.parametrize("name", sc.MODEL_CASES)
def test_significance_decisions_from_the_references_smoothed_statistics(name):
    from pulseportraiture_amd.ppspline import significant_eigvec
    g = _g(name)
    ieig, snrs = significant_eigvec(g["stats"][:, :4], pc.CASES[name][1])
    np.testing.assert_array_equal(ieig, g["ieig"])
    np.testing.assert_allclose(snrs, g["stats"][:len(snrs), 4], rtol=1e-13)


@pytest.mark.parametrize("name", sc.MODEL_CASES)
def test_make_smooth_spline_model_host_flow_and_the_spl_round_trip(name, tmp_path, capsys):
    from pulseportraiture_amd.splmodel import read_spline_model
    dp, g, port = _portrait(name)
    eng = GoldenEngine(g, port)
    dp.make_smooth_spline_model(engine=eng, model_name="a name", rchi2_tol=0.1)
    out = capsys.readouterr().out
    nbin = pc.CASES[name][1]
    pow2 = nbin & (nbin - 1) == 0
    assert ("not a power of two" in out) == (not pow2)
    assert eng.smooth_calls == [(10, int(np.log2(nbin)) if pow2 else 1, 0.1, "hard"), (1, int(np.log2(nbin)) if pow2 else 1, 0.1, "hard")]
    ie = g["ieig"]
    np.testing.assert_array_equal(dp.ieig, ie)
    np.testing.assert_array_equal(dp.smooth_eigvec[:, ie], g["smooth_eigvec"][:, ie])
    np.testing.assert_array_equal(dp.smooth_mean_prof, g["smooth_mean_prof"])
    np.testing.assert_array_equal(dp.mean_prof, g["mean_prof"])
    np.testing.assert_array_equal(dp.tck[0], g["t"])
    np.testing.assert_allclose(dp.proj_port, g["proj_port"], rtol=0, atol=1e-13 * np.abs(g["proj_port"]).max())
    np.testing.assert_allclose(np.array(dp.tck[1]), g["c"], rtol=0, atol=1e-9 * np.abs(g["c"]).max())
    np.testing.assert_allclose(dp.model[g["rows"]], g["model_rows"], rtol=0, atol=1e-9 * np.abs(g["model_rows"]).max())
    np.testing.assert_allclose(dp.reconst_port[g["rows_x"]], g["reconst_rows"], rtol=0, atol=1e-12 * np.abs(g["reconst_rows"]).max())
    dp.write_model(str(tmp_path / "m.spl"), quiet=True)
    model_name, source, datafile, mean_prof, eigvec, tck = read_spline_model(str(tmp_path / "m.spl"), quiet=True)
    assert model_name == "a name"
    np.testing.assert_array_equal(mean_prof, g["smooth_mean_prof"])          # the smoothed mean and vectors are written
    np.testing.assert_array_equal(eigvec, g["smooth_eigvec"][:, ie])


def test_zero_component_smoothed_model_is_the_tiled_smoothed_mean():
    dp, g, port = _portrait("64x256")
    dp.make_smooth_spline_model(engine=GoldenEngine(g, port), snr_cutoff=np.inf, quiet=True)
    assert dp.ncomp == 0 and dp.proj_port.shape == (64, 0) and not dp.smooth_eigvec.any()
    for m in (dp.model, dp.modelx, dp.reconst_port):
        np.testing.assert_array_equal(m, np.tile(g["smooth_mean_prof"], (64, 1)))


def test_an_odd_row_length_falls_back_to_the_unsmoothed_model(capsys):
    from pulseportraiture_amd import pplib
    x = np.arange(255.0)
    assert pplib.smart_smooth(x, try_nlevels=0) is x
    assert pplib.smart_smooth(x[None]) is not None and np.array_equal(pplib.smart_smooth(x), x[None])
    port = np.tile(x, (2, 1))
    assert pplib.smart_smooth(port) is port
    with pytest.raises(KeyError):
        pplib.smart_smooth(np.arange(256.0), wavelet="db8")      # the reference reads kwargs['wave']
    with pytest.raises(NotImplementedError):
        pplib.wavelet_smooth(np.arange(256.0), wavelet="sym4")
    stats = pplib.smooth_stats(x[None], x[None], None)
    assert stats.shape == (1, 4) and stats[0, 2] == 254.0


def test_parser_defaults_of_the_smoothing_command():
    from pulseportraiture_amd import ppspline_run, ppspline_smooth_run
    o = ppspline_smooth_run.parser().parse_args(["-d", "avg.npz"])
    assert (o.datafile, o.modelfile, o.model_name, o.archive, o.norm) == ("avg.npz", None, None, None, "prof")
    assert (int(o.max_ncomp), float(o.snr_cutoff), float(o.rchi2_tol), int(o.k), float(o.sfac)) == (10, 150.0, 0.1, 3, 1.0)
    assert o.max_nbreak is None and not o.make_plots and not o.quiet
    assert ppspline_run.refusal(o, ["avg.npz"], smooth=True) is None
    o = ppspline_smooth_run.parser().parse_args(["-d", "avg.npz", "-s", "-T", "0.3"])
    assert o.smooth and float(o.rchi2_tol) == 0.3 and ppspline_run.refusal(o, ["avg.npz"], smooth=True) is None
    assert "ppspline_smooth_run" in ppspline_smooth_run.parser().format_usage()


def test_the_smoothing_command_still_refuses_what_it_cannot_do(capsys):
    from pulseportraiture_amd.ppspline_smooth_run import main
    assert main(["-d", "avg.npz", "--plots"]) == 2
    assert capsys.readouterr().err.startswith("ppspline_smooth_run: ")


def test_the_two_refusals_still_name_pywavelets_and_point_to_the_new_route(capsys):
    from pulseportraiture_amd.ppspline_run import main
    dp, g, port = _portrait("64x256")
    with pytest.raises(NotImplementedError, match="PyWavelets") as e:
        dp.make_spline_model(engine=GoldenEngine(g, port))
    assert "make_smooth_spline_model" in str(e.value) and "ppspline_smooth_run" in str(e.value)
    assert main(["-d", "avg.npz", "-s"]) == 2
    err = capsys.readouterr().err
    assert "PyWavelets" in err and "ppspline_smooth_run" in err and "make_smooth_spline_model" in err
