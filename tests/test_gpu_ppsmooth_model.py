"""Smoothed .spl templates on the GPU against the true reference's make_spline_model(smooth=True) run on the PyWavelets
stand-in (tests/golden/ppsmooth_model_*.npz, from make_golden_ppsmooth.py).

Decisions -- the significant eigenvectors, every vector's level and evaluation count, the knots -- are compared
exactly; the golden script asserts that no coefficient lies within 1e-9 lopt of lopt at any factor the reference
evaluated, and that no S/N is within 1e-6 of a cutoff.

Values.  What goes INTO the smoothing, the eigenvectors and the mean profile, carries the reference's own scatter: how
far each moves when the reference is handed the channels in another order (scat_* in ppspline_<case>.npz; 1e-15 for
the leading eigenvector, 7e-11 for the seventh of 48x1000, whose eigenvalue is nearly degenerate).  The unsmoothed
tests allow ten times that, floored at 1e-13 of the scale.  For a fixed threshold mask the smoothing is a linear map
of 2-norm <= 1 (thresholding inside a tight frame), so an input deviation d reaches the smoothed vector as at most
sqrt(nbin) |d|_inf.  The bar of every smoothed quantity is therefore sqrt(nbin) times the unsmoothed test's bar of the
quantity it is made from, per eigenvector where there is one.  Eigenvector signs are aligned by the dot product with
the reference's column (smoothing is odd).
"""
import os
import pickle

import numpy as np
import pytest

from tests import ppsmooth_cases as sc
from tests import ppspline_cases as pc
from tests.gpu_support import run_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P0 = 0.003


def _g(name):
    return np.load(os.path.join(GOLDEN, "ppsmooth_model_%s.npz" % name))


def _port(name):
    port = pc.make_input(name)[0]
    assert pc.sha256(port) == str(_g(name)["input_sha256"]), "the regenerated input is not the reference's"
    return port


def _portrait(name):
    from pulseportraiture_amd.ppspline import DataPortrait
    from pulseportraiture_amd.pptoas import data_from_arrays
    g = _g(name)
    return DataPortrait(data_from_arrays(_port(name)[None, None], g["freqs"], [P0], [55000.0], weights=g["weights"][None],
                                         noise_stds=g["noise_stds"][None, None], SNRs=g["SNRs"][None, None],
                                         bw=float(g["bw"]), source="fake", filename=name + ".npz"), quiet=True)


class Bars(object):
    """sqrt(nbin) x the bars of tests/test_gpu_ppspline.py (10 x the reference's scatter, floored at 1e-13 of the
    scale) for the quantities of case `name`; per-eigenvector quantities by the eigenvector's index."""

    def __init__(self, name):
        self.u = np.load(os.path.join(GOLDEN, "ppspline_%s.npz" % name))
        self.amp = np.sqrt(pc.CASES[name][1])

    def whole(self, key, scale):
        return self.amp * max(10.0 * float(np.max(self.u["scat_" + key])), 1e-13 * scale)

    def columns(self, key, cols, scales):
        """Per eigenvector `cols`: scat_eigvec is indexed by the eigenvector, scat_proj_port / scat_c by the position in
        the unsmoothed run's ieig (an eigenvector that run did not keep takes the largest scatter it recorded)."""
        scat = np.asarray(self.u["scat_" + key], dtype=np.float64)
        if key != "eigvec":
            pos = {int(c): i for i, c in enumerate(self.u["ieig"])}
            scat = np.array([scat[pos[int(c)]] if int(c) in pos else scat.max() for c in cols])
        else:
            scat = scat[cols]
        return self.amp * np.maximum(10.0 * scat, 1e-13 * np.asarray(scales, dtype=np.float64))


def _close(key, got, want, bar):
    dev = np.abs(np.asarray(got) - np.asarray(want))
    print("%-18s dev %.3e  bar %.3e" % (key, dev.max() if dev.size else 0.0, np.min(bar)))
    return bool(np.all(dev <= bar))


def _check_model(name, mean_prof, eigvec, tck, ieig=None):
    g, b = _g(name), Bars(name)
    ie = g["ieig"]
    if ieig is not None:
        np.testing.assert_array_equal(ieig, ie)
    assert eigvec.shape == (len(g["mean_prof"]), len(ie))
    sg = np.sign(np.sum(eigvec * g["smooth_eigvec"][:, ie], axis=0))
    np.testing.assert_array_equal(tck[0], g["t"])
    assert tck[2] == int(g["k"])
    bad = [k for k, ok in (
        ("smooth_mean_prof", _close("smooth_mean_prof", mean_prof, g["smooth_mean_prof"], b.whole("mean_prof", np.abs(g["mean_prof"]).max()))),
        ("smooth_eigvec", _close("smooth_eigvec", eigvec * sg, g["smooth_eigvec"][:, ie], b.columns("eigvec", ie, np.ones(len(ie)))[None, :])),
        ("coefficients", _close("coefficients", np.array(tck[1]) * sg[:, None], g["c"],
                                b.columns("c", ie, np.abs(g["c"]).max(axis=1))[:, None]))) if not ok]
    assert not bad, bad
    return sg


@pytest.mark.parametrize("name", sc.MODEL_CASES)
def test_make_smooth_spline_model_against_the_reference(name):
    g = _g(name)
    dp = _portrait(name)
    dp.make_smooth_spline_model(quiet=True, **pc.CASES[name][5])
    sg = _check_model(name, dp.smooth_mean_prof, dp.smooth_eigvec[:, dp.ieig], dp.tck, dp.ieig)
    ie, b = g["ieig"], Bars(name)
    mscale = np.abs(g["model_rows"]).max()
    # vectors that are not significant stay zero in smooth_eigvec; the raw basis and mean are kept beside it
    assert not dp.smooth_eigvec[:, [i for i in range(10) if i not in ie]].any()
    assert dp.eigvec.shape == dp.smooth_eigvec.shape
    assert _close("mean_prof", dp.mean_prof, g["mean_prof"], b.whole("mean_prof", np.abs(g["mean_prof"]).max()) / b.amp)
    nfreq = len(g["freqs"])
    assert dp.model.shape == (nfreq, len(g["mean_prof"]))
    bad = [k for k, ok in (
        ("proj_port", _close("proj_port", dp.proj_port * sg, g["proj_port"],
                             b.columns("proj_port", ie, np.abs(g["proj_port"]).max(axis=0))[None, :])),
        ("modelx", _close("modelx", dp.modelx[g["rows_x"]], g["modelx_rows"], b.whole("modelx", mscale))),
        ("model", _close("model", dp.model[g["rows"]], g["model_rows"], b.whole("model", mscale))),
        # (the reconstruction is a sum of the same products as the model's rows)
        ("reconst_port", _close("reconst_port", dp.reconst_port[g["rows_x"]], g["reconst_rows"], b.whole("modelx", mscale)))) if not ok]
    assert not bad, bad
    # the decisions of every examined vector, then the mean profile: level and evaluations exactly, factor to 1e-12
    from pulseportraiture_amd import pplib
    rows = np.vstack([dp.eigvec.T, dp.mean_prof[None]])
    _, info = pplib.smart_smooth(rows, return_info=True)
    np.testing.assert_array_equal(info["level"], g["levels"])
    np.testing.assert_array_equal(info["nfev"], g["nfevs"])
    np.testing.assert_allclose(info["fact"], g["facts"], rtol=0, atol=1e-12)
    ieig2, sev = pplib.find_significant_eigvec(dp.eigvec)
    np.testing.assert_array_equal(ieig2, ie)
    np.testing.assert_array_equal(sev, dp.smooth_eigvec)
    # the unsmoothed model of the same object drops the smoothed attributes again
    dp.make_spline_model(smooth=False, quiet=True)
    assert not hasattr(dp, "smooth_eigvec") and not hasattr(dp, "smooth_mean_prof")


@pytest.mark.parametrize("name", sc.MODEL_CASES)
def test_command_line_writes_the_references_smoothed_model(name, tmp_path):
    from pulseportraiture_amd.splmodel import read_spline_model
    g = _g(name)
    np.savez(tmp_path / "avg.npz", subints=_port(name)[None, None], freqs=g["freqs"][None], Ps=np.array([P0]),
             epochs=np.array([55000.0]), weights=g["weights"][None], noise_stds=g["noise_stds"][None, None],
             bw=float(g["bw"]), source="fake", SNRs=g["SNRs"][None, None])
    out = run_module("ppspline_smooth_run", ["-d", "avg.npz", "-N", "None", "-l", "the model", "-s"], tmp_path, 300)
    assert "Wrote modelfile avg.npz.spl." in out and "uses %d basis" % len(g["ieig"]) in out
    model_name, source, datafile, mean_prof, eigvec, tck = read_spline_model(str(tmp_path / "avg.npz.spl"), quiet=True)
    assert (model_name, source, datafile) == ("the model", "fake", "avg.npz")
    _check_model(name, mean_prof, eigvec, tck)


def test_rchi2_tol_takes_effect(tmp_path):
    """-T 0 lets no smoothed candidate pass: every vector comes back zero and the model is the (zeroed) mean profile."""
    dp = _portrait("64x256")
    dp.make_smooth_spline_model(quiet=True, rchi2_tol=0.0)
    assert dp.ncomp == 0 and not dp.smooth_mean_prof.any() and not dp.model.any()


def test_toas_with_the_smoothed_template_are_the_references():
    """GetTOAs on 8 synthetic subints with the smoothed .spl written here against the same call with a .spl pickled
    from the reference's smoothed outputs: |dphi| <= 1e-9 rot, the standing caller-level bar."""
    import tempfile
    from pulseportraiture_amd.gmodel import example_model
    from pulseportraiture_amd.pplib import rotate_data
    from pulseportraiture_amd.pptoas import GetTOAs, data_from_arrays
    name = "64x256"
    g = _g(name)
    dp = _portrait(name)
    dp.make_smooth_spline_model(quiet=True)
    tmp = tempfile.mkdtemp(prefix="ppsmooth_e2e_")
    mine, theirs = os.path.join(tmp, "mine.spl"), os.path.join(tmp, "reference.spl")
    dp.write_model(mine, quiet=True)
    ie = g["ieig"]
    sg = np.sign(np.sum(dp.smooth_eigvec[:, ie] * g["smooth_eigvec"][:, ie], axis=0))
    with open(theirs, "wb") as f:
        pickle.dump([dp.model_name, dp.source, dp.datafile, g["smooth_mean_prof"], g["smooth_eigvec"][:, ie] * sg,
                     [g["t"], list(g["c"] * sg[:, None]), int(g["k"])]], f, protocol=2)
    freqs, clean, P = example_model(64, 256)
    rng = np.random.default_rng(99)
    nsub = 8
    subints = np.empty((nsub, 1, 64, 256))
    for i in range(nsub):
        subints[i, 0] = rotate_data(clean, -rng.uniform(-0.3, 0.3), -rng.normal(0.0, 3e-4), P, freqs, np.inf) + \
            0.05 * rng.standard_normal(clean.shape)
    phis = []
    for modelfile in (mine, theirs):
        data = data_from_arrays(subints, freqs, np.full(nsub, P), [55000.0 + i for i in range(nsub)], bw=800.0,
                                filename="synthetic.npz")
        gt = GetTOAs(data, modelfile, quiet=True)
        gt.get_TOAs(quiet=True)
        assert len(gt.ok_isubs[0]) == nsub
        phis.append(np.array(gt.phis[0]))
    dphi = np.abs((phis[0] - phis[1] + 0.5) % 1.0 - 0.5)
    print("end to end: max |dphi| = %.3e rot" % dphi.max())
    assert np.all(dphi <= 1e-9), dphi


def test_smooth_portrait_side_effects():
    from pulseportraiture_amd import pplib
    dp = _portrait("64x256")
    port0 = dp.port.copy()
    dp.smooth_portrait(smart=False, nlevel=4, fact=1.0)
    want = pplib.wavelet_smooth(port0, nlevel=4, fact=1.0)
    np.testing.assert_array_equal(dp.port, want)
    np.testing.assert_array_equal(dp.portx, want[dp.ok_ichans[0]])
    np.testing.assert_allclose(dp.noise_stds[0, 0], pplib.get_noise(want, chans=True), rtol=1e-11)
    np.testing.assert_allclose(dp.noise_stdsxs, pplib.get_noise(want, chans=True)[dp.ok_ichans[0]], rtol=1e-11)
    np.testing.assert_array_equal(dp.flux_prof, want.mean(axis=1))
    np.testing.assert_array_equal(dp.flux_profx, dp.portx.mean(axis=1))
    dp2 = _portrait("64x256")
    dp2.smooth_portrait(smart=True)
    np.testing.assert_array_equal(dp2.port, pplib.smart_smooth(port0, try_nlevels=8))
    assert np.abs(dp2.port - port0).max() > 0
