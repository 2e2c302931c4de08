"""The callers of the fit's residual portrait: GetTOAs.show_fit against the reference's own show_fit
(tests/golden/showfit.npz), GetTOAs.get_residuals against show_fit, and the ppresid_run command line on simulated
archives.

Bars.  show_fit's port and model_scaled: the kernel's bar, rot_bar(nbin) x (max |data row| + |a_n| max |model row|)
(tests/test_gpu_resid_kernels.py), plus 2 pi (nbin / 2) |dphi_n| max |row| -- what the difference dphi_n between this
package's fitted delay of channel n and the reference's does to a rotated row, to first order.  dphi_n is measured and
written to the parity file (PP_PPRESID_PARITY_OUT, profiles/ppresid_parity.json).  get_residuals against
port - model_scaled: twice the kernel's bar (two inverse transforms against one).  The command's reduced chi^2: 1 +- 5 sqrt(2 / dof), five standard deviations of a chi^2 of that
many degrees of freedom; noiseless data: a residual below 1e-9 of the data's maximum."""
import os
import re

import numpy as np
import pytest

from tests import ppfake_cases as pc
from tests import rot_refs as rr
from tests.gpu_support import default_eng, measured_writer, run_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MEASURED, _write_measured = measured_writer("PP_PPRESID_PARITY_OUT")
CASES = ["zap", "gm", "scat", "rot"]


def _golden():
    return np.load(os.path.join(GOLDEN, "showfit.npz"))


def _gettoas(g, name):
    """GetTOAs on the golden's arrays, fitted with the reference's seed and solver and the golden's keywords."""
    from pulseportraiture_amd.pptoas import GetTOAs, MJD, data_from_arrays
    v = lambda k: g["%s_%s" % (name, k)]        # noqa: E731
    epochs = [MJD(int(d), float(f)) for d, f in zip(v("epoch_days"), v("epoch_fracs"))]
    data = data_from_arrays(
        v("subints"), v("freqs"), v("Ps"), epochs, weights=v("weights"), noise_stds=v("noise_stds"), SNRs=v("SNRs"),
        DM=float(v("scal_DM")), doppler_factors=v("doppler_factors"), backend_delay=float(v("scal_backend_delay")),
        telescope=str(v("scal_telescope")), telescope_code=str(v("scal_telescope_code")), backend=str(v("scal_backend")),
        frontend=str(v("scal_frontend")), bw=float(v("scal_bw")), nu0=float(v("scal_nu0")), subtimes=v("subtimes"),
        source=str(v("scal_source")), filename="fake.fits")
    kw = {}
    for k in g.files:
        if k.startswith(name + "_kw_"):
            a = g[k]
            kw[k[len(name) + 4:]] = a.item() if a.ndim == 0 else tuple(a.tolist())
    gt = GetTOAs(data, os.path.join(GOLDEN, "example.gmodel"), quiet=True)
    gt.get_TOAs(quiet=True, seed='reference', **kw)
    return gt, data


def _delays(phi, DM, GM, df, nu_refs, freqs, P):
    return np.array([float(rr.delay_ld(phi, DM / df, GM / df ** 3, nu, nu_refs[0], nu_refs[1], P)) for nu in freqs])


@pytest.fixture(scope="module")
def fitted():
    g = _golden()
    return g, {name: _gettoas(g, name) for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_show_fit_returns_the_references_tuple(fitted, name):
    g, fits = fitted
    gt, data = fits[name]
    v = lambda k: g["%s_%s" % (name, k)]        # noqa: E731
    isub, rotate = int(v("isub")), float(v("rotate"))
    port, model_scaled, ok_ichans, freqs, noise_stds = gt.show_fit(isub=isub, rotate=rotate)
    np.testing.assert_array_equal(ok_ichans, v("fit_ok_ichans"))
    np.testing.assert_array_equal(freqs, v("fit_freqs"))
    np.testing.assert_array_equal(noise_stds, v("fit_noise_stds"))
    nbin = port.shape[-1]
    df = lambda d: d[isub] if int(v("bary")) else 1.0        # noqa: E731
    mine = _delays(gt.phis[0][isub], gt.DMs[0][isub], gt.GMs[0][isub], df(gt.doppler_fs[0]), gt.nu_refs[0][isub], freqs,
                   data.Ps[isub])
    theirs = _delays(v("out_phis")[isub], v("out_DMs")[isub], v("out_GMs")[isub], df(v("out_doppler_fs")),
                     v("out_nu_refs")[isub], freqs, data.Ps[isub])
    dphi = np.abs(mine - theirs)
    rowmax = np.abs(v("subints")[isub, 0]).max(axis=-1) + np.abs(v("fit_model_scaled")).max(axis=-1)
    for got, want, what in ((port, v("fit_port"), "port"), (model_scaled, v("fit_model_scaled"), "model_scaled")):
        assert got.shape == want.shape and got.dtype == np.float64
        bar = rr.rot_bar(nbin) * rowmax + 2 * np.pi * (nbin // 2) * dphi * np.abs(want).max(axis=-1)
        dev = np.abs(got - want).max(axis=-1)
        live = bar > 0
        worst = float((dev[live] / bar[live]).max())
        MEASURED.setdefault("show_fit " + what, {})[name] = dict(
            deviation=float(dev.max()), of_bar=worst, dphi_n_max=float(dphi.max()), kernel_bar=float((rr.rot_bar(nbin) * rowmax).max()))
        print(name, what, "worst row %.3e, %.3f of its bar; max |dphi_n| %.2e rot" % (float(dev.max()), worst, float(dphi.max())))
        assert np.all(dev <= bar), (name, what, worst)
    zapped = np.setdiff1d(np.arange(data.nchan), ok_ichans)
    assert not port[zapped].any() and not model_scaled[zapped].any()


def test_show_fit_refuses_plots(fitted):
    gt, _ = fitted[1]["zap"]
    for kw in (dict(show=True), dict(savefig=True)):
        with pytest.raises(NotImplementedError, match="plots are outside the accelerated path"):
            gt.show_fit(**kw)
    assert gt.show_fit(return_fit=False) is None


@pytest.mark.parametrize("name", ["zap", "gm", "scat"])
def test_get_residuals_is_show_fits_difference(fitted, name):
    """Every fitted subint, frame "model", host and device output; unfitted channels are zero rows with NaN chi^2; the
    chi^2 is the residual's own sum of squares; get_channels_to_zap's figure is the same number."""
    gt, data = fitted[1][name]
    res = gt.get_residuals(frame="model")
    assert res.resid.shape == (data.nsub, data.nchan, data.nbin) and res.channel_red_chi2.shape == (data.nsub, data.nchan)
    np.testing.assert_array_equal(res.ok_isubs, gt.ok_isubs[0])
    dev = gt.get_residuals(frame="model", on_device=True)
    assert dev.resid.is_cuda and dev.resid.cpu().numpy().tobytes() == res.resid.tobytes()
    gt.channel_red_chi2s, gt.zap_channels = [], []
    gt.get_channels_to_zap()
    for j, isub in enumerate(res.ok_isubs):
        port, model_scaled, ok_ichans, _, noise = gt.show_fit(isub=int(isub))
        np.testing.assert_array_equal(res.ok_ichans[isub], ok_ichans)
        bar = 2 * rr.rot_bar(data.nbin) * (np.abs(data.subints[isub, 0]).max(axis=-1) + np.abs(model_scaled).max(axis=-1))
        diff = np.abs(res.resid[isub] - (port - model_scaled)).max(axis=-1)
        MEASURED.setdefault("get_residuals vs show_fit", {})["%s-%d" % (name, isub)] = dict(
            deviation=float(diff.max()), of_bar=float((diff / bar).max()))
        assert np.all(diff <= bar), (name, isub, float((diff / bar).max()))
        zapped = np.setdiff1d(np.arange(data.nchan), ok_ichans)
        assert not res.resid[isub][zapped].any() and np.isnan(res.channel_red_chi2[isub][zapped]).all()
        own = np.sum(res.resid[isub][ok_ichans] ** 2, axis=-1) / noise[ok_ichans] ** 2 / (data.nbin - 2)
        np.testing.assert_allclose(res.channel_red_chi2[isub][ok_ichans], own, rtol=1e-9)
        assert np.array_equal(res.channel_red_chi2[isub][ok_ichans], np.asarray(gt.channel_red_chi2s[0][j]))
    back = gt.get_residuals(frame="data")
    np.testing.assert_array_equal(back.channel_red_chi2, res.channel_red_chi2)
    assert not np.array_equal(back.resid, res.resid)


# ---- the command line ----------------------------------------------------------------------------------------
SHAPE = ["--nfiles", "2", "--nsub", "3", "--nchan", "8", "--nbin", "64"]
LINE = re.compile(r"^(\S+): (\d+) fitted subint\(s\), reduced chi2 (\S+) \(dof (\d+)\), largest \|residual\|/sigma (\S+) at "
                  r"\(subint (\d+), channel (\d+), bin (\d+)\)$")


SMOOTH = """MODEL   smooth
CODE    000
FREQ    1500.00000
DC      0.00000000 0
TAU     0.00000000 0
ALPHA  -4.000      0
COMP01  0.30000000 0   0.00200000 0   0.15000000 0   0.00000000 0    1.00000000 0   -1.00000000 0
COMP02  0.55000000 0  -0.00100000 0   0.22000000 0   0.00000000 0    0.50000000 0   -0.50000000 0
"""


def _fake(tmp_path, noise_std, more=(), model=pc.GMODEL):
    args = ["-m", model, "-e", pc.PARFILE, "-o", "fake-%d.npz", "--dDM", "2e-4,-3e-4", "--phase", "0.03", "--noise_std",
            "%.6g" % noise_std, "--seed", "11", "--metafile", "list.txt", "--quiet", "--f64"] + SHAPE + list(more)
    run_module("ppfake_run", args, tmp_path, 120)
    return ["fake-1.npz", "fake-2.npz"]


def _peak():
    from pulseportraiture_amd.gmodel import gaussian_portrait, read_gmodel
    from pulseportraiture_amd.parfile import psr_par
    freqs = np.linspace(1100.0 + 50.0, 1900.0 - 50.0, 8)
    return float(gaussian_portrait(read_gmodel(pc.GMODEL), freqs, 64, psr_par(pc.PARFILE).P0).max())


def test_ppresid_run_writes_archives_with_a_chi2_of_one(tmp_path):
    from pulseportraiture_amd import archive
    names = _fake(tmp_path, 0.05 * _peak())
    out = run_module("ppresid_run", ["-d", "list.txt", "-m", pc.GMODEL, "--DM", "34.56789", "--metafile", "out.txt"], tmp_path, 300)
    lines = [LINE.match(ln) for ln in out.splitlines() if "fitted subint" in ln]
    assert len(lines) == 2 and all(lines), out
    written = (tmp_path / "out.txt").read_text().split()
    assert [os.path.basename(w) for w in written] == ["fake-1.resid.npz", "fake-2.resid.npz"]
    for m, name, w in zip(lines, names, written):
        src, _ = archive.load_archive(str(tmp_path / name), default_eng())
        res, _ = archive.load_archive(str(tmp_path / os.path.basename(w)), default_eng())
        assert res.subints.shape == src.subints.shape == (3, 1, 8, 64) and res.subints.dtype == src.subints.dtype
        assert int(res.dmc) == int(src.dmc) and float(res.DM) == float(src.DM)
        np.testing.assert_array_equal(res.freqs, src.freqs)
        nfit, red, dof = int(m.group(2)), float(m.group(3)), int(m.group(4))
        assert nfit == 3 and dof == 3 * 8 * 62
        print(name, "reduced chi2 %.4f, bar 1 +- %.4f" % (red, 5 * np.sqrt(2.0 / dof)), "worst", m.group(5))
        MEASURED.setdefault("ppresid_run reduced chi2", {})[name] = dict(red_chi2=red, dof=dof, bar=5 * np.sqrt(2.0 / dof))
        assert abs(red - 1.0) <= 5 * np.sqrt(2.0 / dof)
        assert np.abs(res.subints).max() < 0.5 * np.abs(src.subints).max()
        i, n, b = (int(m.group(k)) for k in (6, 7, 8))
        assert float(m.group(5)) == pytest.approx(abs(res.subints[i, 0, n, b]) / src.noise_stds[i, 0, n], abs=2e-3)


def test_ppresid_run_on_noiseless_data_leaves_nothing(tmp_path):
    """The template here has components of FWHM 0.15 and 0.22 rot: its harmonics at and near Nyquist of 64 bins are
    below 1e-35 of the peak.  (A rotation keeps only the real part of the Nyquist harmonic, so a template with power
    there -- example.gmodel has 5e-3 of its peak at 64 bins -- cannot be taken out of rotated data to better than
    that, whatever forms the residual.)  The fit is --seed device, whose Newton solver iterates until its step is rounding:
    measured 1.6e-10 and 1.7e-10 of the data's maximum for the two archives.  The default retraces SciPy's trust-ncg and
    stops where that stops: measured with it, 0.8e-9 and 2.7e-9."""
    (tmp_path / "smooth.gmodel").write_text(SMOOTH)
    names = _fake(tmp_path, 0.0, model="smooth.gmodel")
    run_module("ppresid_run", ["-d", "list.txt", "-m", "smooth.gmodel", "--DM", "34.56789", "--seed", "device", "--quiet"],
               tmp_path, 300)
    for name in names:
        with np.load(str(tmp_path / name)) as z, np.load(str(tmp_path / name.replace(".npz", ".resid.npz"))) as r:
            ratio = float(np.abs(r["subints"]).max() / np.abs(z["subints"]).max())
        print(name, "largest residual: %.3e of the data's maximum" % ratio)
        MEASURED.setdefault("ppresid_run noiseless residual", {})[name] = dict(of_data_max=ratio, bar=1e-9)
        assert ratio < 1e-9
    # the default seed's figures, for the record beside the others (README.md states them); held only to 2e-8, what
    # the 1e-9 rot the fit's phase is held to against the reference (tests/test_gpu_parity.py PHI_BAR) does to a pulse
    # whose power ends at the third harmonic: 2 pi 3 1e-9 = 1.9e-8 of its amplitude
    run_module("ppresid_run", ["-d", "list.txt", "-m", "smooth.gmodel", "--DM", "34.56789", "-e", "dflt.npz", "--quiet"], tmp_path, 300)
    for name in names:
        with np.load(str(tmp_path / name)) as z, np.load(str(tmp_path / name.replace(".npz", ".dflt.npz"))) as r:
            ratio = float(np.abs(r["subints"]).max() / np.abs(z["subints"]).max())
        print(name, "default seed, largest residual: %.3e of the data's maximum" % ratio)
        MEASURED.setdefault("ppresid_run noiseless residual, default seed", {})[name] = dict(of_data_max=ratio, bar=2e-8)
        assert ratio < 2e-8


def test_ppresid_run_model_frame_scrunches_to_one_subint(tmp_path):
    _fake(tmp_path, 0.05 * _peak())
    run_module("ppresid_run", ["-d", "fake-1.npz", "-m", pc.GMODEL, "--DM", "34.56789", "--frame", "model", "-e", "tf.npz",
                               "--quiet"], tmp_path, 300)
    run_module("ppscrunch_run", ["-d", "fake-1.tf.npz", "-T", "--quiet"], tmp_path, 300)
    with np.load(str(tmp_path / "fake-1.tf.npz")) as r, np.load(str(tmp_path / "fake-1.tf.scr.npz")) as s:
        assert int(r["dmc"]) == 1 and r["subints"].shape == (3, 1, 8, 64)
        assert s["subints"].shape == (1, 1, 8, 64)
        # the mean of the aligned residuals: noise goes down, and it is what ppscrunch adds up
        np.testing.assert_allclose(s["subints"][0, 0], r["subints"][:, 0].mean(axis=0), atol=1e-6 * np.abs(r["subints"]).max())


def _top_quarter_noise(rows):
    """get_noise_PS of every row: sqrt of the mean of |rfft|^2 / nbin over the top quarter of the harmonics."""
    pows = np.abs(np.fft.rfft(rows, axis=-1)) ** 2 / rows.shape[-1]
    return np.sqrt(pows[..., int(0.75 * pows.shape[-1]):].mean(axis=-1))


def test_ppresid_run_data_frame_of_a_dedispersed_archive_is_in_the_stored_frame(tmp_path):
    """An archive stored dedispersed (dmc = 1) is put back before the fit, so --frame data turns the residual to the
    stored state again: data - residual is then the model alone.  The template is the smooth one (no power in the top
    quarter of 64 bins' harmonics), so the noise estimate of data - residual holds only what two rotations in a row
    cost the residual: at most its Nyquist harmonic, one of the nine harmonics of that quarter -- a third of the data's
    estimate.  A residual left in the dispersed frame would not cancel the data's noise at all (sqrt(2) of it).  Bar:
    half the data's estimate, in every row."""
    (tmp_path / "smooth.gmodel").write_text(SMOOTH)
    _fake(tmp_path, 0.05, more=("--dedispersed",), model="smooth.gmodel")
    run_module("ppresid_run", ["-d", "fake-1.npz", "-m", "smooth.gmodel", "--DM", "34.56789", "--quiet"], tmp_path, 300)
    with np.load(str(tmp_path / "fake-1.npz")) as z, np.load(str(tmp_path / "fake-1.resid.npz")) as r:
        assert int(z["dmc"]) == 1 and int(r["dmc"]) == 1
        data, resid = z["subints"][:, 0], r["subints"][:, 0]
    ratio = _top_quarter_noise(data - resid) / _top_quarter_noise(data)
    print("noise of data - residual over the data's, worst row: %.3f" % float(ratio.max()))
    MEASURED.setdefault("ppresid_run dedispersed archive", {})["fake-1.npz"] = dict(worst_noise_ratio=float(ratio.max()), bar=0.5)
    assert np.all(ratio < 0.5)
    assert np.all(_top_quarter_noise(resid) > 0.5 * _top_quarter_noise(data))      # (the residual keeps the noise)


def test_ppresid_run_refuses_more_than_one_polarisation(tmp_path):
    from tests.gpu_support import child_env
    import subprocess
    import sys
    _fake(tmp_path, 0.05 * _peak(), more=("--npol", "4"))
    p = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.ppresid_run", "-d", "fake-1.npz", "-m", pc.GMODEL],
                       cwd=str(tmp_path), env=child_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "4 polarisations" in p.stderr
