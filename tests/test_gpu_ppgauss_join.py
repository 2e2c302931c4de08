"""Joined multi-band ppgauss fits on the device against the TRUE reference (tests/golden/make_golden_ppgauss_join.py):
the residual rows of a band map and a join table, the golden joined fits through the engine, make_gaussian_model on
two bands, and the command line from two archives to TOAs.

Bars
  residual rows   the unjoined rows test's bar (2e-14 max|model| over sigma_n plus one ulp of |data| / sigma_n) plus
                  2 pi M max|phi_n| eps max|model| / sigma_n: the rounding of the rotation phasor's argument 2 pi k phi_n
                  (k <= M = nbin / 2), which the device (k phi_n exactly, reduced modulo 1) and NumPy (the rounded
                  product) round independently
  bitwise         rows whose rotation is zero are the unjoined rows; a set's rows do not depend on its neighbours
  fits            tests/test_gpu_ppgauss.py's _check_fit: within 10 x the golden's self-scatter and 1e-3 sigma, chi2 <=
                  golden (1 + 1e-9), errors to 1e-4, the same dof
  make_gaussian_model   every pass's phase and DM within the legacy fit_portrait bars (1e-9 rot, 1e-6 cm^-3 pc) of the
                  reference's, the .join numbers within the fit bars, the written model within 6e-9 of the fitted
                  parameters; model and data with the offsets taken out again against NumPy at 8e-14 of the peak
With PP_PPGAUSS_JOIN_PARITY_OUT set, the achieved distances are written there as JSON
(profiles/ppgauss_join_parity.json)."""
import os

import numpy as np
import pytest

from tests.gpu_support import eng, measured_writer, run_module  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MEASURED, _write_measured = measured_writer("PP_PPGAUSS_JOIN_PARITY_OUT")
PHI_BAR, DM_BAR = 1e-9, 1e-6        # the legacy fit_portrait golden test's bars (tests/test_gpu_parity.py)
Dconst = 0.000241 ** -1


def _g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def join_ichans_of(g, prefix="join_ichans"):
    out = []
    while prefix + str(len(out)) in g.files:
        out.append(g[prefix + str(len(out))])
    return out


NJ = 2          # bands of the rows golden


def _set_args(sets, nbin, njoin=NJ):
    """(positional, join) of Engine.gauss_residuals for vectors [DC, tau, comps ..., phase1, DM1, ..., alpha]."""
    sets = np.atleast_2d(sets)
    nm = sets.shape[1] - 1 - 2 * njoin
    return ((sets[:, 0], sets[:, 1] / nbin, sets[:, -1], sets[:, 2:nm].reshape(len(sets), (nm - 2) // 6, 6)),
            sets[:, nm:-1].reshape(len(sets), njoin, 2))


def _rows_case(g, nbin):
    band = np.full(len(g["freqs"]), -1)
    band[g["band0"]], band[g["band1"]] = 0, 1
    return g["n%d_data" % nbin], g["errs"], g["freqs"], band


def _rotations(g, sets, band):
    """phi_n of every set and channel (0 for the channel in no band)."""
    join = np.atleast_2d(sets)[:, -5:-1].reshape(-1, NJ, 2)
    k = Dconst / float(g["P"]) * (g["freqs"] ** -2.0 - float(g["nu_ref"]) ** -2.0)
    phi = join[:, np.maximum(band, 0), 0] + join[:, np.maximum(band, 0), 1] * k[None]
    return np.where(band[None] >= 0, phi, 0.0)


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_joined_residual_rows_against_the_reference(eng, nbin, code, scattered):
    """fit_gaussian_portrait_function with join_ichans on the edge model (Nyquist power at 64 bins): 7 channels, two
    bands and a channel in none; the seven sets step phase2, DM1, DM2, tau, a loc and the scattering index, so one
    launch holds sets that differ in join parameters, in tau and in alpha."""
    g = _g("ppgauss_join_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    data, errs, freqs, band = _rows_case(g, nbin)
    sets, want = g[tag + "_sets"], g[tag + "_rows"].reshape(7, len(freqs), nbin)
    eng.gauss_fit_begin(data, freqs, errs)
    try:
        eng.gauss_fit_join(band, float(g["P"]))
        worst = 0.0
        for pick in ([0], [0, 1], list(range(7)), [3, 6, 1]):
            args, join = _set_args(sets[pick], nbin)
            got = eng.gauss_residuals(code, float(g["nu_ref"]), *args, fetch=True, join=join)
            assert got.shape == (len(pick), len(freqs), nbin)
            model = data[None] - want[pick] * errs[None, :, None]
            phimax = np.abs(_rotations(g, sets[pick], band)).max()
            bar = (2e-14 * np.abs(model).max() / errs + np.spacing(np.abs(data).max(axis=1) / errs) +
                   2 * np.pi * (nbin // 2) * phimax * np.finfo(np.float64).eps * np.abs(model).max() / errs)
            dev = np.abs(got - want[pick])
            worst = max(worst, float((dev / bar[None, :, None]).max()))
            assert np.all(dev <= bar[None, :, None]), (tag, pick, float((dev / bar[None, :, None]).max()))
        MEASURED.setdefault("residual_rows", {})[tag] = dict(of_bar=worst)
        print(tag, "worst deviation %.3f of the bar" % worst)
    finally:
        eng.gauss_fit_end()


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("scattered", [0, 1])
def test_zero_join_parameters_are_the_unjoined_rows_bitwise(eng, nbin, scattered):
    """With a band map resident, sets whose join parameters are all zero -- as a table of zeros, or as no table --
    give the bits of the same call on a fit without a band map: the unjoined fit did not change."""
    g = _g("ppgauss_join_rows")
    tag = "n%d_c011_t%d" % (nbin, scattered)
    data, errs, freqs, band = _rows_case(g, nbin)
    sets = g[tag + "_sets"].copy()
    sets[:, -5:-1] = 0.0
    args, join = _set_args(sets, nbin)
    assert not join.any()
    nu_ref = float(g["nu_ref"])
    eng.gauss_fit_begin(data, freqs, errs)
    try:
        plain = eng.gauss_residuals("011", nu_ref, *args, fetch=True)
        eng.gauss_fit_join(band, float(g["P"]))
        zeros = eng.gauss_residuals("011", nu_ref, *args, fetch=True, join=join)
        none = eng.gauss_residuals("011", nu_ref, *args, fetch=True)
        # a second begin clears the band map
        eng.gauss_fit_begin(data, freqs, errs)
        again = eng.gauss_residuals("011", nu_ref, *args, fetch=True)
    finally:
        eng.gauss_fit_end()
    np.testing.assert_array_equal(zeros, plain)
    np.testing.assert_array_equal(none, plain)
    np.testing.assert_array_equal(again, plain)
    # ... and they are the reference's all-zero rows, to the unjoined rows test's bar
    want = g[tag + "_zero_rows"].reshape(len(freqs), nbin)
    model = data - want * errs[:, None]
    bar = 2e-14 * np.abs(model).max() / errs + np.spacing(np.abs(data).max(axis=1) / errs)
    assert np.all(np.abs(plain[0] - want) <= bar[:, None])


@pytest.mark.parametrize("nbin", [64, 100])
def test_rows_of_a_set_do_not_depend_on_the_launch(eng, nbin):
    """The rows of a set are the same bits alone, in a triple and among all seven -- also where the neighbours differ
    in tau, in alpha and in which bands they rotate; and a channel whose rotation is zero in a set keeps the bits it has
    without a band map (64 bins: no transform at all for such a row when tau is zero too; at 100 bins a set with a
    rotation anywhere takes all its rows through their harmonics, and an unscattered set's rows without a rotation are
    written again afterwards: tests/test_gpu_gauss_kernels.py holds them to the unjoined bits at every row length)."""
    g = _g("ppgauss_join_rows")
    data, errs, freqs, band = _rows_case(g, nbin)
    nu_ref = float(g["nu_ref"])
    for scattered in (0, 1):
        sets = g["n%d_c000_t%d_sets" % (nbin, scattered)]
        eng.gauss_fit_begin(data, freqs, errs)
        try:
            args, join = _set_args(sets, nbin)
            plain = eng.gauss_residuals("000", nu_ref, *args, fetch=True)
            eng.gauss_fit_join(band, float(g["P"]))
            full = eng.gauss_residuals("000", nu_ref, *args, fetch=True, join=join)
            for pick in ([0], [4], [3, 6, 1], [6, 5, 4, 3, 2, 1, 0]):
                args, join = _set_args(sets[pick], nbin)
                np.testing.assert_array_equal(eng.gauss_residuals("000", nu_ref, *args, fetch=True, join=join), full[pick])
        finally:
            eng.gauss_fit_end()
        # every row with a rotation is rotated; one without -- the channel in no band, and band 0's channel at nu_ref,
        # where a Delta-DM rotates nothing -- keeps its bits
        rot = _rotations(g, sets, band) != 0
        assert rot.sum() == rot.size - 2 * len(sets)
        moved = np.abs(full - plain).max(axis=-1) > 0
        assert np.all(moved[rot])
        if nbin == 64:
            assert not np.any(moved[~rot])


def test_join_refusals_return_messages_and_leave_the_fit_usable(eng):
    from pulseportraiture_amd.engine import EngineError
    g = _g("ppgauss_join_rows")
    data, errs, freqs, band = _rows_case(g, 64)
    P, nu_ref = float(g["P"]), float(g["nu_ref"])
    sets = g["n64_c000_t1_sets"][:2]
    args, join = _set_args(sets, 64)
    eng.gauss_fit_end()         # (whatever an earlier test left resident)
    with pytest.raises(EngineError, match="no fit is open"):
        eng.gauss_fit_join(band, P)
    eng.gauss_fit_begin(data, freqs, errs)
    try:
        want = eng.gauss_residuals("000", nu_ref, *args, fetch=True)
        with pytest.raises(EngineError, match="join parameters without a resident band map"):
            eng.gauss_residuals("000", nu_ref, *args, join=join)
        with pytest.raises(EngineError, match="0 bands"):
            eng.gauss_fit_join(np.full(7, -1), P)
        with pytest.raises(EngineError, match="17 bands"):
            eng.gauss_fit_join(band, P, njoin=17)
        with pytest.raises(EngineError, match=r"band_of_chan\[2\] = 1 is outside \[-1, 1\)"):
            eng.gauss_fit_join(band, P, njoin=1)
        low = band.copy()
        low[5] = -2
        with pytest.raises(EngineError, match=r"band_of_chan\[5\] = -2 is outside"):
            eng.gauss_fit_join(low, P)
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(EngineError, match="is no period"):
                eng.gauss_fit_join(band, bad)
        with pytest.raises(ValueError, match="one entry per resident channel"):
            eng.gauss_fit_join(band[:-1], P)
        # none of them made a band map resident, and the open fit still works
        with pytest.raises(EngineError, match="without a resident band map"):
            eng.gauss_residuals("000", nu_ref, *args, join=join)
        np.testing.assert_array_equal(eng.gauss_residuals("000", nu_ref, *args, fetch=True), want)
        eng.gauss_fit_join(band, P)
        with pytest.raises(ValueError, match="join holds 3 bands"):
            eng.gauss_residuals("000", nu_ref, *args, join=np.zeros((2, 3, 2)))
        with pytest.raises(ValueError, match=r"\[nsets,njoin,2\]"):
            eng.gauss_residuals("000", nu_ref, *args, join=np.zeros((3, 2, 2)))
        got = eng.gauss_residuals("000", nu_ref, *args, fetch=True, join=join)
        assert np.all(np.isfinite(got)) and np.abs(got - want).max() > 0
        chi2, gvec, G = eng.gauss_normal(np.array([1e-3]))
        assert np.isfinite(chi2) and chi2 == pytest.approx(float(np.sum(got[0] ** 2)), rel=1e-12)
        # a refused join leaves the resident one in place
        with pytest.raises(EngineError, match="17 bands"):
            eng.gauss_fit_join(band, P, njoin=17)
        np.testing.assert_array_equal(eng.gauss_residuals("000", nu_ref, *args, fetch=True, join=join), got)
    finally:
        eng.gauss_fit_end()
    with pytest.raises(EngineError, match="no fit is open"):
        eng.gauss_fit_join(band, P)


def _check_fit(name, fitted, fit_errs, chi2, dof, g):
    """tests/test_gpu_ppgauss.py's _check_fit."""
    want, sig = g["fitted_params"], g["fit_errs"]
    v = sig > 0
    dist = np.abs(fitted - want)[v] / sig[v]
    scatter = float(np.max(g["self_scatter"]))
    rel = np.abs(fit_errs[v] / sig[v] - 1.0)
    MEASURED[name] = dict(max_distance_sigma=float(dist.max()), self_scatter_sigma=scatter, bar_sigma=10 * scatter,
                          chi2_rel=float(chi2 / float(g["chi2"]) - 1.0), fit_errs_rel=float(rel.max()))
    print(name, "max distance %.2e sigma (self-scatter %.2e), chi2 rel %.1e, errs rel %.1e" %
          (dist.max(), scatter, chi2 / float(g["chi2"]) - 1.0, rel.max()))
    assert np.all(fitted[~v] == want[~v])
    assert np.all(fit_errs[~v] == 0.0)
    assert dist.max() <= 1e-3
    assert dist.max() <= 10 * scatter
    assert chi2 <= float(g["chi2"]) * (1 + 1e-9)
    assert rel.max() <= 1e-4
    assert dof == int(g["dof"])


@pytest.mark.parametrize("name", ["2x8x128", "3x6x100"])
def test_golden_joined_fits_through_the_engine(eng, name):
    from pulseportraiture_amd.pplib import fit_gaussian_portrait, get_bin_centers
    g = _g("ppgauss_join_fit_" + name)
    nchan, nbin = g["data"].shape
    with eng.profiled() as kt:
        r = fit_gaussian_portrait(str(g["code"]), g["data"], g["init_params"], float(g["scattering_index_in"]),
                                  np.outer(g["errs"], np.ones(nbin)), g["fit_flags"], False, get_bin_centers(nbin),
                                  g["freqs"], float(g["nu_ref"]),
                                  join_params=[join_ichans_of(g), g["join_init"], g["join_flags"]], P=float(g["P"]),
                                  engine=eng)
    # one iteration is one gauss_residuals plus one gauss_normal, plus one of each per trial step
    lm = r.lm_results
    assert kt["gauss_resid"][1] == lm.niter + lm.nfev + 1 and kt["gauss_normal"][1] == lm.niter + lm.nfev
    assert r.scattering_index == float(g["scattering_index"]) and r.scattering_index_err == 0.0
    assert len(r.fitted_params) == len(g["init_params"]) + len(g["join_init"])
    _check_fit("fit_" + name, r.fitted_params, r.fit_errs, r.chi2, r.dof, g)
    MEASURED["fit_" + name].update(jacobians=int(lm.niter), trial_steps=int(lm.nfev), message=lm.message)
    assert np.sum((r.residuals / g["errs"][:, None]) ** 2) == pytest.approx(r.chi2, rel=1e-12)


def _bunches(m):
    from pulseportraiture_amd.pptoas import data_from_arrays
    out = []
    for i in range(2):
        sub, freqs = m["band%d_subints" % i], m["band%d_freqs" % i]
        nchan = sub.shape[2]
        out.append(data_from_arrays(sub, freqs, m["Ps"], [55000.0], noise_stds=np.full((1, 1, nchan), float(m["noise_std"])),
                                    SNRs=m["band%d_SNRs" % i], bw=-abs(freqs[0, 0] - freqs[0, 1]) * nchan,
                                    source="PSR_1234-5678", filename="band%d.npz" % (i + 1)))
    return out


def test_make_gaussian_model_on_two_bands(eng, tmp_path):
    """The reference's DataPortrait(metafile) and make_gaussian_model(modelfile, niter=1) on the two-band case: the
    start the device's fit_phase_shift gives, every pass of check_convergence, the .join file and the final model.
    Measured on an MI355X: the pass's phase 3e-11 rot and DM 1.5e-10 from the reference's, the parameters 4.0e-5 sigma
    (the reference's two solves: 3.4e-5); the final model portrait 7.1e-7 and the data 1.3e-6 from the reference's, which
    is what parameters that far apart give -- recorded, not barred: the bars on them are against NumPy with the
    parameters fitted here."""
    from pulseportraiture_amd.ppgauss import DataPortrait
    m, g = _g("ppgauss_join_model"), _g("ppgauss_join_fit_2x8x128")
    start = tmp_path / "start.gmodel"
    start.write_bytes(m["start_gmodel"].tobytes())
    dp = DataPortrait(_bunches(m))
    dp.engine = eng
    dp.joinfile = str(tmp_path / "bands.join")          # (where the fitted parameters go)
    for i in range(2):
        np.testing.assert_array_equal(dp.join_ichanxs[i], m["join_ichanxs%d" % i])
    np.testing.assert_allclose(dp.join_params, m["join_params_init"], rtol=0, atol=PHI_BAR)
    dp.make_gaussian_model(modelfile=str(start), niter=1, writemodel=True, outfile=str(tmp_path / "out.gmodel"),
                           writeerrfile=True, quiet=True)
    assert abs(dp.nu_fit - float(m["nu_fit"])) < 1e-9
    want = m["passes"]
    got = np.array(dp.convergence_history, dtype=np.float64)
    print("passes\n", got, "\nreference\n", want)
    MEASURED["model_passes"] = dict(dphi=float(np.abs(got[:len(want), 0] - want[:len(got), 0]).max()),
                                    dDM=float(np.abs(got[:len(want), 2] - want[:len(got), 2]).max()))
    assert got.shape == want.shape
    for a, b in zip(got, want):
        assert abs((a[0] - b[0] + 0.5) % 1.0 - 0.5) < PHI_BAR and abs(a[2] - b[2]) < DM_BAR
        np.testing.assert_allclose([a[1], a[3], a[4]], [b[1], b[3], b[4]], rtol=1e-6)
        assert a[5] == b[5]
    # the join parameters and the model's: the fit bars against the reference's values and errors here (the same data
    # and objective as the fit golden from another start of the join parameters, whose self-scatter stands for both)
    full = np.concatenate([dp.model_params, dp.join_params])
    errs = np.concatenate([dp.model_param_errs, dp.join_param_errs])
    ref = dict(fitted_params=np.concatenate([m["model_params"], m["join_params"]]),
               fit_errs=np.concatenate([m["model_param_errs"], m["join_param_errs"]]), chi2=m["chi2"], dof=m["dof"],
               self_scatter=g["self_scatter"])
    _check_fit("model_2x8x128", full, errs, dp.chi2, dp.dof, ref)
    # the .join file: the reference's layout, its numbers within the same bars
    lines = open(str(tmp_path / "bands.join")).read().splitlines()
    ref_lines = m["join_text"].tobytes().decode().splitlines()
    assert len(lines) == len(ref_lines) * len(want) and lines[0] == ref_lines[0]
    sig = m["join_param_errs"]
    scatter = float(np.max(g["self_scatter"]))
    for ib, (mine, theirs) in enumerate(zip(lines[-2:], ref_lines[-2:])):
        a, b = mine.split(), theirs.split()
        assert a[0] == b[0] == "band%d.npz" % (ib + 1) and len(a) == len(b) == 5
        for col, s, half_ulp in ((1, sig[2 * ib], 0.5e-10), (3, sig[2 * ib + 1], 0.5e-6)):
            bar = min(1e-3, 10 * scatter) * s + 2 * half_ulp          # (both files round to the last printed digit)
            assert abs(float(a[col]) - float(b[col])) <= bar, (mine, theirs)
        for col in (2, 4):
            assert float(a[col]) == pytest.approx(float(b[col]), rel=1e-4, abs=2e-10 if col == 2 else 2e-6)
    # the final model: the written file holds the fitted parameters to its digits
    from pulseportraiture_amd import gmodel
    mdl = gmodel.read_gmodel(str(tmp_path / "out.gmodel"))
    assert mdl["ngauss"] == 3 and os.path.exists(str(tmp_path / "out.gmodel_errs"))
    np.testing.assert_allclose(mdl["params"], dp.model_params, rtol=0, atol=6e-9)
    # ... and model and data are left with the bands' offsets taken out again, as the reference leaves them: the model is
    # the joined portrait of the fitted parameters rotated back band by band (NOT the plain portrait: each rotation keeps
    # the real part of the Nyquist term only, and the second component is narrow enough at 128 bins to have one), the
    # data the input rotated by minus the join parameters -- against NumPy, at the unjoined rows test's 2e-14 of the
    # peak per transform (four of them)
    k = np.arange(65)

    def rotated_back(port):
        out = np.array(port)
        for ic, (phi, DM) in zip(dp.join_ichans, -dp.join_params.reshape(2, 2)):
            phis = phi + Dconst * DM / dp.Ps[0] * (dp.freqs[0, ic] ** -2.0 - dp.nu_ref ** -2.0)
            out[ic] = np.fft.irfft(np.fft.rfft(out[ic], axis=-1) * np.exp(2j * np.pi * np.outer(phis, k)), axis=-1)
        return out
    host = dict(params=dp.model_params, code=dp.model_code, nu_ref=dp.nu_ref, alpha=dp.scattering_index, ngauss=3)
    there = gmodel.gaussian_portrait(host, dp.freqs[0], 128, P=128.0, join_ichans=dp.join_ichans, join_params=dp.join_params,
                                     P_join=dp.Ps[0])
    want_model = rotated_back(there)
    np.testing.assert_allclose(dp.model, want_model, rtol=0, atol=8e-14 * np.abs(want_model).max())
    plain = gmodel.gaussian_portrait(host, dp.freqs[0], 128, P=128.0)
    assert np.abs(want_model - plain).max() > 1e-6 * np.abs(plain).max()          # (the Nyquist term is there)
    back = rotated_back(m["port_in"])
    np.testing.assert_allclose(dp.port, back, rtol=0, atol=8e-14 * np.abs(back).max())
    np.testing.assert_allclose(dp.portx, back, rtol=0, atol=8e-14 * np.abs(back).max())
    # the distance of both to the reference's (another solve of the same minimum) is recorded, not barred
    MEASURED["model_2x8x128"].update(model_max_abs=float(np.abs(dp.model - m["model"]).max()),
                                     port_max_abs=float(np.abs(dp.port - m["port_out"]).max()))


def test_command_line_round_trip_to_toas(tmp_path):
    """two band archives -> ppgauss_join_run -M -> .gmodel + .join -> pptoas_run on one of the bands: the joined route
    README describes."""
    from pulseportraiture_amd import gmodel
    m, g = _g("ppgauss_join_model"), _g("ppgauss_join_fit_2x8x128")
    for i in range(2):
        nchan = m["band%d_subints" % i].shape[2]
        np.savez(tmp_path / ("band%d.npz" % (i + 1)), subints=m["band%d_subints" % i], freqs=m["band%d_freqs" % i], Ps=m["Ps"],
                 epochs=np.array([55000.0]), noise_stds=np.full((1, 1, nchan), 0.05), bw=-400.0, source="PSR_1234-5678")
    (tmp_path / "bands.txt").write_text("band1.npz\nband2.npz\n")
    (tmp_path / "start.gmodel").write_bytes(m["start_gmodel"].tobytes())
    out = run_module("ppgauss_join_run", ["-M", "bands.txt", "-I", "start.gmodel", "-o", "out.gmodel", "-m", "joined_here"],
                     tmp_path, 300)
    assert "Fitting Gaussian model portrait..." in out
    mdl = gmodel.read_gmodel(str(tmp_path / "out.gmodel"))
    assert mdl["name"] == "joined_here" and mdl["ngauss"] == 3 and os.path.exists(str(tmp_path / "out.gmodel_errs"))
    # the model is the fit golden's, to the digits a .gmodel holds and the fit's bar
    v = g["fit_errs"][:len(mdl["params"])] > 0
    assert np.all(np.abs(mdl["params"] - g["fitted_params"][:len(mdl["params"])])[v] <= 1e-3 * g["fit_errs"][:len(mdl["params"])][v] + 6e-9)
    lines = (tmp_path / "joined_here.join").read_text().splitlines()
    assert len(lines) == 3 and lines[0].startswith("# archive name") and [ln.split()[0] for ln in lines[1:]] == ["band1.npz", "band2.npz"]
    assert float(lines[1].split()[1]) == 0.0 and abs(float(lines[2].split()[1]) - float(g["fitted_params"][-2])) < 1e-9
    toas = run_module("pptoas_run", ["-d", "band2.npz", "-m", "out.gmodel", "-o", "band2.tim"], tmp_path, 300)
    tim = (tmp_path / "band2.tim").read_text().splitlines()
    assert len([ln for ln in tim if "band2.npz" in ln]) == 1, (toas, tim)
