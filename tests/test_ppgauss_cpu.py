"""ppgauss on the host: the .gmodel writer, the bound transforms, the host restatement of the residuals, the
Levenberg-Marquardt driver on a NumPy evaluator against the reference's fits (tests/golden/make_golden_ppgauss.py),
the flag logic, the tau unit changes and the command line's parsing.  No GPU."""
import os

import numpy as np
import pytest

from pulseportraiture_amd import gaussfit, gmodel, ppgauss_run

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_write_gmodel_is_the_references_text(tmp_path):
    """DataPortrait.write_model / write_errfile of the reference on the 12 x 200 fit (one loc moved past 1): the same
    bytes through ppgauss.DataPortrait's two methods, and parse_gmodel reads them back."""
    from pulseportraiture_amd.ppgauss import DataPortrait
    g = _g("ppgauss_model_text")
    dp = DataPortrait.__new__(DataPortrait)
    dp.model_params, dp.model_param_errs = g["model_params"].copy(), g["model_param_errs"].copy()
    dp.Ps, dp.nbin, dp.model_name, dp.model_code = [float(g["P"])], int(g["nbin"]), "PSR_1234-5678", "000"
    dp.nu_ref, dp.fit_flags, dp.fitalpha, dp.datafile = float(g["nu_ref"]), g["fit_flags"], 0, "fake.npz"
    dp.scattering_index, dp.scattering_index_err = float(g["scattering_index"]), float(g["scattering_index_err"])
    dp.write_model(outfile=str(tmp_path / "m.gmodel"), quiet=True)
    dp.write_errfile(errfile=str(tmp_path / "m.gmodel_errs"), quiet=True)
    for mine, theirs in (("m.gmodel", "ppgauss_fit.gmodel"), ("m.gmodel_errs", "ppgauss_fit.gmodel_errs")):
        assert open(str(tmp_path / mine), "rb").read() == open(os.path.join(GOLDEN, theirs), "rb").read()
    np.testing.assert_array_equal(dp.model_params, g["model_params"])          # (the object's own parameters stay)
    mdl = gmodel.read_gmodel(str(tmp_path / "m.gmodel"))
    assert (mdl["name"], mdl["code"], mdl["ngauss"], mdl["fit_alpha"]) == ("PSR_1234-5678", "000", 3, 0)
    want = g["model_params"].copy()
    want[8] -= 1.0                                      # the loc % 1 tidy-up
    want[1] *= float(g["P"]) / int(g["nbin"])           # bins -> seconds
    np.testing.assert_allclose(mdl["params"], want, rtol=0, atol=5.1e-9)
    np.testing.assert_array_equal(mdl["fit_flags"], g["fit_flags"].astype(int))
    # append
    gmodel.write_gmodel(str(tmp_path / "m.gmodel"), "second", "011", 1500.0, want, g["fit_flags"], -4.0, 1, append=True, quiet=True)
    assert open(str(tmp_path / "m.gmodel")).read().count("MODEL") == 2


def test_tau_unit_changes(tmp_path):
    """bins <-> seconds: a model file's TAU [s] enters the fit in bins (ppgauss.py:110) and leaves in seconds (:351, :368)."""
    from pulseportraiture_amd.ppgauss import DataPortrait
    P, nbin = 0.004, 512
    dp = DataPortrait.__new__(DataPortrait)
    dp.Ps, dp.nbin, dp.model_name, dp.model_code, dp.nu_ref, dp.fitalpha = [P], nbin, "x", "000", 1400.0, 0
    dp.fit_flags = np.ones(8)
    dp.model_params = np.array([0.0, 3.2, 0.5, 0.0, 0.02, 0.0, 1.0, 0.0])           # tau = 3.2 bins
    dp.model_param_errs = np.array([0.0, 0.64, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    dp.scattering_index, dp.scattering_index_err = -4.0, 0.0
    dp.write_model(outfile=str(tmp_path / "t.gmodel"), quiet=True)
    dp.write_errfile(errfile=str(tmp_path / "t.gmodel_errs"), quiet=True)
    assert gmodel.read_gmodel(str(tmp_path / "t.gmodel"))["params"][1] == pytest.approx(3.2 * P / nbin, abs=5.1e-9)
    assert gmodel.read_gmodel(str(tmp_path / "t.gmodel_errs"))["params"][1] == pytest.approx(0.64 * P / nbin, abs=5.1e-9)
    assert gmodel.read_gmodel(str(tmp_path / "t.gmodel_errs"))["name"] == "x_errors"


@pytest.mark.parametrize("lo,hi", [(-np.inf, np.inf), (0.0, np.inf), (0.0, 0.25), (-np.inf, 2.0)])
def test_bound_transforms_round_trip(lo, hi):
    for x in (0.013, 0.2, 0.2499):
        p = gaussfit.to_internal(x, lo, hi)
        assert gaussfit.to_external(p, lo, hi) == pytest.approx(x, rel=1e-13)
        eps = 1e-6
        num = (gaussfit.to_external(p + eps, lo, hi) - gaussfit.to_external(p - eps, lo, hi)) / (2 * eps)
        assert gaussfit.d_external(p, lo, hi) == pytest.approx(num, rel=1e-7)
    for p in (-30.0, -1.0, 0.0, 2.5, 1e3):          # every internal value lands inside the bounds
        assert lo <= gaussfit.to_external(p, lo, hi) <= hi


def test_covariance_is_carried_back_to_the_external_parameters():
    """A linear model y = a t + b with a >= 0 and 0 <= b <= 0.25: the driver's errors are those of linear least
    squares (covariance times chi2 / dof), whatever the internal parameters are; a fixed parameter has error 0."""
    rng = np.random.default_rng(3)
    t = np.linspace(0, 1, 50)
    y = 0.7 * t + 0.1 + 0.01 * rng.standard_normal(50)
    sigma = 0.02

    def evaluate(sets, h):
        R = np.array([(y - (s[0] * t + s[1] + s[2])) / sigma for s in np.atleast_2d(sets)])
        return gaussfit.normal_equations(R, h)
    r = gaussfit.levenberg_marquardt(evaluate, [0.5, 0.2, 0.0], [True, True, False], [0.0, 0.0, -np.inf], [np.inf, 0.25, np.inf], 50)
    A = np.stack([t, np.ones(50)], axis=1) / sigma
    x, res = np.linalg.lstsq(A, y / sigma, rcond=None)[:2]
    cov = np.linalg.inv(A.T @ A) * (res[0] / 48)
    np.testing.assert_allclose(r.x[:2], x, rtol=1e-7)
    np.testing.assert_allclose(r.stderr[:2], np.sqrt(np.diag(cov)), rtol=1e-5)
    assert r.stderr[2] == 0.0 and r.x[2] == 0.0 and r.dof == 48
    assert r.chi2 == pytest.approx(res[0], rel=1e-10)
    with pytest.raises(ValueError, match="outside its bounds"):
        gaussfit.levenberg_marquardt(evaluate, [0.5, 0.3, 0.0], [True, True, False], [0.0, 0.0, -np.inf], [np.inf, 0.25, np.inf], 50)


def test_portrait_bounds():
    lo, hi = gaussfit.portrait_bounds(2 + 12 + 1)
    assert list(lo) == [-np.inf, 0.0, -np.inf, -np.inf, 0.0, -np.inf, 0.0, -np.inf, -np.inf, -np.inf, 0.0, -np.inf, 0.0,
                        -np.inf, -np.inf]
    assert [i for i in range(15) if np.isfinite(hi[i])] == [4, 10] and hi[4] == 0.25


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_host_residuals_against_the_reference(nbin, code, scattered):
    """gaussfit.host_residuals (on gmodel.gaussian_portrait) against fit_gaussian_portrait_function's rows, within the
    bar tests/test_host_cpu.py holds gaussian_portrait to (rtol 1e-13, atol 1e-14 on the model), over sigma_n."""
    g = _g("ppgauss_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    data, errs, freqs = g["n%d_data" % nbin], g["n%d_errs" % nbin], g["n%d_freqs" % nbin]
    with np.errstate(invalid="ignore"):
        got = gaussfit.host_residuals(g[tag + "_sets"], data, errs, code, freqs, float(g["nu_ref"])).reshape(9, 3, nbin)
    want = g[tag + "_rows"].reshape(9, 3, nbin)
    model = data[None] - want * errs[None, :, None]
    bar = (1e-14 + 1e-13 * np.abs(model)) / errs[None, :, None] + np.spacing(np.abs(want))
    assert np.all(np.abs(got - want) <= bar), float((np.abs(got - want) / bar).max())


def test_normal_equations_are_the_definition():
    rng = np.random.default_rng(5)
    R, h = rng.standard_normal((4, 30)), np.array([1e-3, 2e-3, 5e-4])
    chi2, g, G = gaussfit.normal_equations(R, h)
    D = (R[1:] - R[0]) / h[:, None]
    assert chi2 == pytest.approx(np.sum(R[0] ** 2)) and np.allclose(g, D @ R[0]) and np.allclose(G, D @ D.T)
    chi2, g, G = gaussfit.normal_equations(R[:1], np.zeros(0))
    assert g.shape == (0,) and G.shape == (0, 0)


@pytest.mark.parametrize("name", ["16x256", "12x200"])
def test_driver_reaches_the_golden_fits(name):
    """The LM driver on the NumPy evaluator: every parameter within 1e-3 of its golden 1 sigma (a thousandth of the
    statistical error; the reference's own two solves differ by 20 times less), chi2 <= golden chi2 (1 + 1e-9),
    fit_errs within 1e-4."""
    g = _g("ppgauss_fit_" + name)
    nchan, nbin = g["data"].shape
    code, nu_ref = str(g["code"]), float(g["nu_ref"])
    r = gaussfit.fit_gaussian_portrait(code, g["data"], g["init_params"], float(g["scattering_index_in"]), g["errs"],
                                       g["fit_flags"], False, np.arange(nbin), g["freqs"], nu_ref,
                                       evaluator=gaussfit.numpy_evaluator(g["data"], g["errs"], code, g["freqs"], nu_ref))
    v = g["fit_errs"] > 0
    assert np.array_equal(v, g["fit_flags"] != 0)
    dist = np.abs(r.fitted_params - g["fitted_params"])[v] / g["fit_errs"][v]
    print(name, "max distance %.2e sigma, self-scatter %.2e" % (dist.max(), g["self_scatter"].max()))
    assert dist.max() <= 1e-3
    assert np.all(r.fitted_params[~v] == g["init_params"][~v]) and np.all(r.fit_errs[~v] == 0.0)
    assert r.chi2 <= float(g["chi2"]) * (1 + 1e-9)
    assert np.abs(r.fit_errs[v] / g["fit_errs"][v] - 1.0).max() <= 1e-4
    assert r.dof == int(g["dof"]) == nchan * nbin - int(v.sum())
    assert r.scattering_index == float(g["scattering_index"]) and r.scattering_index_err == 0.0
    assert r.residuals.shape == (nchan, nbin) and np.sum((r.residuals / g["errs"][:, None]) ** 2) == pytest.approx(r.chi2, rel=1e-12)


def test_profile_fit_is_the_portrait_path():
    g = _g("ppgauss_profile")
    n = len(g["profile"])
    r = gaussfit.fit_gaussian_profile(g["profile"], g["init_params"], np.zeros(n) + float(g["noise"]),
                                      evaluator_factory=gaussfit.numpy_evaluator)
    v = g["fit_errs"] > 0
    assert list(v) == [True, False, True, True, True]
    assert (np.abs(r.fitted_params - g["fitted_params"])[v] / g["fit_errs"][v]).max() <= 1e-3
    assert r.chi2 <= float(g["chi2"]) * (1 + 1e-9) and r.dof == int(g["dof"])
    assert np.abs(r.fit_errs[v] / g["fit_errs"][v] - 1.0).max() <= 1e-4 and r.fit_errs[1] == 0.0
    # residuals = data - model at the fitted parameters (pplib.py:1906-1908); chi2 is their weighted square sum
    assert np.sum((r.residuals / float(g["noise"])) ** 2) == pytest.approx(r.chi2, rel=1e-12)
    assert np.sum((g["residuals"] / float(g["noise"])) ** 2) == pytest.approx(float(g["chi2"]), rel=1e-12)
    # flags in the reference's order: [DC, (loc, wid, amp) ...] beside fit_scattering
    r2 = gaussfit.fit_gaussian_profile(g["profile"], g["init_params"], float(g["noise"]), fit_flags=[0, 1, 0, 1],
                                       evaluator_factory=gaussfit.numpy_evaluator)
    assert list(r2.fit_errs > 0) == [False, False, True, False, True]
    assert r2.fitted_params[0] == g["init_params"][0] and r2.fitted_params[3] == g["init_params"][3]


def test_joined_fits_and_bad_shapes_are_refused():
    g = _g("ppgauss_fit_12x200")
    args = [str(g["code"]), g["data"], g["init_params"], -4.0, g["errs"], g["fit_flags"], False, np.arange(200), g["freqs"], 1300.0]
    with pytest.raises(NotImplementedError, match="join"):
        gaussfit.fit_gaussian_portrait(*args, join_params=[[[0, 1]], [0.0, 0.0], [1, 1]])
    with pytest.raises(ValueError, match="constant along"):
        gaussfit.fit_gaussian_portrait(*args[:4], np.random.default_rng(0).uniform(1, 2, g["data"].shape), *args[5:],
                                       evaluator=lambda s, h: None)
    with pytest.raises(ValueError, match="2 \\+ 6 ngauss"):
        gaussfit.fit_gaussian_portrait(args[0], args[1], g["init_params"][:-1], *args[3:], evaluator=lambda s, h: None)


def test_flag_logic_of_make_gaussian_model():
    from pulseportraiture_amd.ppgauss import portrait_start
    prof = [0.01, 0.4, 0.2, 0.05, 5.0, 0.3, 0.02, 2.0]
    p, f = portrait_start(prof)
    assert list(p) == [0.01, 0.4, 0.2, 0.0, 0.05, 0.0, 5.0, 0.0, 0.3, 0.0, 0.02, 0.0, 2.0, 0.0]
    assert list(f) == [1, 0] + [1] * 12                             # fixscat is the default
    assert list(portrait_start(prof, fixscat=False)[1]) == [1] * 14
    assert list(portrait_start(prof, fixloc=True)[1][3::6]) == [0, 0]
    assert list(portrait_start(prof, fixwid=True)[1][5::6]) == [0, 0]
    assert list(portrait_start(prof, fixamp=True)[1][7::6]) == [0, 0]
    f = portrait_start(prof, fixloc=True, fixwid=True, fixamp=True)[1]
    assert list(f) == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    # a fiducial Gaussian: every location drifts but the first component's, whatever fixloc says
    for fixloc in (False, True):
        assert list(portrait_start(prof, fixloc=fixloc, fiducial_gaussian=True)[1][3::6]) == [0, 1]


def _opts(*argv):
    return ppgauss_run.parser().parse_args(list(argv))


def test_command_line_parsing_and_refusals(capsys):
    o = _opts("-d", "a.npz", "--autogauss", "0.05")
    assert (o.fixloc, o.fixwid, o.fixamp, o.fixscat, o.fixalpha, o.fgauss, o.quiet) == (True, False, False, True, True, False, True)
    assert o.model_code == "000" and int(o.niter) == 0 and float(o.tau) == 0.0 and o.normalize is None
    assert ppgauss_run.refusal(o) is None and ppgauss_run.refusal(o, ["a.npz"]) is None
    o = _opts("-d", "a.npz", "-I", "m.gmodel", "-o", "o.gmodel", "-e", "o.errs", "-m", "name", "--nu_ref", "1400", "--bw", "200",
              "--tau", "1e-5", "--fitloc", "--fixwid", "--fixamp", "--fitscat", "--fitalpha", "--mcode", "011", "--niter", "3",
              "--fgauss", "--norm", "prof", "--verbose")
    assert (o.modelfile, o.outfile, o.errfile, o.model_name, o.nu_ref, o.bw_ref) == ("m.gmodel", "o.gmodel", "o.errs", "name", "1400", "200")
    assert (o.fixloc, o.fixwid, o.fixamp, o.fixscat, o.fixalpha, o.fgauss, o.quiet) == (False, True, True, False, False, True, False)
    assert (o.model_code, o.niter, o.normalize) == ("011", "3", "prof") and ppgauss_run.refusal(o) is None
    o = _opts("-d", "a.npz", "--gauss", "0.2,0.05,3", "--gauss", "0.3,0.02,1.5")
    assert ppgauss_run.parse_gauss(o.gauss) == [(0.2, 0.05, 3.0), (0.3, 0.02, 1.5)] and ppgauss_run.refusal(o) is None
    for argv, word in ((["-M", "meta.txt", "--autogauss", "0.05"], "-M/--metafile"),
                       (["-d", "a.npz", "-j", "join.txt", "--autogauss", "0.05"], "-j/--joinfile"),
                       (["-d", "a.npz", "--figure", "f.png", "--autogauss", "0.05"], "--figure"),
                       (["--autogauss", "0.05"], "-d"),
                       (["-d", "a.npz", "--autogauss", "0.05", "--norm", "median"], "Unknown normalization"),
                       (["-d", "a.npz", "--gauss", "0.2,0.05"], "three numbers"),
                       (["-d", "a.npz", "--gauss", "a,b,c"], "three numbers")):
        msg = ppgauss_run.refusal(_opts(*argv))
        assert msg is not None and word in msg, (argv, msg)
    # none of -I, --autogauss, --gauss: the message names all three
    msg = ppgauss_run.refusal(_opts("-d", "a.npz"))
    assert all(w in msg for w in ("-I", "--autogauss", "--gauss"))
    assert "2 archives" in ppgauss_run.refusal(_opts("-d", "meta.txt", "--autogauss", "0.05"), ["a.npz", "b.npz"])
    # main() prints the message and returns 2 before anything touches a device
    assert ppgauss_run.main(["-d", "a.npz"]) == 2
    assert "ppgauss_run: no initial components" in capsys.readouterr().err


def test_pplib_keeps_the_reference_signatures():
    import inspect
    from pulseportraiture_amd import pplib
    assert list(inspect.signature(pplib.fit_gaussian_portrait).parameters)[:13] == [
        "model_code", "data", "init_params", "scattering_index", "errs", "fit_flags", "fit_scattering_index", "phases",
        "freqs", "nu_ref", "join_params", "P", "quiet"]
    assert list(inspect.signature(pplib.fit_gaussian_profile).parameters)[:6] == [
        "data", "init_params", "errs", "fit_flags", "fit_scattering", "quiet"]
    from pulseportraiture_amd.ppgauss import DataPortrait
    assert list(inspect.signature(DataPortrait.make_gaussian_model).parameters)[1:23] == [
        "modelfile", "ref_prof", "tau", "fixloc", "fixwid", "fixamp", "fixscat", "fixalpha", "scattering_index", "model_code",
        "niter", "fiducial_gaussian", "auto_gauss", "writemodel", "outfile", "writeerrfile", "errfile", "model_name",
        "residplot", "quiet", "init_gauss"][:22]
