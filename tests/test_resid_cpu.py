"""No GPU: the references of the fit's residual portrait (tests/resid_refs.py) against the reference's own show_fit
(tests/golden/showfit.npz, made by tests/golden/make_golden_showfit.py) and against rot_refs' rotate_ld / scatter_ld
composed in long double; ppresid_run's option table; the C declaration of pp_fit_residuals against the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import pptoas_oracle as orc
from tests import resid_refs as rf
from tests import rot_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble


def golden_case(g, name):
    """What the references need for the subint show_fit was asked for, rebuilt from the stored results as show_fit
    rebuilds it (pptoas.py:1352-1402): Doppler factors undone, 10**tau, the unscattered template at Ps.mean()."""
    v = lambda k: g["%s_%s" % (name, k)]        # noqa: E731
    isub = int(v("isub"))
    df = v("out_doppler_fs")[isub] if int(v("bary")) else 1.0
    phi, DM, GM = v("out_phis")[isub], v("out_DMs")[isub] / df, v("out_GMs")[isub] / df ** 3
    tau, alpha = v("out_taus")[isub], v("out_alphas")[isub]
    if tau != 0.0 and int(v("log10_tau")):
        tau = 10.0 ** tau
    nu_DM, nu_GM, nu_tau = v("out_nu_refs")[isub]
    freqs, P = v("freqs")[isub], v("Ps")[isub]
    data = v("subints")[isub, 0]
    nbin = data.shape[-1]
    _, code, nu_ref, _, params, _, malpha, _ = orc.parse_gmodel(open(os.path.join(GOLDEN, "example.gmodel")).read())
    params = params.copy()
    params[1] = 0.0 if tau != 0.0 else params[1] * nbin / v("Ps").mean()
    model = orc.gen_gaussian_portrait(code, params, malpha, orc.get_bin_centers(nbin), freqs, nu_ref)
    phin = np.array([float(rr.delay_ld(phi, DM, GM, nu, nu_DM, nu_GM, P)) for nu in freqs])
    taun = np.zeros(len(freqs)) if tau == 0.0 else tau * (freqs / nu_tau) ** alpha
    return dict(data=data, model=model, phin=phin, taun=taun, scales=v("out_scales")[isub], mask=v("weights")[isub] > 0,
                rotate=float(v("rotate")), port=v("fit_port"), model_scaled=v("fit_model_scaled"))


def turned(rows, rotate):
    """rotate_data(rows, rotate): both of show_fit's outputs are turned by `rotate`."""
    if not rotate:
        return rows
    k = np.arange(rows.shape[-1] // 2 + 1)
    return np.fft.irfft(np.fft.rfft(rows, axis=-1) * np.exp(2j * np.pi * k * rotate), rows.shape[-1], axis=-1)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "showfit.npz"))


def test_golden_holds_the_cases_asked_for(golden):
    shapes = {n: golden[n + "_fit_port"].shape for n in golden["names"]}
    assert shapes == {"zap": (8, 64), "gm": (6, 100), "scat": (8, 128), "rot": (8, 64)}
    assert int((golden["zap_weights"][0] == 0).sum()) == 2 and len(golden["zap_fit_ok_ichans"]) == 6
    assert golden["gm_out_GMs"][0] != 0 and int(golden["gm_kw_fit_GM"]) == 1
    assert golden["scat_out_taus"][0] != 0 and int(golden["scat_log10_tau"]) == 1 and golden["scat_out_alphas"][0] != 0
    assert float(golden["rot_rotate"]) == 0.1
    assert os.path.getsize(os.path.join(GOLDEN, "showfit.npz")) < 200e3


@pytest.mark.parametrize("name", ["zap", "gm", "scat", "rot"])
def test_restatement_reproduces_the_references_show_fit(golden, name):
    """Frame "model" of resid_refs.rows_f64 is show_fit's (port, model_scaled) to 1e-12 of each row's maximum."""
    c = golden_case(golden, name)
    nchan = len(c["data"])
    rows = [rf.rows_f64(c["data"][n], c["model"][n], c["phin"][n], c["taun"][n], c["scales"][n], "model") for n in range(nchan)]
    port = turned(np.stack([r["port"] for r in rows]), c["rotate"]) * c["mask"][:, None]
    model = turned(np.stack([r["model"] for r in rows]), c["rotate"])
    for got, want, what in ((port, c["port"], "port"), (model, c["model_scaled"], "model_scaled")):
        top = np.abs(want).max(axis=-1)
        dev = np.abs(got - want).max(axis=-1)
        print(name, what, "worst row: %.2e of its maximum" % float((dev[top > 0] / top[top > 0]).max()))
        assert np.all(dev <= 1e-12 * top), (name, what)
    assert not port[~c["mask"]].any() and not c["port"][~c["mask"]].any()


@pytest.mark.parametrize("frame", rf.FRAMES)
@pytest.mark.parametrize("name", ["zap", "gm", "scat"])
def test_restatement_agrees_with_rotation_and_scattering_composed_in_long_double(golden, name, frame):
    """rows_f64 and rows_ld (one pass through the harmonics) against rotate_ld / scatter_ld applied one after the other,
    on the golden's rows: 1e-12 of the row's maximum for f64, 1e-17 for long double; resid is port - model.  In the
    data's frame the two differ by design in the Nyquist term alone -- two transforms in a row each keep a real part,
    Re(B_M m_M) cos, where the one pass keeps Re(B_M m_M e^{-i theta}) --, so there every row is compared without its
    alternating component."""
    c = golden_case(golden, name)

    def no_nyquist(rows):
        if frame == "model":
            return rows
        out = {}
        for w, r in rows.items():
            alt = np.where(np.arange(len(r)) % 2 == 0, 1, -1).astype(r.dtype)
            out[w] = r - alt * (np.sum(r * alt) / len(r))
        return out
    for n in range(len(c["data"])):
        args = (c["data"][n], c["model"][n], c["phin"][n], c["taun"][n], c["scales"][n], frame)
        comp, ld, f64 = (no_nyquist(r) for r in (rf.rows_composed_ld(*args), rf.rows_ld(*args), rf.rows_f64(*args)))
        scale = float(np.abs(c["data"][n]).max() + abs(c["scales"][n]) * np.abs(c["model"][n]).max())
        for w in ("port", "model"):
            assert float(np.abs(ld[w] - comp[w]).max()) <= 1e-17 * scale, (n, w)
            assert float(np.abs(f64[w] - comp[w]).max()) <= 1e-12 * scale, (n, w)
        assert float(np.abs(f64["resid"] - (comp["port"] - comp["model"])).max()) <= 1e-12 * scale
        assert float(np.abs(ld["resid"] - (comp["port"] - comp["model"])).max()) <= 1e-17 * scale


def test_frames_are_one_residual_turned(golden):
    """The data frame's residual is the model frame's rotated back by phi_n, but for the Nyquist term, which each
    frame's irfft makes real in its own frame: the rows agree once their alternating component is taken out."""
    c = golden_case(golden, "scat")
    for n in range(len(c["data"])):
        args = (c["data"][n], c["model"][n], c["phin"][n], c["taun"][n], c["scales"][n])
        rm, rd = rf.rows_ld(*args, "model")["resid"], rf.rows_ld(*args, "data")["resid"]
        back = rr.rotate_ld(rm, -c["phin"][n])
        alt = np.where(np.arange(len(rm)) % 2 == 0, 1, -1).astype(LD)
        diff = back - rd
        diff = diff - alt * (np.sum(diff * alt) / len(diff))
        assert float(np.abs(diff).max()) <= 1e-16 * float(np.abs(c["data"][n]).max())


# ---- ppresid_run's option table ----------------------------------------------------------------------------
def _opts(*args):
    from pulseportraiture_amd import ppresid_run as run
    return run.parser().parse_args(["-d", "a.npz", "-m", "m.gmodel"] + list(args))


def test_ppresid_run_defaults():
    from pulseportraiture_amd import ppresid_run as run
    o = _opts()
    assert (o.ext, o.frame, o.metafile, o.quiet, o.noise_method) == ("resid.npz", "data", None, False, None)
    assert run.refusal(o) is None
    kw = run.get_toas_kwargs(o)
    assert kw == dict(nu_refs=None, DM0=None, bary=True, fit_DM=True, fit_GM=False, fit_scat=False, log10_tau=True,
                      scat_guess=None, fix_alpha=False, method='trust-ncg', quiet=False, seed="reference")


def test_ppresid_run_fit_options_reach_get_TOAs():
    from pulseportraiture_amd import ppresid_run as run
    o = _opts("--DM", "12.5", "--no_bary", "--fix_DM", "--fit_dt4", "--fit_scat", "--no_log10_tau", "--scat_guess",
              "1e-5,1400,-4.4", "--fix_alpha", "--nu_ref", "1500", "--noise_method", "fit", "--seed", "device", "-e", "r.npz",
              "--metafile", "out.txt", "--frame", "model", "--quiet")
    assert run.refusal(o) is None
    kw = run.get_toas_kwargs(o)
    assert kw == dict(nu_refs=(1500.0, None), DM0=12.5, bary=False, fit_DM=False, fit_GM=True, fit_scat=True,
                      log10_tau=False, scat_guess=[1e-5, 1400.0, -4.4], fix_alpha=True, method='trust-ncg', quiet=True,
                      seed="device")
    assert (o.ext, o.metafile, o.frame, o.noise_method) == ("r.npz", "out.txt", "model", "fit")
    assert run.get_toas_kwargs(_opts("--nu_ref", "inf"))["nu_refs"] == (np.inf, None)
    # every keyword is one get_TOAs takes
    import inspect
    from pulseportraiture_amd.pptoas import GetTOAs
    assert set(kw) <= set(inspect.signature(GetTOAs.get_TOAs).parameters)


@pytest.mark.parametrize("args, word", [(("--psrchive",), "PSRCHIVE"), (("-T",), "PSRCHIVE"), (("--showplot",), "plots"),
                                        (("--saveplot",), "plots"), (("--noise_method", "rms"), "unknown estimator")])
def test_ppresid_run_refusals(args, word, capsys):
    from pulseportraiture_amd import ppresid_run as run
    assert word in run.refusal(_opts(*args))
    assert run.main(["-d", "a.npz", "-m", "m.gmodel"] + list(args)) == 2
    assert "ppresid_run: " in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _opts("--frame", "sky")


def test_ppresid_run_summary():
    """The printed figures from a residual bunch: sigma 0 and unfitted rows are left out."""
    from pulseportraiture_amd import ppresid_run as run
    from pulseportraiture_amd.pplib import DataBunch
    resid = np.zeros((2, 3, 10))
    resid[0, 1, 7] = -4.0
    resid[0, 2, 3] = 100.0
    noise = np.array([[1.0, 2.0, 0.0], [np.nan] * 3])
    rc2 = np.array([[0.5, 1.5, np.inf], [np.nan] * 3])
    nfit, red, dof, worst, where = run.summary(DataBunch(resid=resid, noise_stds=noise, channel_red_chi2=rc2, ok_isubs=[0]), 10)
    assert (nfit, dof, where) == (1, 16, (0, 1, 7)) and red == pytest.approx(1.0) and worst == pytest.approx(2.0)


# ---- the C ABI ----------------------------------------------------------------------------------------------
def test_c_declaration_binding_and_header_agree():
    from pulseportraiture_amd import _lib
    header = open(os.path.join(ROOT, "include", "pp_toas.h")).read()
    m = re.search(r"int pp_fit_residuals\(([^;]*)\);", header)
    assert m, "pp_fit_residuals is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    want = ["pp_ctx* ctx", "const void* src", "int dtype", "int on_device", "int nsub", "int nchan", "int nbin",
            "const int32_t* model_slot", "const double* freqs", "int64_t freqs_stride", "const double* P",
            "const double* params5", "const double* nu_refs3", "const double* scales", "const double* errs",
            "const double* mask", "int frame", "void* port", "void* model", "void* resid", "double* red_chi2"]
    assert params == want
    source = open(os.path.join(ROOT, "pulseportraiture_amd", "csrc", "pp_resid.h")).read()
    d = re.search(r'extern "C" int pp_fit_residuals\(([^)]*)\)', source)
    types = lambda ps: [" ".join(p.split()).rsplit(" ", 1)[0] for p in ps]        # noqa: E731
    assert types(d.group(1).split(",")) == types(want)
    kinds = {"pp_ctx*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
             "const int32_t*": _lib.c_int32_p, "const double*": _lib.c_double_p,
             "double*": C.c_void_p}        # (red_chi2 is a device pointer for device input: passed as an address)
    res, args = _lib.SYMBOLS["pp_fit_residuals"]
    assert res is C.c_int and args == [kinds[t] for t in types(want)]
    assert re.search(r"#define PP_ABI_VERSION\s+11\b", header) and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert hasattr(lib, "pp_fit_residuals")
    # no GPU, or bad arguments: an error code and a message, never a crash
    assert lib.pp_fit_residuals(None, None, 0, 0, 1, 1, 64, None, None, 0, None, None, None, None, None, None, 0, None,
                                None, None, None) != 0
    assert "pp_fit_residuals" in _lib.last_error()
