"""CPU-side checks of the narrowband scattering fit: the NumPy restatement the GPU tests
compare with reproduces the true reference's objective, the new entry point is exported
with its documented prototype and refuses bad arguments, and the caller's guess recipe,
TOA flags and command-line mapping are what the issue states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nbscat_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fits():
    return np.load(os.path.join(GOLDEN, "nbscat_fits.npz"))


def cases(g):
    """(index, prof, mprof, sigma, guess, log10_tau) of every stored problem."""
    seen = {}
    for i in range(len(g["nbin"])):
        nb = int(g["nbin"][i])
        j = seen.get(nb, 0)
        seen[nb] = j + 1
        yield i, g["prof_%d" % nb][j], g["mprof_%d" % nb][j], float(g["sigma"][i]), float(g["guess"][i]), \
            bool(g["log10_tau"][i])


def test_restatement_reproduces_the_reference_objective(fits):
    """f, grad f and Hess f of tests/nbscat_ref.py at the three stored points of all 24 cases against the true
    reference's fit_portrait_full_function / _deriv / _2deriv: <= 1e-12 relative (to the largest entry of each)."""
    n = 0
    for i, prof, mprof, sigma, guess, l10 in cases(fits):
        X, p, Sd = nr.spectra(prof, mprof, sigma)
        for q in range(3):
            f, g, h = nr.fgh(X, p, fits["pts"][i, q], l10)
            assert abs(f - fits["f"][i, q]) <= 1e-12 * abs(fits["f"][i, q]), (i, q)
            assert np.abs(g - fits["g"][i, q]).max() <= 1e-12 * np.abs(fits["g"][i, q]).max(), (i, q)
            assert np.abs(h - fits["h"][i, q]).max() <= 1e-12 * np.abs(fits["h"][i, q]).max(), (i, q)
            n += 1
    assert n == 72


def test_restatement_fit_sits_inside_the_reference_spread(fits):
    """The restatement's own fit (SciPy to a tight gradient, then Newton on the gradient) of three stored cases
    agrees with the true reference's trust-ncg answer within the spread of the reference's variants."""
    out = fits["out"]
    for i, prof, mprof, sigma, guess, l10 in cases(fits):
        if i not in (1, 9, 22):
            continue
        r = nr.fit(prof, mprof, sigma, guess, None, l10)
        spread = np.abs(out[i, 1:, :9] - out[i, 0, :9]).max(axis=0)
        assert abs(r[0] - out[i, 0, 0]) <= 4 * max(spread[0], 1e-13), i
        assert abs(r[2] - out[i, 0, 2]) <= 4 * max(spread[2], 1e-13), i
        np.testing.assert_allclose(r[[1, 3, 4, 5, 6, 7, 8]], out[i, 0, [1, 3, 4, 5, 6, 7, 8]], rtol=1e-5)


def test_entry_point_is_exported_with_its_prototype():
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 11 and lib.pp_abi_version() == 11
    header = open(os.path.join(ROOT, "include", "pp_toas.h")).read()
    m = re.search(r"int pp_fit_phase_tau_batch\(([^;]*)\);", header)
    assert m, "pp_fit_phase_tau_batch is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["pp_ctx* ctx", "const double* data", "const double* model", "const double* noise",
                    "const double* guess", "int nprof", "int nbin", "double lo", "double hi", "int Ns",
                    "int log10_tau", "double* out"]
    assert "#define PP_NBS_NOUT 11" in header
    restype, argtypes = _lib.SYMBOLS["pp_fit_phase_tau_batch"]
    dp = _lib.c_double_p
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, dp, dp, dp, dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, dp]


def test_entry_point_refuses_null_arguments_before_any_device_work():
    """Without a context (no GPU needed) the call returns PP_EINVAL and names itself in the error string."""
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, _lib.c_double_p)
    assert lib.pp_fit_phase_tau_batch(None, p, p, None, p, 1, 16, -0.5, 0.5, 100, 1, p) == -1
    assert "pp_fit_phase_tau_batch" in _lib.last_error()


def test_guess_recipe():
    from pulseportraiture_amd.pptoas import narrowband_tau_guesses
    from pulseportraiture_amd.pplib import scattering_alpha
    freqs, P, nbin = np.array([1200.0, 1500.0, 1800.0]), 0.003, 256
    # scat_guess = (tau [s], nu_ref, alpha) wins over the model's values
    lin = narrowband_tau_guesses(freqs, P, nbin, False, scat_guess=(30e-6, 1500.0, -4.0), model_tau=1e-3,
                                 model_nu_ref=1300.0, alpha=-2.0)
    np.testing.assert_allclose(lin, (30e-6 / P) * (freqs / 1500.0) ** -4.0, rtol=1e-15)
    np.testing.assert_allclose(narrowband_tau_guesses(freqs, P, nbin, True, scat_guess=(30e-6, 1500.0, -4.0)),
                               np.log10(lin), rtol=1e-15)
    # the Gaussian model's tau scaled from its FREQ with its alpha, or the default index
    np.testing.assert_allclose(narrowband_tau_guesses(freqs, P, nbin, False, model_tau=2e-5, model_nu_ref=1300.0,
                                                      alpha=-3.5), (2e-5 / P) * (freqs / 1300.0) ** -3.5, rtol=1e-15)
    np.testing.assert_allclose(narrowband_tau_guesses(freqs, P, nbin, False, model_tau=2e-5, model_nu_ref=1300.0),
                               (2e-5 / P) * (freqs / 1300.0) ** scattering_alpha, rtol=1e-15)
    # nothing known: 0, which log10_tau turns into 1 / nbin
    assert not narrowband_tau_guesses(freqs, P, nbin, False).any()
    np.testing.assert_array_equal(narrowband_tau_guesses(freqs, P, nbin, True), np.log10(np.full(3, 1.0 / nbin)))
    np.testing.assert_array_equal(narrowband_tau_guesses(freqs, P, nbin, True, model_tau=0.0, model_nu_ref=1300.0,
                                                         alpha=-4.0), np.log10(np.full(3, 1.0 / nbin)))
    # the same recipe as the restatement the goldens were made with
    np.testing.assert_array_equal(narrowband_tau_guesses(freqs, P, nbin, True, scat_guess=(45e-6, 1500.0, -4.0)),
                                  nr.tau_guesses((45e-6, 1500.0, -4.0), None, None, None, -4.0, freqs, P, nbin, True))


def test_scattering_toa_flags():
    from pulseportraiture_amd.pptoas import narrowband_scat_flags
    P, df = 0.003, 1.0002
    f = narrowband_scat_flags(-2.0, 0.01, -3e-7, P, df, True)
    assert sorted(f) == ["log10_scat_time", "log10_scat_time_err", "phi_tau_cov", "scat_time"]
    assert f["scat_time"] == 10 ** -2.0 * P / df * 1e6 and f["log10_scat_time"] == -2.0 + np.log10(P / df)
    assert f["log10_scat_time_err"] == 0.01 and f["phi_tau_cov"] == -3e-7
    f = narrowband_scat_flags(0.01, 2e-4, -3e-9, P, df, False)
    assert sorted(f) == ["phi_tau_cov", "scat_time", "scat_time_err"]
    assert f["scat_time"] == 0.01 * P / df * 1e6 and f["scat_time_err"] == 2e-4 * P / df * 1e6
    assert f["phi_tau_cov"] == -3e-9


def test_command_line_maps_to_narrowband_keywords():
    from pulseportraiture_amd import pptoas_run
    opts = pptoas_run.parser().parse_args(["-d", "a.npz", "-m", "m.gmodel", "--narrowband", "--fit_scat",
                                           "--no_log10_tau", "--scat_guess", "3e-5,1500,-4.0", "--quiet"])
    assert opts.narrowband and pptoas_run.refusal(opts) is None
    kw = pptoas_run.get_narrowband_kwargs(opts)
    assert kw["fit_scat"] is True and kw["log10_tau"] is False and kw["scat_guess"] == [3e-5, 1500.0, -4.0]
    assert set(kw) == {"fit_scat", "log10_tau", "scat_guess", "print_phase", "print_flux", "print_parangle",
                       "addtnl_toa_flags", "method", "quiet"}
    opts = pptoas_run.parser().parse_args(["-d", "a.npz", "-m", "m.gmodel", "--narrowband", "--fit_scat"])
    kw = pptoas_run.get_narrowband_kwargs(opts)
    assert kw["fit_scat"] is True and kw["log10_tau"] is True and kw["scat_guess"] is None
    # (the reference's spelling of the switch still works)
    opts = pptoas_run.parser().parse_args(["-d", "a.npz", "-m", "m.gmodel", "--narrowband", "--fit_scat", "--no_logscat"])
    assert pptoas_run.get_narrowband_kwargs(opts)["log10_tau"] is False


def test_fit_phase_shift_scat_signature():
    """The signature the reference planned (pptoas.py:988-991)."""
    import inspect
    from pulseportraiture_amd.pptoaslib import fit_phase_shift_scat
    sig = inspect.signature(fit_phase_shift_scat)
    assert list(sig.parameters) == ["prof", "model_prof", "param_guesses", "P", "err", "fit_flags", "bounds",
                                    "log10_tau", "option", "sub_id", "method", "is_toa", "quiet"]
    assert sig.parameters["log10_tau"].default is True and sig.parameters["fit_flags"].default == [1, 1]
