"""The 'fit' noise method without a GPU: the NumPy restatement (tests/noisefit_refs.py) against the true
reference's fixture, the library's host-only width table against the restatement for every H, the binding, the
host definitions, and --noise_method on every command line."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from pulseportraiture_amd import _lib, pplib
from tests import noisefit_refs as nf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = np.load(os.path.join(GOLDEN, "noisefit.npz"))
NPULSE = 8
# each command with the other arguments it needs to get as far as its refusal()
COMMANDS = {"pptoas_run": ["-d", "x.npz", "-m", "x.gmodel"], "ppzap_run": ["-d", "x.npz"], "ppalign_run": ["-M", "x.txt"],
            "ppspline_run": ["-d", "x.npz"], "ppspline_smooth_run": ["-d", "x.npz"], "ppgauss_run": ["-d", "x.npz", "--autogauss", "0.05"],
            "ppgauss_join_run": ["-M", "x.txt", "--autogauss", "0.05"], "ppscrunch_run": ["-d", "x.npz"]}


@pytest.mark.parametrize("nbin", nf.LENGTHS_FIXTURE)
def test_restatement_equals_the_reference(nbin):
    rows = FIX["rows_%d" % nbin]
    assert len(rows) == NPULSE + len(nf.SPECIAL)
    for fn in nf.FNS:
        res = [nf.noise_fit_row(r, fn=fn) for r in rows]
        np.testing.assert_array_equal([r["kc"] for r in res], FIX["kc_%s_%d" % (fn, nbin)])
        np.testing.assert_array_equal([r["cell"] for r in res], FIX["cell_%s_%d" % (fn, nbin)])
        chi2 = np.array([[r["chi2_best"], r["chi2_second"]] for r in res])
        want = FIX["chi2_%s_%d" % (fn, nbin)]
        np.testing.assert_array_equal(np.isnan(chi2), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_allclose(chi2[ok], want[ok], rtol=1e-13, atol=0.0)
    noise = np.array([nf.noise_fit_row(r)["noise"] for r in rows])
    for key in ("noise_1d_%d", "noise_chans_%d", "noise_get_%d"):
        np.testing.assert_allclose(noise, FIX[key % nbin], rtol=1e-13, atol=0.0)


def test_fixture_pins_the_tie_and_the_zero_power_rules():
    at = {name: NPULSE + i for i, name in enumerate(nf.SPECIAL)}
    for nbin in nf.LENGTHS_FIXTURE:
        H = nbin // 2 + 1
        kc, cell = FIX["kc_exp_dc_%d" % nbin], FIX["cell_exp_dc_%d" % nbin]
        for name in ("zeros", "zero_sum_int"):
            assert kc[at[name]] == H - 1 and tuple(cell[at[name]]) == (0, 0, 0)
        assert FIX["noise_1d_%d" % nbin][at["zeros"]] == 0.0
        # the b = 0 winner: all 20 widths tie exactly and the first one wins
        assert tuple(cell[at["b0"]][:2]) == (0, 0)
        J = nf.chi2_grid(np.log10(nf.power_spectrum(FIX["rows_%d" % nbin][at["b0"]])), "exp_dc")[0]
        assert (J[:, 0, :] == J[0, 0, :]).all()


def test_fixture_rows_are_not_marginal():
    """Every fixture row's choice of width is far from a toss-up (the bar the GPU comparison needs)."""
    for nbin in nf.LENGTHS_FIXTURE:
        for fn in nf.FNS:
            margin = nf.noise_fit_rows(FIX["rows_%d" % nbin], fn=fn)[3]
            assert (margin >= 1e-6).all(), (nbin, fn, margin)


def test_gpu_test_rows_are_not_marginal():
    """The seeds of tests/test_gpu_noisefit.py, before any GPU run: no row of any length, and no spectrum of the
    power-spectrum entry's cases, is below the margin the integer comparison needs."""
    for nbin in nf.TEST_LENGTHS:
        for fn in nf.FNS:
            margin = nf.noise_fit_rows(nf.test_rows(nbin), fn=fn)[3]
            assert (margin >= nf.MARGIN_MIN).all(), (nbin, fn, margin)
    for H in nf.TEST_SPECTRA_H:
        for fn in nf.FNS:
            margin = np.array([nf.find_kc_full(p, fn)["margin"] for p in nf.test_spectra(H)])
            assert (margin >= nf.MARGIN_MIN).all(), (H, fn, margin)


@pytest.mark.parametrize("fn", nf.FNS)
def test_library_width_table_for_every_H(fn):
    lib = _lib.load()
    a20, kc20 = np.empty(20), np.empty(20, dtype=np.int32)
    for H in range(5, 2050):
        assert lib.pp_noise_fit_grid(H, _lib.PP_KC_FNS[fn], a20.ctypes.data_as(_lib.c_double_p),
                                     kc20.ctypes.data_as(_lib.c_int32_p)) == 0
        want_a, want_kc = nf.width_table(H, fn)
        assert a20.tobytes() == want_a.tobytes(), H
        np.testing.assert_array_equal(kc20, want_kc, err_msg=str(H))
    assert lib.pp_noise_fit_grid(33, 7, a20.ctypes.data_as(_lib.c_double_p), kc20.ctypes.data_as(_lib.c_int32_p)) != 0
    assert lib.pp_noise_fit_grid(33, 0, None, kc20.ctypes.data_as(_lib.c_int32_p)) != 0


def test_binding_has_the_new_symbols_and_the_old_abi():
    assert {"pp_channel_noise_fit", "pp_channel_snrs_fit", "pp_noise_fit_grid"} <= set(_lib.SYMBOLS)
    assert _lib.ABI_VERSION == 11
    assert _lib.SYMBOLS["pp_noise_fit_grid"] == (C.c_int, [C.c_int, C.c_int, _lib.c_double_p, _lib.c_int32_p])


def test_host_definitions_equal_the_reference():
    data, point = FIX["fkf_data"], tuple(FIX["fkf_point"])
    assert pplib.find_kc_function(point, data, 1.0, 'exp_dc') == FIX["fkf_exp_dc"]
    assert pplib.find_kc_function(point, data, 2.0, 'exp_dc') == FIX["fkf_exp_dc_errs2"]
    assert pplib.find_kc_function((7.6, 1.7, -0.4), data, 1.0, 'half_tri') == FIX["fkf_half_tri"]
    assert pplib.find_kc_function(point, data, 1.0, 'other') == 0.0
    np.testing.assert_array_equal(pplib.half_triangle_function(7.6, 1.7, -0.4, 33), FIX["half_triangle"])


def test_get_noise_keeps_ps_and_refuses_what_the_device_cannot_take(capsys):
    x = FIX["rows_64"][0]
    assert pplib.get_noise(x) == pplib.get_noise_PS(x) == pplib.get_noise(x, method="PS", frac=4)
    assert pplib.get_noise(x, method="median") == 0
    assert capsys.readouterr().out == "Unknown get_noise method.\n"
    with pytest.raises(NotImplementedError, match="ravelled"):
        pplib.get_noise_fit(np.zeros((3, 2048)))
    with pytest.raises(NotImplementedError):
        pplib.find_kc(np.ones(33), errs=np.ones(33))
    assert pplib.find_kc(np.ones(33), fn='other') == 0


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_every_command_takes_noise_method(command, capsys):
    mod = importlib.import_module("pulseportraiture_amd." + command)
    argv = COMMANDS[command]
    # (ppalign_run.parser() is the reference's option table, pinned as such; its own options come with full_parser())
    parser = getattr(mod, "full_parser", mod.parser)
    opts = parser().parse_args(argv)
    assert opts.noise_method is None and mod.refusal(opts) is None
    for value in ("fit", "PS"):
        opts = parser().parse_args(argv + ["--noise_method", value])
        assert opts.noise_method == value and mod.refusal(opts) is None
    opts = parser().parse_args(argv + ["--noise_method", "foo"])
    assert "--noise_method foo" in mod.refusal(opts)
    assert mod.main(argv + ["--noise_method", "foo"]) == 2
    assert capsys.readouterr().err.startswith(command + ": --noise_method foo")
