"""make_fake_pulsar's host side: the .par reader, the delay / amplitude / epoch tables against the reference's own
composition (tests/golden/ppfake_rows.npz), the two stated departures from the reference, and the command line's
help and refusals.  No GPU."""
import os

import numpy as np
import pytest

from tests import ppfake_cases as pc


def _par():
    from pulseportraiture_amd import parfile
    return parfile.psr_par(pc.PARFILE)


def test_par_reader_on_the_example(tmp_path):
    from pulseportraiture_amd import parfile
    par = _par()
    assert par.PSR == "J1234-5678" and par.RAJ == "01:02:03.45678901" and par.DECJ == "-04:05:06.7890123"
    assert par.P0 == np.float64(1.0) / np.float64(345.67890123456789) and par.F0 == 345.67890123456789
    assert par.DM == 34.56789 and par.PEPOCH == 50000.0
    assert not hasattr(par, "F1") and not hasattr(par, "A1") and not hasattr(par, "C")
    # PSRJ stands in for PSR, P0 for F0, Fortran exponents, comment lines and unknown keys skipped
    other = tmp_path / "other.par"
    other.write_text("C PSR J0000+0000\nPSRJ  J4321-8765\nP0  2.5D-3 1\nF1 -1.2D-13\nPEPOCH 5.5D4\nDM 1.25d1\n\nJUNK\n")
    par = parfile.psr_par(str(other))
    assert par.PSR == "J4321-8765" and par.P0 == 2.5e-3 and par.F0 == 400.0 and par.PEPOCH == 55000.0 and par.DM == 12.5
    assert par.RAJ is None and par.DECJ is None
    bad = tmp_path / "bad.par"
    bad.write_text("PSR J1\nDM 3.0\n")
    with pytest.raises(ValueError, match="F0 or P0, PEPOCH"):
        parfile.psr_par(str(bad))


def _tables(case, **more):
    from pulseportraiture_amd.gmodel import parse_gmodel
    from pulseportraiture_amd.pplib import fake_pulsar_tables
    kw = {k: v for k, v in case["kwargs"].items() if k != "nbin"}
    kw.update(more)
    return fake_pulsar_tables(parse_gmodel(case["gmodel"]), _par(), **kw)


@pytest.mark.parametrize("name", pc.NAMES)
def test_host_tables_reproduce_the_reference_rows(name):
    """delays, disp_delays, amps and the model's scattering, applied to gmodel.gaussian_portrait with the oracle's
    rotate_data."""
    from oracle import pptoas_oracle as orc
    from pulseportraiture_amd.gmodel import gaussian_portrait
    case = pc.cases()[name]
    nbin = case["kwargs"]["nbin"]
    t = _tables(case, nsub=2, npol=2, tsub=60.0)
    assert t.delays.shape == (2, 6) and t.amps.shape == (2, 2, 6) and t.sigmas.shape == (6,)
    assert np.array_equal(t.delays[0], t.delays[1]) and np.array_equal(t.amps[0, 0], t.amps[1, 1])
    assert t.dmc == (1 if case["kwargs"].get("dedispersed") else 0) and t.DM == 34.56789
    np.testing.assert_array_equal(t.freqs, np.linspace(1100.0 + 800.0 / 6 / 2.0, 1100.0 + 800.0 - 800.0 / 6 / 2.0, 6))
    port = gaussian_portrait(t.model, t.freqs, nbin, t.Ps[0])
    rows = np.array([t.amps[0, 0, n] * orc.rotate_data(port[n], -t.delays[0, n]) for n in range(6)])
    # the dispersed archive: a second rotation, as PSRCHIVE's dededisperse() is one
    rows = np.array([orc.rotate_data(rows[n], -t.disp_delays[n]) for n in range(6)])
    assert bool(t.disp_delays.any()) == (not t.dmc)
    want = case["rows"]
    dev = np.abs(rows - want).max() / np.abs(want).max()
    print("%s: dev %.3e of the peak, bar %.1e" % (name, dev, case["bar"]))
    assert dev <= case["bar"]


def test_epochs_are_subint_centres_from_the_start():
    from pulseportraiture_amd.pptoas import MJD
    case = pc.cases()["plain_64"]
    t = _tables(case, nsub=3, tsub=300.0)
    # default start: PEPOCH
    assert [e.intday() for e in t.epochs] == [50000] * 3
    np.testing.assert_allclose([e.fracday() for e in t.epochs], (150.0 + 300.0 * np.arange(3)) / 86400.0, rtol=0, atol=1e-16)
    t = _tables(case, nsub=2, tsub=60.0, start_MJD=MJD(57202, 0.999999))
    assert [e.intday() for e in t.epochs] == [57203, 57203]
    np.testing.assert_allclose([e.fracday() for e in t.epochs], 0.999999 - 1.0 + np.array([30.0, 90.0]) / 86400.0, rtol=0, atol=1e-15)
    assert np.array_equal(t.Ps, np.full(2, 1.0 / 345.67890123456789))


def test_departures_from_the_reference():
    """xs None honours phase and dDM (the reference passes the unrotated model on); xs given transforms the phase
    once, whatever the number of subints and polarisations (the reference compounds it in its loops)."""
    from pulseportraiture_amd.pplib import Dconst, phase_transform
    case = pc.cases()["plain_64"]
    par = _par()
    D = Dconst / par.P0
    t0 = _tables(case, phase=0.0, dDM=0.0, dedispersed=True)
    assert not t0.delays.any()
    t = _tables(case, phase=0.13, dDM=2e-3, dedispersed=True)
    np.testing.assert_allclose(t.delays[0], 0.13 + D * 2e-3 * (t.freqs ** -2.0 - 1500.0 ** -2.0), rtol=1e-15)
    assert t.delays[0].min() < 0.13 < t.delays[0].max()
    # the dispersed state adds the ephemeris DM about nu0
    td = _tables(case, phase=0.13, dDM=2e-3, dedispersed=False)
    assert np.array_equal(td.delays, t.delays) and not t.disp_delays.any()
    np.testing.assert_allclose(td.disp_delays, D * par.DM * (t.freqs ** -2.0 - 1500.0 ** -2.0), rtol=1e-15)
    case = pc.cases()["dm_nu_64"]
    one = _tables(case, nsub=1, npol=1, dedispersed=True)
    many = _tables(case, nsub=4, npol=4, dedispersed=True)
    for i in range(4):
        assert np.array_equal(many.delays[i], one.delays[0])
    ph = phase_transform(0.13, par.DM + 2e-3, 1500.0, 1400.0, par.P0)
    term = (t.freqs ** -2.0 - 1400.0 ** -2.0) + 2e5 * (t.freqs ** -4.0 - 1400.0 ** -4.0)
    np.testing.assert_allclose(one.delays[0], ph + D * 2e-3 * term, rtol=1e-14)


def test_helpers_follow_the_reference():
    from oracle import pptoas_oracle as orc
    from pulseportraiture_amd import pplib
    rng = np.random.default_rng(3)
    port = rng.standard_normal((5, 32))
    params = [0.7, 1.3, 0.2, 0.4, 3.1, 0.55]
    np.testing.assert_array_equal(pplib.add_scintillation(port, params), orc.add_scintillation(port, params))
    assert pplib.add_scintillation(port, None, random=False) is not None
    np.testing.assert_array_equal(pplib.add_scintillation(port, None, random=False), port)
    freqs = np.linspace(1200.0, 1800.0, 5)
    np.testing.assert_array_equal(pplib.scattering_times(0.01, -3.6, freqs, 1500.0), orc.scattering_times(0.01, -3.6, freqs, 1500.0))
    # the default law of add_DM_nu is rotate_data's; Cs are padded with ones
    a = pplib.add_DM_nu(port, 0.1, 2e-3, 0.003, freqs, nu_ref=1500.0)
    np.testing.assert_allclose(a, orc.rotate_data(port, 0.1, 2e-3, 0.003, freqs, 1500.0), rtol=0, atol=1e-13)
    b = pplib.add_DM_nu(port, 0.1, 2e-3, 0.003, freqs, xs=[-2.0, -2.0], Cs=[1.0], nu_ref=1500.0)
    np.testing.assert_allclose(b, orc.rotate_data(port, 0.1, 4e-3, 0.003, freqs, 1500.0), rtol=0, atol=1e-13)
    np.testing.assert_allclose(pplib.add_DM_nu(port, 0.25), orc.rotate_data(port, 0.25), rtol=0, atol=1e-13)


def test_t_scat_rides_in_the_model_and_a_model_tau_overrides_it():
    c = pc.cases()
    t = _tables(c["t_scat_64"])
    assert t.model["params"][1] == 5e-5 * (1300.0 / 1500.0) ** -3.6 and t.model["alpha"] == -3.6
    t = _tables(c["model_tau_64"])
    assert t.model["params"][1] == 4e-5 and t.model["alpha"] == -4.0
    t = _tables(c["plain_64"])
    assert t.model["params"][1] == 0.0


def test_per_channel_arguments_are_checked():
    case = pc.cases()["plain_64"]
    with pytest.raises(ValueError, match="noise_stds"):
        _tables(case, noise_stds=np.ones(5))
    with pytest.raises(ValueError, match="scales"):
        _tables(case, scales=np.ones(7))
    t = _tables(case, noise_stds=np.arange(6.0), scales=2.0)
    assert np.array_equal(t.sigmas, np.arange(6.0)) and np.array_equal(t.amps[0, 0], np.full(6, 2.0))


def test_random_scintillation_is_drawn_per_subint_and_polarisation():
    case = pc.cases()["plain_64"]
    a = _tables(case, nsub=2, npol=2, scint=True, rng=np.random.default_rng(5)).amps
    b = _tables(case, nsub=2, npol=2, scint=True, rng=np.random.default_rng(5)).amps
    assert np.array_equal(a, b) and (a >= 0).all()
    flat = a.reshape(4, 6)
    assert all(not np.array_equal(flat[i], flat[j]) for i in range(4) for j in range(i))


def test_ppfake_run_help_and_refusals(capsys):
    from pulseportraiture_amd import ppfake_run
    assert ppfake_run.main([]) == 0
    out = capsys.readouterr().out
    for opt in ("--nfiles", "--days", "--MJD0", "--nsub", "--npol", "--nchan", "--nbin", "--nu0", "--bw", "--tsub", "--phase",
                "--dDM", "--dDM_mean", "--dDM_std", "--noise_std", "--scale", "--dedispersed", "--t_scat", "--alpha",
                "--scint", "--xs", "--Cs", "--nu_DM", "--seed", "--f64", "--quiet", "--metafile"):
        assert opt in out, opt
    with pytest.raises(SystemExit) as e:
        ppfake_run.main(["--help"])
    assert e.value.code == 0
    base = ["-m", pc.GMODEL, "-e", pc.PARFILE]
    ok = ppfake_run.parser().parse_args(base + ["--nfiles", "3", "--dDM", "6e-4,-6e-4,0", "--xs=-2,-4", "--Cs", "1,2e5"])
    assert ppfake_run.refusal(ok) is None
    for argv, word in [(["--nfiles", "0"], "--nfiles"), (["--npol", "0"], "--npol"), (["--nbin", "101"], "--nbin"),
                       (["--nbin", "8194"], "--nbin"), (["--nfiles", "2", "-o", "same.npz"], "%d"),
                       (["--dDM_mean", "3e-4"], "go together"), (["--dDM", "1e-4", "--dDM_mean", "3e-4", "--dDM_std", "1e-4"], "exclude"),
                       (["--nfiles", "3", "--dDM", "1e-4,2e-4"], "one per file"), (["--dDM", "x"], "numbers"),
                       (["--Cs", "1"], "--xs"), (["--noise_std", "-1"], "--noise_std"), (["--dDM_mean", "0", "--dDM_std", "-1"], "--dDM_std")]:
        msg = ppfake_run.refusal(ppfake_run.parser().parse_args(base + argv))
        assert msg is not None and word in msg, (argv, msg)
        assert ppfake_run.main(base + argv) == 2
    assert "ppfake_run: " in capsys.readouterr().err
    assert ppfake_run.main(["-m", pc.GMODEL, "-e", os.path.join(pc.GOLDEN, "no_such.par")]) == 1


def test_the_entry_point_is_bound():
    from pulseportraiture_amd import _lib
    import ctypes as C
    restype, argtypes = _lib.SYMBOLS["pp_fake_portraits"]
    assert restype is C.c_int and len(argtypes) == 11 and argtypes[-2:] == [C.c_uint64, C.c_int64]
    assert hasattr(_lib.load(), "pp_fake_portraits") and _lib.ABI_VERSION == 11
