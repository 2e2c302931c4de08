"""Joined multi-band ppgauss fits on the host: the host restatement of the joined residual rows and the
Levenberg-Marquardt driver on a NumPy evaluator against the reference's joined fits
(tests/golden/make_golden_ppgauss_join.py), the metafile branch of DataPortrait, the join file, and the command line
of ppgauss_join_run.  No GPU."""
import os

import numpy as np
import pytest

from pulseportraiture_amd import gaussfit, gmodel, ppgauss_join_run, ppgauss_run, pplib

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def join_ichans_of(g, prefix="join_ichans"):
    out = []
    while prefix + str(len(out)) in g.files:
        out.append(g[prefix + str(len(out))])
    return out


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_host_rows_against_the_reference(nbin, code, scattered):
    """gaussfit.host_residuals with join_ichans against fit_gaussian_portrait_function's rows: the base, one step each
    of phase2, DM1, DM2, tau, a loc and the scattering index, and the base with every join parameter zero -- to 1e-12
    of the row's peak."""
    g = _g("ppgauss_join_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    data, errs, freqs = g["n%d_data" % nbin], g["errs"], g["freqs"]
    bands = [g["band0"], g["band1"]]
    sets = np.vstack([g[tag + "_sets"], g[tag + "_zero_set"][None]])
    want = np.vstack([g[tag + "_rows"], g[tag + "_zero_rows"][None]]).reshape(len(sets), len(freqs), nbin)
    got = gaussfit.host_residuals(sets, data, errs, code, freqs, float(g["nu_ref"]), bands, float(g["P"]))
    got = got.reshape(want.shape)
    peak = np.abs(want).max(axis=-1, keepdims=True)
    assert np.all(np.abs(got - want) <= 1e-12 * peak), float((np.abs(got - want) / peak).max())
    # the rotation is there: the stepped phase moves band 1's rows and no other
    moved = np.abs(want[1] - want[0]).max(axis=-1) > 0
    assert list(np.flatnonzero(moved)) == sorted(g["band1"])


def check_fit(fitted, fit_errs, chi2, dof, g):
    """The bars of the device tests' _check_fit (tests/test_gpu_ppgauss.py)."""
    want, sig = g["fitted_params"], g["fit_errs"]
    v = sig > 0
    dist = np.abs(fitted - want)[v] / sig[v]
    scatter = float(np.max(g["self_scatter"]))
    rel = np.abs(fit_errs[v] / sig[v] - 1.0)
    print("max distance %.2e sigma (self-scatter %.2e), chi2 rel %.1e, errs rel %.1e" %
          (dist.max(), scatter, chi2 / float(g["chi2"]) - 1.0, rel.max()))
    assert np.all(fitted[~v] == want[~v])
    assert np.all(fit_errs[~v] == 0.0)
    assert dist.max() <= 1e-3
    assert dist.max() <= 10 * scatter
    assert chi2 <= float(g["chi2"]) * (1 + 1e-9)
    assert rel.max() <= 1e-4
    assert dof == int(g["dof"])


def joined_fit(g, **kw):
    nchan, nbin = g["data"].shape
    ichans = join_ichans_of(g)
    return gaussfit.fit_gaussian_portrait(str(g["code"]), g["data"], g["init_params"], float(g["scattering_index_in"]),
                                          np.outer(g["errs"], np.ones(nbin)), g["fit_flags"], False,
                                          pplib.get_bin_centers(nbin), g["freqs"], float(g["nu_ref"]),
                                          join_params=[ichans, g["join_init"], g["join_flags"]], P=float(g["P"]), **kw)


@pytest.mark.parametrize("name", ["2x8x128", "3x6x100"])
def test_golden_joined_fits_on_the_numpy_evaluator(name):
    g = _g("ppgauss_join_fit_" + name)
    ichans = join_ichans_of(g)
    r = joined_fit(g, evaluator=gaussfit.numpy_evaluator(g["data"], g["errs"], str(g["code"]), g["freqs"], float(g["nu_ref"]),
                                                         ichans, float(g["P"])))
    # the reference's order: the join parameters close fitted_params and fit_errs
    assert len(r.fitted_params) == len(g["init_params"]) + 2 * len(ichans) == len(r.fit_errs)
    assert r.fitted_params[len(g["init_params"])] == 0.0 and r.fit_errs[len(g["init_params"])] == 0.0     # band 1's phase
    assert r.scattering_index == float(g["scattering_index"]) and r.scattering_index_err == 0.0
    check_fit(r.fitted_params, r.fit_errs, r.chi2, r.dof, g)
    assert r.residuals.shape == g["data"].shape
    assert np.sum((r.residuals / g["errs"][:, None]) ** 2) == pytest.approx(r.chi2, rel=1e-12)


def test_join_parameters_are_unbounded_and_counted():
    lo, hi = gaussfit.portrait_bounds(2 + 12 + 4 + 1, njoin=2)
    assert list(lo[:14]) == list(gaussfit.portrait_bounds(2 + 12 + 1)[0][:14])
    assert list(hi[:14]) == list(gaussfit.portrait_bounds(2 + 12 + 1)[1][:14])
    assert np.all(np.isinf(lo[14:])) and np.all(np.isinf(hi[14:]))
    band = gaussfit.band_of_channels([[0, 1, 3], [2, 4, 5]], 7)
    assert list(band) == [0, 0, 1, 0, 1, 1, -1]
    with pytest.raises(ValueError, match="twice"):
        gaussfit.band_of_channels([[0, 1], [1, 2]], 4)
    with pytest.raises(ValueError, match="outside"):
        gaussfit.band_of_channels([[0, 4]], 4)


def test_the_period_is_needed_and_shapes_are_checked():
    g = _g("ppgauss_join_fit_2x8x128")
    nbin = g["data"].shape[1]
    args = [str(g["code"]), g["data"], g["init_params"], -4.0, g["errs"], g["fit_flags"], False, np.arange(nbin), g["freqs"],
            float(g["nu_ref"])]
    join = [join_ichans_of(g), g["join_init"], g["join_flags"]]
    with pytest.raises(NotImplementedError, match="join.*period"):
        gaussfit.fit_gaussian_portrait(*args, join_params=join, P=None)
    with pytest.raises(ValueError, match="a phase and a DM"):
        gaussfit.fit_gaussian_portrait(*args, join_params=[join[0], join[1][:-1], join[2]], P=0.003, evaluator=lambda s, h: None)
    with pytest.raises(ValueError, match="no period"):
        gaussfit.fit_gaussian_portrait(*args, join_params=join, P=-1.0, evaluator=lambda s, h: None)
    # more than 99 varied parameters do not fit one launch: 16 components with everything free, and two bands
    rng = np.random.default_rng(0)
    init = np.concatenate([[0.0, 0.0], np.tile([0.5, 0.0, 0.05, 0.0, 1.0, 0.0], 16)])

    class FakeEngine(object):
        GAUSS_FIT_MAX_SETS, GAUSS_FIT_MAX_GAUSS, GAUSS_FIT_MAX_JOIN = 100, 16, 16
    with pytest.raises(ValueError, match="at most 99"):
        gaussfit.fit_gaussian_portrait("000", rng.standard_normal((16, nbin)), init, -4.0, g["errs"], np.ones(len(init)), False,
                                       np.arange(nbin), g["freqs"], 1500.0, join_params=join, P=0.003, engine=FakeEngine())


# ---- the metafile branch of DataPortrait ----------------------------------------------------------------
def bunches_of(m, zap=None, **extra):
    """The bands of the model golden as DataBunches, as stored (channels in descending order)."""
    from pulseportraiture_amd.pptoas import data_from_arrays
    out = []
    for i in range(2):
        sub, freqs = m["band%d_subints" % i], m["band%d_freqs" % i]
        nchan = sub.shape[2]
        w = np.ones((1, nchan))
        if zap is not None and zap[0] == i:
            w[0, zap[1]] = 0.0
        out.append(data_from_arrays(sub, freqs, m["Ps"], [55000.0], weights=w,
                                    noise_stds=np.full((1, 1, nchan), float(m["noise_std"])), SNRs=m["band%d_SNRs" % i],
                                    bw=-abs(freqs[0, 0] - freqs[0, 1]) * nchan, source="PSR_1234-5678",
                                    filename="band%d.npz" % (i + 1), **extra))
    return out


@pytest.fixture()
def host_phase_shift(monkeypatch):
    """fit_phase_shift on the host (the oracle's: scipy's brute and fmin, as the reference's)."""
    from oracle import pptoas_oracle as orc
    monkeypatch.setattr(pplib, "fit_phase_shift",
                        lambda data, model, noise=None, bounds=[-0.5, 0.5], Ns=100: orc.fit_phase_shift(data, model, noise, bounds, Ns))


def test_data_portrait_of_two_bands(host_phase_shift):
    m = _g("ppgauss_join_model")
    dp = pplib.DataPortrait(bunches_of(m))
    assert dp.njoin == 2 and dp.datafiles == ["band1.npz", "band2.npz"] and dp.nbin == 128
    for i in range(2):
        np.testing.assert_array_equal(dp.join_ichans[i], m["join_ichans%d" % i])
        np.testing.assert_array_equal(dp.join_ichanxs[i], m["join_ichanxs%d" % i])
    np.testing.assert_array_equal(dp.isort, m["isort"])
    np.testing.assert_array_equal(dp.isortx, m["isortx"])
    assert not np.array_equal(dp.isort, np.arange(16))              # (the stored order is no sorted one)
    np.testing.assert_array_equal(dp.join_fit_flags, m["join_fit_flags"])
    assert list(dp.join_fit_flags) == [0, 1, 1, 1]
    np.testing.assert_allclose(dp.join_params, m["join_params_init"], rtol=0, atol=1e-9)
    assert dp.join_params[0] == 0.0 and dp.join_params[1] == 0.0 and dp.join_params[3] == 0.0
    np.testing.assert_array_equal(dp.freqs, m["freqs"])
    np.testing.assert_array_equal(dp.port, m["port_in"])
    np.testing.assert_array_equal(dp.portx, m["port_in"])
    assert dp.Ps == [float(m["Ps"][0])] and dp.nu0 == float(m["nu0"]) and dp.bw == pytest.approx(float(m["bw"]), rel=1e-14)
    assert dp.masks.shape == (1, 1, 16, 128) and dp.noise_stds.shape == (1, 1, 16) and dp.SNRs.shape == (1, 1, 16)
    assert dp.weights.shape == (1, 16) and len(dp.noise_stdsxs) == len(dp.SNRsxs) == 16
    assert dp.all_join_params[0] is dp.join_ichanxs and dp.all_join_params[1] is dp.join_params
    # a bunch's own profile is used when it has one: five bins late, so the model's band is to be rotated to later phase
    b = bunches_of(m)
    b[1]["prof"] = np.roll(b[0]["subints"][0, 0].mean(axis=0), 5)
    assert pplib.DataPortrait(b).join_params[2] == pytest.approx(-5.0 / 128, abs=2e-3)


def test_data_portrait_with_a_zapped_channel(host_phase_shift):
    m = _g("ppgauss_join_model")
    dp = pplib.DataPortrait(bunches_of(m, zap=(int(m["zap_band"]), int(m["zap_chan"]))))
    for i in range(2):
        np.testing.assert_array_equal(dp.join_ichans[i], m["zap_join_ichans%d" % i])
        np.testing.assert_array_equal(dp.join_ichanxs[i], m["zap_join_ichanxs%d" % i])
    np.testing.assert_array_equal(dp.isortx, m["zap_isortx"])
    assert dp.join_nchans == list(m["zap_join_nchans"]) and dp.join_nchanxs == list(m["zap_join_nchanxs"])
    np.testing.assert_array_equal(dp.freqsxs[0], m["zap_freqsx"])
    np.testing.assert_allclose(dp.join_params, m["zap_join_params"], rtol=0, atol=1e-9)
    assert dp.portx.shape == (15, 128) and dp.port.shape == (16, 128) and list(dp.ok_ichans[0]) == list(np.flatnonzero(dp.weights[0]))
    assert np.all(dp.port[np.flatnonzero(dp.weights[0] == 0)] == 0.0)


def test_data_portrait_refusals(host_phase_shift):
    m = _g("ppgauss_join_model")
    with pytest.raises(RuntimeError, match="DataBunch"):
        pplib.DataPortrait("bands.txt")
    b = bunches_of(m)
    b[1]["nbin"] = 64
    with pytest.raises(ValueError, match="band2.npz.*64 bins"):
        pplib.DataPortrait(b)
    b = bunches_of(m)
    b[0]["nsub"] = 2
    with pytest.raises(ValueError, match="band1.npz.*one subint"):
        pplib.DataPortrait(b)


def test_join_file_round_trip(host_phase_shift, tmp_path, capsys):
    """write_join_parameters writes the reference's bytes and appends; a DataPortrait given the file starts from its
    last block, in the new four-column layout and in the old one without errors."""
    m = _g("ppgauss_join_model")
    dp = pplib.DataPortrait(bunches_of(m))
    dp.model_name = "PSR_1234-5678"
    dp.join_params, dp.join_param_errs = m["join_params"], m["join_param_errs"]
    want = m["join_text"].tobytes()
    assert want == open(os.path.join(GOLDEN, "ppgauss_join_model.join"), "rb").read()
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        dp.write_join_parameters()
        assert open("PSR_1234-5678.join", "rb").read() == want
        dp.join_params = dp.join_params * 2.0
        dp.write_join_parameters()                          # appended
    finally:
        os.chdir(cwd)
    text = open(str(tmp_path / "PSR_1234-5678.join"), "rb").read()
    assert text.startswith(want) and text.count(b"# archive name") == 2
    back = pplib.DataPortrait(bunches_of(m), joinfile=str(tmp_path / "PSR_1234-5678.join"))
    np.testing.assert_allclose(back.join_params[0::2], 2.0 * m["join_params"][0::2], rtol=0, atol=0.51e-10)
    np.testing.assert_allclose(back.join_params[1::2], 2.0 * m["join_params"][1::2], rtol=0, atol=0.51e-6)
    # the reference reading its own file (one block): the same numbers
    one = tmp_path / "one.join"
    one.write_bytes(want)
    np.testing.assert_array_equal(pplib.DataPortrait(bunches_of(m), joinfile=str(one)).join_params, m["join_params_read"])
    # a given joinfile is the one written to
    back.join_param_errs = m["join_param_errs"]
    back.write_join_parameters()
    assert open(str(tmp_path / "PSR_1234-5678.join"), "rb").read().count(b"# archive name") == 3
    # the old layout: name, phase, DM -- listed in another order than the metafile's
    old = tmp_path / "old.join"
    old.write_text("band2.npz   0.25   -0.002\nband1.npz   0.0   0.001\n")
    np.testing.assert_array_equal(pplib.DataPortrait(bunches_of(m), joinfile=str(old)).join_params, [0.0, 0.001, 0.25, -0.002])
    capsys.readouterr()
    bad = tmp_path / "bad.join"
    bad.write_text("band2.npz   x   y\nother.npz 0 0\n")
    kept = pplib.DataPortrait(bunches_of(m), joinfile=str(bad)).join_params
    assert "Bad join file." in capsys.readouterr().out
    np.testing.assert_allclose(kept, m["join_params_init"], rtol=0, atol=1e-9)


# ---- the command line --------------------------------------------------------------------------------------
def _opts(*argv):
    return ppgauss_join_run.parser().parse_args(list(argv))


def test_command_line_parsing_and_refusals(tmp_path, capsys):
    o = _opts("-M", "bands.txt", "--autogauss", "0.05")
    assert (o.metafile, o.joinfile, o.datafile) == ("bands.txt", None, None)
    assert (o.fixloc, o.fixwid, o.fixamp, o.fixscat, o.fixalpha, o.fgauss, o.quiet) == (True, False, False, True, True, False, True)
    assert ppgauss_join_run.refusal(o) is None and ppgauss_join_run.refusal(o, ["a.npz", "b.npz"]) is None
    o = _opts("-M", "bands.txt", "-j", "old.join", "-I", "m.gmodel", "-o", "o.gmodel", "--niter", "2", "--mcode", "011")
    assert (o.joinfile, o.modelfile, o.outfile, o.niter, o.model_code) == ("old.join", "m.gmodel", "o.gmodel", "2", "011")
    assert ppgauss_join_run.refusal(o) is None
    # the parser is ppgauss_run's own, with the same options
    assert sorted(vars(o)) == sorted(vars(ppgauss_run.parser().parse_args(["-d", "a.npz"])))
    for argv, word in ((["--autogauss", "0.05"], "-M/--metafile"),
                       (["-M", "b.txt", "-d", "a.npz", "--autogauss", "0.05"], "-d/--datafile"),
                       (["-M", "b.txt", "--figure", "f.png", "--autogauss", "0.05"], "--figure"),
                       (["-M", "b.txt", "--autogauss", "0.05", "--norm", "median"], "Unknown normalization"),
                       (["-M", "b.txt", "--gauss", "0.2,0.05"], "three numbers"),
                       (["-M", "b.txt"], "--autogauss")):
        msg = ppgauss_join_run.refusal(_opts(*argv))
        assert msg is not None and word in msg, (argv, msg)
    assert "17 archives" in ppgauss_join_run.refusal(_opts("-M", "b.txt", "--autogauss", "0.05"), ["x.npz"] * 17)
    assert "0 archives" in ppgauss_join_run.refusal(_opts("-M", "b.txt", "--autogauss", "0.05"), [])
    # main() prints the message and returns 2 before anything touches a device
    assert ppgauss_join_run.main(["--autogauss", "0.05"]) == 2
    assert "ppgauss_join_run: no metafile" in capsys.readouterr().err
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    assert ppgauss_join_run.main(["-M", str(empty), "--autogauss", "0.05"]) == 2
    assert "0 archives" in capsys.readouterr().err
    # ppgauss_run keeps refusing the joined route, and says where it lives
    for argv in (["-M", "b.txt", "--autogauss", "0.05"], ["-d", "a.npz", "-j", "x.join", "--autogauss", "0.05"]):
        assert "ppgauss_join_run" in ppgauss_run.refusal(ppgauss_run.parser().parse_args(argv))


def test_host_portrait_rotation_is_the_references_two_steps():
    """gmodel.gaussian_portrait(join_ichans=...) scatters, lets irfft drop the imaginary Nyquist part, then rotates:
    at 64 bins the edge model has Nyquist power, and rotating in the same pass as the scattering filter would keep
    Re(d_M B_M e^{2 pi i M phi}) instead of Re(d_M B_M) cos(2 pi M phi)."""
    g = _g("ppgauss_join_rows")
    v = g["n64_c000_t1_sets"][0]
    mdl = gaussfit._model_of(v, "000", float(g["nu_ref"]), 64, njoin=2)
    plain = gmodel.gaussian_portrait(mdl, g["freqs"], 64, P=64.0)
    joined = gmodel.gaussian_portrait(mdl, g["freqs"], 64, P=64.0, join_ichans=[g["band0"], g["band1"]],
                                      join_params=v[-5:-1], P_join=float(g["P"]))
    np.testing.assert_array_equal(joined[6], plain[6])                  # the channel in no band
    n = int(g["band1"][0])
    phi = v[-3] + pplib.Dconst * v[-2] / float(g["P"]) * (g["freqs"][n] ** -2.0 - float(g["nu_ref"]) ** -2.0)
    H = np.fft.rfft(plain[n])
    assert abs(H[32].real) > 1e-6 * np.abs(H).max()                     # there is Nyquist power
    want = np.fft.irfft(H * np.exp(2j * np.pi * phi * np.arange(33)))
    np.testing.assert_allclose(joined[n], want, rtol=0, atol=1e-14 * np.abs(want).max())
    with pytest.raises(ValueError, match="P_join"):
        gmodel.gaussian_portrait(mdl, g["freqs"], 64, P=64.0, join_ichans=[g["band0"]], join_params=[0.1, 0.0])
