"""The narrowband scattering fit on the GPU (pp_fit_phase_tau_batch, k_fps_scat) against the true reference's
one-channel fit_portrait_full (tests/golden/nbscat_*.npz, from make_golden_nbscat.py) and against the NumPy
restatement tests/nbscat_ref.py.

The bar of every field is 4 x the largest difference the true reference shows against ITSELF over the whole golden
set, between its three stored variants (trust-ncg, Newton-CG, trust-ncg from a start displaced by 1e-3 rot), with a
floor of 1e-13: phi in rotations, tau as stored (rot or log10 rot), everything else relative.  The bars are computed
here from the golden.  With PP_NBSCAT_PARITY_OUT set, the spreads, the bars and the device's largest deviations are
written there (profiles/nbscat_parity.json)."""
import os

import numpy as np
import pytest

from tests import nbscat_ref as nr
from tests.gpu_support import default_eng, dump_measured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(GOLDEN, "example.gmodel")
FITS = np.load(os.path.join(GOLDEN, "nbscat_fits.npz"))
NAMES = nr.COLS[:9]
MEASURED = {}


def deviation(a, b):
    """Per field: |dphi| in rotations (mod 1), |dtau| as stored, the rest relative to b.  a, b: [..., >= 9]."""
    a, b = np.asarray(a, dtype=np.float64)[..., :9], np.asarray(b, dtype=np.float64)[..., :9]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(a - b) / np.abs(b)
    d[..., 0] = np.abs((a[..., 0] - b[..., 0] + 0.5) % 1.0 - 0.5)
    d[..., 2] = np.abs(a[..., 2] - b[..., 2])
    return d


def _spread():
    out = FITS["out"]
    s = np.maximum(np.maximum(deviation(out[:, 1], out[:, 0]), deviation(out[:, 2], out[:, 0])),
                   deviation(out[:, 2], out[:, 1]))
    return s.max(axis=0)


SPREAD = _spread()
BARS = np.maximum(4.0 * SPREAD, 1e-13)


def _note(section, dev):
    dev = np.asarray(dev, dtype=np.float64).reshape(-1, 9).max(axis=0)
    MEASURED[section] = {n: (None if np.isnan(v) else float(v)) for n, v in zip(NAMES, dev)}     # (null: not compared)
    print(section, " ".join("%s %.2e/%.2e" % (n, v, b) for n, v, b in zip(NAMES, dev, BARS)))


def _within(section, got, want, cols=range(9)):
    dev = deviation(got, want)
    _note(section, dev)
    for c in cols:
        assert np.all(dev[..., c] <= BARS[c]), (section, NAMES[c], float(np.nanmax(dev[..., c])), BARS[c])
        assert not np.isnan(dev[..., c]).any(), (section, NAMES[c])


@pytest.fixture(scope="module", autouse=True)
def _write_measured():
    yield
    if MEASURED:
        dump_measured("PP_NBSCAT_PARITY_OUT",
                      dict(fields=list(NAMES), reference_spread=dict(zip(NAMES, map(float, SPREAD))),
                           bars=dict(zip(NAMES, map(float, BARS))), device_max_deviation=MEASURED))


# ---- fit level: every golden case ---------------------------------------------------------------------
def test_fit_level_parity_on_all_golden_cases():
    nbins, l10s = FITS["nbin"], FITS["log10_tau"]
    got = np.full((len(nbins), 11), np.nan)
    for nbin in (256, 100, 1024):
        rows = np.where(nbins == nbin)[0]
        for l10 in (True, False):
            sel = [j for j, i in enumerate(rows) if bool(l10s[i]) == l10]
            idx = rows[sel]
            got[idx] = default_eng().fit_phase_tau_batch(FITS["prof_%d" % nbin][sel], FITS["mprof_%d" % nbin][sel],
                                                  noise=FITS["sigma"][idx], tau_guess=FITS["guess"][idx], log10_tau=l10)
    assert len(got) == 24 and np.all(got[:, 10] == 2), got[:, 10]
    assert np.all(got[:, 9] >= 3) and np.all(got[:, 9] <= 64)
    _within("fit_level_vs_trust_ncg", got, FITS["out"][:, 0])


# ---- sizes where the kernel can go wrong --------------------------------------------------------------
SIZES = [100, 256, 1024, 2048, 4096]
_SYNTH = {}


def synth(nbin, nprof=37):
    """nprof scattered, shifted, noisy copies of a two-component profile, and SciPy's fit of each (computed once)."""
    if nbin not in _SYNTH:
        rng = np.random.default_rng(4200 + nbin)
        ph = (np.arange(nbin) + 0.5) / nbin
        model = np.exp(-0.5 * ((ph - 0.4) / 0.02) ** 2) + 0.4 * np.exp(-0.5 * ((ph - 0.47) / 0.035) ** 2)
        k = np.arange(nbin // 2 + 1)
        tau = rng.uniform(0.004, 0.03, nprof)
        phi = rng.uniform(-0.5, 0.5, nprof)
        amp = rng.uniform(0.5, 2.0, nprof)
        sigma = np.full(nprof, 0.05)
        F = np.fft.rfft(model)[None] * amp[:, None] / (1.0 + 2.0j * np.pi * k[None] * tau[:, None]) * \
            np.exp(-2.0j * np.pi * k[None] * phi[:, None])
        data = np.fft.irfft(F, nbin, axis=-1) + rng.normal(0.0, 0.05, (nprof, nbin))
        guess = np.log10(1.3 * tau)
        want = np.array([nr.fit(data[i], model, sigma[i], guess[i], None, True) for i in range(nprof)])
        _SYNTH[nbin] = dict(data=data, model=np.tile(model, (nprof, 1)), sigma=sigma, guess=guess, want=want, tau=tau)
    return _SYNTH[nbin]


@pytest.mark.parametrize("nbin", SIZES)
def test_sizes_batch_of_37_against_the_restatement(nbin):
    s = synth(nbin)
    got = default_eng().fit_phase_tau_batch(s["data"], s["model"], noise=s["sigma"], tau_guess=s["guess"], log10_tau=True)
    assert np.all(got[:, 10] == 2), got[:, 10]
    _within("sizes_nbin%d_nprof37" % nbin, got, s["want"])


@pytest.mark.parametrize("nbin", SIZES)
def test_sizes_one_profile_linear_tau_against_the_restatement(nbin):
    s = synth(nbin)
    i = 5
    want = nr.fit(s["data"][i], s["model"][i], s["sigma"][i], 1.3 * s["tau"][i], None, False)
    got = default_eng().fit_phase_tau_batch(s["data"][i], s["model"][i], noise=s["sigma"][i:i + 1],
                                     tau_guess=1.3 * s["tau"][i], log10_tau=False)
    assert got.shape == (1, 11) and got[0, 10] == 2
    _within("sizes_nbin%d_nprof1_linear" % nbin, got[0], want)


@pytest.mark.parametrize("nbin", SIZES)
def test_batch_independence(nbin):
    """Profile 17 of the 37 fitted alone equals itself in the batch, bit for bit, in every output."""
    s = synth(nbin)
    e = default_eng()
    batch = e.fit_phase_tau_batch(s["data"], s["model"], noise=s["sigma"], tau_guess=s["guess"], log10_tau=True)
    alone = e.fit_phase_tau_batch(s["data"][17], s["model"][17], noise=s["sigma"][17:18], tau_guess=s["guess"][17],
                                  log10_tau=True)
    assert alone[0].tobytes() == batch[17].tobytes()


def test_measured_noise_matches_the_restatement():
    """noise = None: sigma from the top quarter of the power spectrum, as fit_phase_shift_batch measures it."""
    s = synth(256)
    got = default_eng().fit_phase_tau_batch(s["data"][:3], s["model"][:3], noise=None, tau_guess=s["guess"][:3], log10_tau=True)
    want = np.array([nr.fit(s["data"][i], s["model"][i], None, s["guess"][i], None, True) for i in range(3)])
    _within("measured_noise", got, want)


# ---- degenerate rows inside an otherwise good batch ---------------------------------------------------
@pytest.mark.parametrize("log10_tau", [True, False])
def test_degenerate_rows_do_not_disturb_their_neighbours(log10_tau):
    s = synth(256)
    rng = np.random.default_rng(9)
    n = 12
    data, model = s["data"][:n].copy(), s["model"][:n].copy()
    guess = s["guess"][:n] if log10_tau else 10.0 ** s["guess"][:n]
    e = default_eng()
    clean = e.fit_phase_tau_batch(data, model, noise=s["sigma"][:n], tau_guess=guess, log10_tau=log10_tau)
    assert np.all(clean[:, 10] == 2)
    bad = {2: "zero data", 5: "zero model", 7: "nan", 10: "noise only"}
    data[2] = 0.0
    model[5] = 0.0
    data[7] = np.nan
    data[10] = rng.normal(0.0, 0.05, 256)
    got = e.fit_phase_tau_batch(data, model, noise=s["sigma"][:n], tau_guess=guess, log10_tau=log10_tau)
    for i, what in bad.items():
        assert got[i, 10] not in (0, 1, 2, 4), (what, got[i])
        assert np.isnan(got[i, [0, 1, 2, 3, 8]]).all(), (what, got[i])
        assert 0 <= got[i, 9] <= 64
    for i in range(n):
        if i not in bad:
            assert got[i].tobytes() == clean[i].tobytes(), i
    # NaN in the noise or in the guess of one row
    sig = s["sigma"][:n].copy()
    sig[3] = np.inf
    g2 = np.array(guess, dtype=np.float64)
    g2[4] = np.nan
    got = e.fit_phase_tau_batch(s["data"][:n], s["model"][:n], noise=sig, tau_guess=g2, log10_tau=log10_tau)
    assert got[3, 10] == 3 and got[4, 10] == 3
    assert got[0].tobytes() == clean[0].tobytes() and got[11].tobytes() == clean[11].tobytes()


def test_argument_checks_return_before_device_work():
    from pulseportraiture_amd.engine import EngineError
    e = default_eng()
    x = np.ones((2, 256))
    for kw, a in ((dict(Ns=0), x), (dict(), np.ones((2, 255))), (dict(), np.ones((2, 4098))), (dict(), np.ones((2, 6)))):
        with pytest.raises(EngineError):
            e.fit_phase_tau_batch(a, a, noise=[0.1, 0.1], tau_guess=0.01, log10_tau=False, **kw)


# ---- tau -> 0 ---------------------------------------------------------------------------------------------
def _unscattered(nbin=256, n=6):
    rng = np.random.default_rng(31)
    ph = (np.arange(nbin) + 0.5) / nbin
    model = np.exp(-0.5 * ((ph - 0.4) / 0.02) ** 2) + 0.4 * np.exp(-0.5 * ((ph - 0.47) / 0.035) ** 2)
    k = np.arange(nbin // 2 + 1)
    phi, amp = rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 2.0, n)
    data = np.fft.irfft(np.fft.rfft(model)[None] * amp[:, None] * np.exp(-2.0j * np.pi * k[None] * phi[:, None]), nbin, axis=-1)
    return data, np.tile(model, (n, 1)), np.full(n, 0.05)


def test_tau_to_zero_agrees_with_the_phase_only_fit():
    """Linear tau on unscattered (noise-free) data: phi, phi_err, scale and snr are those of
    fit_phase_shift_batch(finish='newton') under the fit-level bars, and |tau| <= 3 tau_err.

    At tau = 0 the (phi, tau) block of the Hessian is K [[1, 1], [1, 1]] for any profile (d conj(B_k) / dtau = i w
    is the derivative of the phasor by phi / 2 pi): a scattering time and a delay cannot be told apart there.  The
    device reports that as a singular Hessian -- return code 3, no covariance, tau_err infinite -- with the phase,
    its error and the amplitude's at the fixed tau it ended on, which is the phase-only fit."""
    data, model, sigma = _unscattered()
    e = default_eng()
    got = e.fit_phase_tau_batch(data, model, noise=sigma, tau_guess=0.0, log10_tau=False)
    fps = e.fit_phase_shift_batch(data, model, noise=sigma, finish='newton')
    assert np.all(np.abs(got[:, 2]) <= 3.0 * got[:, 3]), got[:, 2:4]
    want = np.full((len(got), 9), np.nan)
    want[:, 0], want[:, 1], want[:, 4], want[:, 6] = fps[:, 0], fps[:, 1], fps[:, 2], fps[:, 4]
    _within("tau_to_zero", got, want, cols=(0, 1, 4, 6))
    assert np.all(got[:, 10] == 3) and np.isinf(got[:, 3]).all() and np.isnan(got[:, 8]).all(), got
    np.testing.assert_allclose(got[:, 5], fps[:, 3], rtol=BARS[5])
    assert np.all(np.abs(got[:, 2]) < 1e-8), got[:, 2]


# ---- caller level -------------------------------------------------------------------------------------
def _bunch(g):
    from pulseportraiture_amd.pptoas import MJD, data_from_arrays
    epochs = [MJD(int(d), float(f)) for d, f in zip(g["epoch_days"], g["epoch_fracs"])]
    return data_from_arrays(
        g["subints"], g["freqs"], g["Ps"], epochs, weights=g["weights"], noise_stds=g["noise_stds"], SNRs=g["SNRs"],
        DM=float(g["scal_DM"]), doppler_factors=g["doppler_factors"], backend_delay=float(g["scal_backend_delay"]),
        telescope=str(g["scal_telescope"]), telescope_code=str(g["scal_telescope_code"]), backend=str(g["scal_backend"]),
        frontend=str(g["scal_frontend"]), bw=float(g["scal_bw"]), nu0=float(g["scal_nu0"]), subtimes=g["subtimes"],
        source=str(g["scal_source"]), filename="fake.fits")


@pytest.mark.parametrize("name", ["nbscat_gettoas_log10", "nbscat_gettoas_lin"])
def test_get_narrowband_TOAs_fit_scat_matches_the_reference_fits(name):
    from pulseportraiture_amd.pptoas import GetTOAs
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    l10 = bool(g["kw_log10_tau"])
    gt = GetTOAs(_bunch(g), MODEL, quiet=True)
    gt.get_narrowband_TOAs(fit_scat=True, log10_tau=l10, scat_guess=tuple(g["kw_scat_guess"]), quiet=True)
    used = g["weights"] > 0
    used[[i for i in range(len(used)) if i not in set(g["out_ok_isubs"])]] = False
    assert used.sum() == 12 and not used[2].any()
    assert gt.nfit == 2 and gt.fit_flags == [1, 1] and gt.log10_tau == l10
    np.testing.assert_array_equal(gt.ok_isubs[0], g["out_ok_isubs"])
    assert len(gt.TOA_list) == used.sum()
    got = np.stack([np.asarray(getattr(gt, f)[0], dtype=np.float64) for f in
                    ("phis", "phi_errs", "taus", "tau_errs", "scales", "scale_errs", "channel_snrs")], axis=-1)
    want = np.stack([g["out_" + f] for f in ("phis", "phi_errs", "taus", "tau_errs", "scales", "scale_errs",
                                             "channel_snrs")], axis=-1)
    cov = gt.covariances[0]
    assert cov.shape == (3, 8, 2, 2)
    full_got = np.concatenate([got, np.full(got.shape[:2] + (1,), 1.0), cov[..., 0, 1][..., None]], axis=-1)
    full_want = np.concatenate([want, np.full(got.shape[:2] + (1,), 1.0), g["out_phi_tau_cov"][..., None]], axis=-1)
    _within("caller_" + name, full_got[used], full_want[used])
    np.testing.assert_array_equal(cov[..., 1, 0], cov[..., 0, 1])
    np.testing.assert_array_equal(cov[..., 0, 0][used], gt.phi_errs[0][used] ** 2)
    np.testing.assert_array_equal(cov[..., 1, 1][used], gt.tau_errs[0][used] ** 2)
    assert np.all(gt.rcs[0][used] == 2) and np.all(gt.nfevals[0][used] >= 3)
    # the zapped subint and the masked channels are left at zero
    for f in ("phis", "phi_errs", "taus", "tau_errs", "scales", "scale_errs", "channel_snrs", "nfevals", "rcs"):
        assert not np.asarray(getattr(gt, f)[0])[~used].any(), f
    assert not cov[~used].any()
    # TOAs: the MJD to the time the phase bar corresponds to, the error like phi_err
    for isub, ichan in zip(*np.where(used)):
        t = gt.TOAs[0][isub, ichan]
        dt = (t.intday() - g["out_TOA_days"][isub, ichan]) + (t.fracday() - g["out_TOA_fracs"][isub, ichan])
        assert abs(dt * 86400.0 / g["Ps"][isub]) <= BARS[0] + 1e-11, (isub, ichan)    # (1e-11 rot: an MJD fraction's ulp)
    np.testing.assert_allclose(np.asarray(gt.TOA_errs[0], dtype=float)[used], g["out_TOA_errs"][used], rtol=BARS[1])
    t0 = gt.TOA_list[0]
    assert sorted(t0.flags.keys()) == list(g["out_toa0_flag_names"])
    for k, v in zip(g["out_toa0_scat_names"], g["out_toa0_scat_values"]):
        np.testing.assert_allclose(t0.flags[str(k)], v, rtol=1e-5)
    for toa in gt.TOA_list:
        assert "phi_tau_cov" in toa.flags and "scat_time" in toa.flags
        assert ("log10_scat_time" in toa.flags) == l10 and ("scat_time_err" in toa.flags) == (not l10)


def test_get_narrowband_TOAs_without_fit_scat_is_unchanged():
    """fit_scat=False still reproduces the reference's own narrowband run (gettoas_narrowband.npz)."""
    from pulseportraiture_amd.pptoas import GetTOAs
    g = np.load(os.path.join(GOLDEN, "gettoas_narrowband.npz"))
    gt = GetTOAs(_bunch(g), MODEL, quiet=True)
    gt.get_narrowband_TOAs(fit_scat=False, quiet=True)
    assert len(gt.TOA_list) == int(g["out_ntoa"]) and gt.nfit == 1 and gt.fit_flags == [1, 0] and gt.log10_tau is False
    used = g["weights"] > 0
    used[[i for i in range(len(used)) if i not in set(g["out_ok_isubs"])]] = False
    dph = np.abs((gt.phis[0] - g["out_phis"] + 0.5) % 1.0 - 0.5)
    assert dph[used].max() < 1e-11 and not gt.phis[0][~used].any()
    for fld in ("phi_errs", "scales", "scale_errs", "channel_snrs", "TOA_errs"):
        np.testing.assert_allclose(np.asarray(getattr(gt, fld)[0], dtype=float)[used], g["out_" + fld][used], rtol=1e-8)
    assert not gt.taus[0].any() and not gt.tau_errs[0].any() and gt.covariances[0].shape == (5, 32, 1, 1)
    assert sorted(gt.TOA_list[0].flags.keys()) == list(g["out_toa0_flag_names"])


def test_fit_phase_shift_scat_returns_the_planned_fields():
    from pulseportraiture_amd.pptoaslib import fit_phase_shift_scat
    s = synth(256)
    r = fit_phase_shift_scat(s["data"][0], s["model"][0], [None, s["guess"][0]], 0.003, s["sigma"][0], log10_tau=True)
    w = s["want"][0]
    _within("fit_phase_shift_scat", [r.phi, r.phi_err, r.tau, r.tau_err, r.scale, r.scale_err, r.snr, r.red_chi2,
                                     r.covariance_matrix[0, 1]], w)
    assert r.phase == r.phi and r.covariance_matrix.shape == (2, 2) and r.return_code == 2 and r.nfeval >= 3
    assert r.chi2 == r.red_chi2 * 253 and r.duration > 0
    p = fit_phase_shift_scat(s["data"][0], s["model"][0], [None, 0.0], 0.003, s["sigma"][0], fit_flags=[1, 0])
    assert hasattr(p, "phase") and hasattr(p, "phase_err") and not hasattr(p, "tau")


def test_command_line_writes_the_scattering_flags(tmp_path):
    """pptoas_run --narrowband --fit_scat on an .npz archive: one .tim line per good channel, each with the
    scattering flags of its log10_tau setting."""
    from pulseportraiture_amd import pptoas_run
    from pulseportraiture_amd.pptoas import MJD
    g = np.load(os.path.join(GOLDEN, "nbscat_gettoas_log10.npz"))
    epochs = np.empty(len(g["epoch_days"]), dtype=object)
    epochs[:] = [MJD(int(d), float(f)) for d, f in zip(g["epoch_days"], g["epoch_fracs"])]
    arch = tmp_path / "a.npz"
    np.savez(arch, subints=g["subints"], freqs=g["freqs"], Ps=g["Ps"], epochs=epochs, weights=g["weights"],
             noise_stds=g["noise_stds"], SNRs=g["SNRs"], DM=float(g["scal_DM"]), doppler_factors=g["doppler_factors"],
             backend_delay=float(g["scal_backend_delay"]), telescope=str(g["scal_telescope"]),
             telescope_code=str(g["scal_telescope_code"]), backend=str(g["scal_backend"]),
             frontend=str(g["scal_frontend"]), bw=float(g["scal_bw"]), nu0=float(g["scal_nu0"]),
             subtimes=g["subtimes"], source=str(g["scal_source"]))
    for extra, want, absent in (([], ("-log10_scat_time ", "-log10_scat_time_err "), "-scat_time_err "),
                                (["--no_log10_tau"], ("-scat_time_err ",), "-log10_scat_time ")):
        tim = tmp_path / ("nb%d.tim" % len(extra))
        assert pptoas_run.main(["-d", str(arch), "-m", MODEL, "-o", str(tim), "--narrowband", "--fit_scat",
                                "--scat_guess", "45e-6,1500,-4.0", "--quiet"] + extra) == 0
        lines = [ln for ln in tim.read_text().splitlines() if ln.strip() and not ln.startswith("FORMAT")]
        assert len(lines) == 12, lines
        for ln in lines:
            assert "-scat_time " in ln and "-phi_tau_cov " in ln and absent not in ln, ln
            for w in want:
                assert w in ln, ln
