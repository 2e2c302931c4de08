"""ppscrunch without a GPU: the ABI's bookkeeping, the group planning, the host bookkeeping of tscrunch / fscrunch /
pscrunch, the epoch rule, load_data's order of operations and refusals, the ppscrunch_run command and the callers -- with
a stub engine whose scrunch, rotate_portraits, channel_noise and channel_snrs are NumPy (tests/scrunch_refs.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pulseportraiture_amd import _lib, archive, pplib, pptoas, ppscrunch_run, scrunch
from pulseportraiture_amd.pptoas import MJD
from tests import scrunch_refs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "example.gmodel")


NumpyEngine = sr.NumpyEngine


def _bunch(state="Coherence", dmc=1, DM=12.5, seed=3):
    """5 x 2 x 6 x 16: zero weights, subint 3 dead, channel 5 dead in subints 2 .. 4 (time group 1 of 2 has a dead cell)."""
    rng = np.random.default_rng(seed)
    nsub, npol, nchan, nbin = 5, 2, 6, 16
    w = rng.uniform(0.5, 2.0, size=(nsub, nchan))
    w[0, 1] = w[1, 2] = 0.0
    w[3] = 0.0
    w[2:, 5] = 0.0
    freqs = np.linspace(1200.0, 1700.0, nchan) + 0.01 * np.arange(nsub)[:, None]
    epochs = [MJD(57000, 0.2 + 0.003 * i + 1e-5 * i * i) for i in range(nsub)]
    d = pptoas.data_from_arrays(rng.normal(size=(nsub, npol, nchan, nbin)), freqs, 0.004 + 1e-9 * np.arange(nsub), epochs,
                                weights=w, noise_stds=np.ones((nsub, npol, nchan)), SNRs=np.ones((nsub, npol, nchan)),
                                DM=DM, dmc=dmc, doppler_factors=1.0 + 1e-5 * np.arange(nsub), bw=600.0, nu0=1450.0,
                                subtimes=10.0 + np.arange(nsub), parallactic_angles=0.1 * np.arange(nsub),
                                filename="five.npz")
    d.state = state
    return d


def _consistent(d):
    nsub, npol, nchan, nbin = d.subints.shape
    assert (d.nsub, d.npol, d.nchan, d.nbin) == (nsub, npol, nchan, nbin)
    assert d.weights.shape == (nsub, nchan) and d.freqs.shape == (nsub, nchan)
    assert d.noise_stds.shape == (nsub, npol, nchan) and d.SNRs.shape == (nsub, npol, nchan)
    assert len(d.Ps) == len(d.epochs) == len(d.subtimes) == len(d.doppler_factors) == len(d.parallactic_angles) == nsub
    assert [list(c) for c in d.ok_ichans] == [list(np.where(d.weights[i] > 0)[0]) for i in range(nsub)]
    assert list(d.ok_isubs) == [i for i in range(nsub) if (d.weights[i] > 0).any()]
    assert np.array_equal(d.masks, (d.weights > 0)[:, None, :, None])
    assert d.integration_length == float(np.sum(d.subtimes))


def test_pp_scrunch_is_bound_and_declared():
    assert "pp_scrunch" in _lib.SYMBOLS and len(_lib.SYMBOLS["pp_scrunch"][1]) == 16
    with open(os.path.join(ROOT, "include", "pp_toas.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pp_scrunch\s*\(", header)
    assert all(("#define PP_POL_%s" % k.upper()) in header and str(v) for k, v in _lib.PP_POL.items())
    assert _lib.ABI_VERSION == 11


def test_group_planning():
    assert list(scrunch.plan_groups(5, 2)) == [0, 3, 5]
    assert list(scrunch.plan_groups(5)) == [0, 5] and list(scrunch.plan_groups(5, 1)) == [0, 5]
    assert list(scrunch.plan_groups(7, 3)) == [0, 3, 5, 7] and list(scrunch.plan_groups(4, 4)) == [0, 1, 2, 3, 4]
    assert list(scrunch.plan_groups(5, 2)) == list(sr.group_offsets(5, 2))
    for bad in (6, 0, -1):
        with pytest.raises(ValueError):
            scrunch.plan_groups(5, bad)


def test_tscrunch_bookkeeping():
    eng, d = NumpyEngine(), _bunch()
    t = scrunch.tscrunch(d, nsub=2, engine=eng)
    _consistent(t)
    w = d.weights
    want, wwant, _ = sr.scrunch_ref(d.subints, w, [0, 3, 5], None, "keep")
    assert np.array_equal(t.subints, want) and np.array_equal(t.weights, wwant)
    assert t.weights[1, 5] == 0.0 and not t.subints[1, :, 5].any()          # the dead cell
    assert (t.nsub, t.npol, t.nchan) == (2, 2, 6) and d.nsub == 5            # a new bunch
    Ws = w.sum(axis=1)
    for g, sl in enumerate((slice(0, 3), slice(3, 5))):
        assert t.subtimes[g] == d.subtimes[sl].sum()
        for k in ("Ps", "doppler_factors", "parallactic_angles"):
            assert np.isclose(t[k][g], (Ws[sl] * d[k][sl]).sum() / Ws[sl].sum(), rtol=1e-15, atol=0)
        for c in range(6):
            tot = w[sl, c].sum()
            nu = (w[sl, c] * d.freqs[sl, c]).sum() / tot if tot > 0 else d.freqs[sl, c].mean()
            assert np.isclose(t.freqs[g, c], nu, rtol=1e-15, atol=0)
    assert t.integration_length == d.integration_length and t.bw == 600.0 and t.nu0 == 1450.0
    assert t.dmc == 1 and t.DM == 12.5 and t.state == "Coherence"
    # noise and S/N are measured from the scrunched rows
    assert np.array_equal(t.noise_stds, t.subints.std(axis=-1))
    one = scrunch.tscrunch(d, engine=eng)
    _consistent(one)
    assert one.nsub == 1 and list(one.ok_isubs) == [0]


def test_epoch_rule():
    eng, d = NumpyEngine(), _bunch()
    t = scrunch.tscrunch(d, nsub=2, engine=eng)
    Ws = d.weights.sum(axis=1)
    for g, members in enumerate(([0, 1, 2], [3, 4])):
        e0 = d.epochs[members[0]]
        good = [s for s in members if Ws[s] > 0]
        ebar = e0 + MJD(0, sum(Ws[s] * (d.epochs[s] - e0).in_days() for s in good) / sum(Ws[s] for s in good))
        anchor = min(good, key=lambda s: abs((d.epochs[s] - ebar).in_days()))
        k = np.round((ebar - d.epochs[anchor]).in_days() * 86400.0 / t.Ps[g])
        got = (t.epochs[g] - d.epochs[anchor])
        turns = (got.intday() * 86400.0 + got.fracday() * 86400.0) / t.Ps[g]
        assert abs(turns - k) < 1e-6 and (k != 0) == (g == 0)          # a whole number of periods from the anchor (group 1 has one good member)
        assert abs((t.epochs[g] - ebar).in_days()) * 86400.0 <= 0.5 * t.Ps[g] * (1 + 1e-9)
    assert anchor == 4          # (subint 3 is dead: it cannot be the anchor)


def test_fscrunch_and_pscrunch_bookkeeping():
    eng, d = NumpyEngine(), _bunch()
    f = scrunch.fscrunch(d, nchan=3, engine=eng)
    _consistent(f)
    want, wwant, _ = sr.scrunch_ref(d.subints, d.weights, None, [0, 2, 4, 6], "keep")
    assert np.array_equal(f.subints, want) and np.array_equal(f.weights, wwant)
    assert f.nchan == 3 and list(f.ok_isubs) == [0, 1, 2, 4] and f.bw == 600.0 and f.nu0 == 1450.0
    for i in range(5):
        for g in range(3):
            sl = slice(2 * g, 2 * g + 2)
            tot = d.weights[i, sl].sum()
            nu = (d.weights[i, sl] * d.freqs[i, sl]).sum() / tot if tot > 0 else d.freqs[i, sl].mean()
            assert np.isclose(f.freqs[i, g], nu, rtol=1e-15, atol=0)
    assert not any(c[0] == "rotate" for c in eng.log)          # dedispersed: summed as it is
    # stored dispersed: the member channels are rotated to their group's frequency first, dmc stays 0
    eng2, disp = NumpyEngine(), _bunch(dmc=0)
    f2 = scrunch.fscrunch(disp, nchan=3, engine=eng2)
    _consistent(f2)
    assert f2.dmc == 0 and any(c[0] == "rotate" and c[1] == 12.5 for c in eng2.log)
    assert not np.array_equal(f2.subints, f.subints)
    # pscrunch by state
    p = scrunch.pscrunch(d, engine=eng)
    _consistent(p)
    live = d.weights != 0
    assert p.npol == 1 and p.state == "Intensity" and np.array_equal(p.weights, d.weights)
    assert np.array_equal(p.subints[:, 0][live], (d.subints[:, 0] + d.subints[:, 1])[live])
    s = scrunch.pscrunch(_bunch(state="Stokes"), engine=eng)
    assert s.npol == 1 and np.array_equal(s.subints[:, 0][live], d.subints[:, 0][live])
    i = scrunch.pscrunch(s, engine=eng)
    assert i.npol == 1 and np.array_equal(i.subints, s.subints)


def test_dedisperse_and_back():
    eng, d = NumpyEngine(), _bunch(dmc=0)
    a = scrunch.dedisperse(d, engine=eng)
    assert a.dmc == 1 and eng.log[0] == ("rotate", 12.5, 1450.0)
    assert scrunch.dedisperse(a, engine=eng).subints is a.subints          # already so: nothing is done
    b = scrunch.dededisperse(a, engine=eng)
    # (there and back gives the rows again up to the Nyquist harmonic, of which every inverse transform keeps the real part)
    assert b.dmc == 0 and np.allclose(np.fft.rfft(b.subints)[..., :-1], np.fft.rfft(d.subints)[..., :-1], atol=1e-12)
    assert scrunch.dededisperse(d, engine=eng).subints is d.subints


def test_load_data_order_and_refusals(capsys):
    eng, d = NumpyEngine(), _bunch(dmc=0)
    out = pplib.load_data(d, dedisperse=True, tscrunch=True, pscrunch=True, fscrunch=True, flux_prof=True, quiet=True,
                          engine=eng)
    ops = [c for c in eng.log if c[0] in ("rotate", "scrunch")]
    assert ops[0][0] == "rotate"                                             # dedisperse
    assert ops[1] == ("scrunch", 1, None, "keep")                            # tscrunch
    assert ops[2] == ("scrunch", None, None, "sum01")                        # pscrunch
    assert ops[3] == ("scrunch", None, 1, "keep")                            # fscrunch
    assert out.subints.shape == (1, 1, 1, 16) and out.arch is None and out.state == "Intensity"
    assert out.prof.shape == (16,) and np.allclose(out.prof, out.subints[0, 0, 0], atol=1e-12)
    # (flux_prof has the channels the archive has after its own fscrunch, as in the reference)
    assert out.flux_prof.shape == (1,) and out.prof_noise > 0 and out.prof_SNR == out.prof_SNR
    assert pplib.load_data(d, flux_prof=True, quiet=True, engine=eng).flux_prof.shape == (6,)
    d2 = _bunch()
    d2.prof_SNR = 123.0
    assert pplib.load_data(d2, quiet=True, engine=eng).prof_SNR == 123.0     # the archive's own
    with pytest.raises(NotImplementedError, match="baseline"):
        pplib.load_data(d, rm_baseline=True, quiet=True, engine=eng)
    with pytest.raises(NotImplementedError, match="Intensity"):
        pplib.load_data(d, state="Stokes", quiet=True, engine=eng)
    assert pplib.load_data(d, state="Intensity", quiet=True, engine=eng).npol == 1
    capsys.readouterr()
    pplib.load_data(d, engine=eng)
    text = capsys.readouterr().out
    assert "Reading data from five.npz" in text and "# subints          = 5" in text and "pol'n state        = Coherence" in text


def test_ppscrunch_run_parser_and_round_trip(tmp_path):
    o = ppscrunch_run.parser().parse_args("-d a.npz -T -F -p -D -e x.npz --metafile m.txt --quiet".split())
    assert (o.datafiles, o.tscrunch, o.fscrunch, o.pscrunch, o.dedisperse, o.dededisperse, o.ext, o.metafile, o.quiet) == \
        ("a.npz", True, True, True, True, False, "x.npz", "m.txt", True)
    o = ppscrunch_run.parser().parse_args("-d a.npz --setnsub 4 --setnchn 8 --dededisperse -o out.npz".split())
    assert (o.setnsub, o.setnchn, o.dededisperse, o.outfile, o.ext) == (4, 8, True, "out.npz", "scr.npz")
    assert ppscrunch_run.refusal(o) is None
    for bad in ("-d a -T --setnsub 2", "-d a -F --setnchn 2", "-d a -D --dededisperse", "-d a --setnsub 0"):
        assert ppscrunch_run.refusal(ppscrunch_run.parser().parse_args(bad.split())) is not None
    assert ppscrunch_run.output_name("/x/y/arch.npz", "scr.npz") == "/x/y/arch.scr.npz"
    eng = NumpyEngine()
    t = ppscrunch_run.scrunched(_bunch(), ppscrunch_run.parser().parse_args("-d a --setnsub 2 -p".split()), eng)
    name = ppscrunch_run.write_archive(str(tmp_path / "t.scr.npz"), t)
    back, fname = archive.load_bunch(name)
    assert fname == name and back.state == "Intensity"
    for k in ("subints", "freqs", "Ps", "weights", "noise_stds", "SNRs", "doppler_factors", "subtimes",
              "parallactic_angles", "ok_isubs", "masks"):
        assert np.array_equal(np.asarray(back[k]), np.asarray(t[k])), k
    for k in ("DM", "dmc", "nsub", "npol", "nchan", "nbin", "telescope", "source", "integration_length"):
        assert back[k] == t[k], k
    assert float(back.bw) == t.bw and float(back.nu0) == t.nu0
    assert [list(c) for c in back.ok_ichans] == [list(c) for c in t.ok_ichans]
    assert [e.in_days() for e in back.epochs] == [e.in_days() for e in t.epochs]


@pytest.mark.parametrize("module,args", [("pptoas_run", ["-d", "x.npz", "-m", MODEL]), ("ppalign_run", ["-M", "meta.txt"]),
                                         ("ppzap_run", ["-d", "x.npz"])])
def test_older_commands_still_refuse_T_and_name_ppscrunch_run(module, args, tmp_path):
    r = subprocess.run([sys.executable, "-m", "pulseportraiture_amd." + module] + args + ["-T"], capture_output=True,
                       text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and r.stdout == ""
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith(module + ":") and "PSRCHIVE" in lines[0] and "ppscrunch_run -T" in lines[0]


class _StubGetTOAs(pptoas.GetTOAs):
    """get_TOAs with the fit replaced and the archive operations on the NumPy engine; `seen` records what the fit got."""

    def __init__(self, *a, **kw):
        pptoas.GetTOAs.__init__(self, *a, **kw)
        self.eng, self.seen = NumpyEngine(), []

    def _engine(self, distributed):
        return self.eng

    def _load_template(self, eng, slot, freqs_row, nbin, P, unscattered=False):
        pass

    def _archive_fit(self, eng, d, a, opt):
        nok, nchan = len(a.isubs), d.nchan
        self.seen.append((d.nsub, np.asarray(a.port).shape, list(a.isubs)))
        res = dict(params=np.zeros((nok, 5)), param_errs=np.full((nok, 5), 1e-4), cov=np.zeros((nok, 5, 5)),
                   nu_refs=np.full((nok, 3), 1500.0), nfeval=np.ones(nok, dtype=np.int32),
                   return_code=np.zeros(nok, dtype=np.int32), scales=np.ones((nok, nchan)),
                   scale_errs=np.ones((nok, nchan)), snr=np.ones(nok), channel_snrs=np.ones((nok, nchan)),
                   red_chi2=np.ones(nok), duration=0.1)
        res["params"][:, 1] = d.DM
        return res, 0.1, {sl: np.ones(nchan) for sl in set(a.slots.values())}


def test_get_TOAs_tscrunch_fits_one_subint_per_archive():
    def total(seed):
        d = _bunch(state="Intensity", dmc=0, seed=seed)
        d.subints = d.subints[:, :1]
        d.update(npol=1, noise_stds=d.noise_stds[:, :1], SNRs=d.SNRs[:, :1])
        return d
    archives = [total(3), total(4)]
    gt = _StubGetTOAs(archives, MODEL, quiet=True)
    gt.get_TOAs(tscrunch=True, quiet=True, seed="device")
    assert gt.seen == [(1, (1, 6, 16), [0]), (1, (1, 6, 16), [0])]
    assert len(gt.TOA_list) == 2 and [len(m) for m in gt.MJDs] == [1, 1] and gt.tscrunch
    assert archives[0].nsub == 5                                  # the caller's bunch is untouched
    gt2 = _StubGetTOAs(archives, MODEL, quiet=True)
    gt2.get_TOAs(quiet=True, seed="device")
    assert [s[0] for s in gt2.seen] == [5, 5] and len(gt2.TOA_list) == 8
    with pytest.raises(NotImplementedError):
        gt.get_TOAs(tscrunch=True, show_plot=True)


def test_good_channel_counts_of_the_scrunched_subint(tmp_path):
    d = _bunch()
    assert archive.good_channel_counts(d, tscrunch=True) == [6] and archive.good_channel_counts(d) == [5, 5, 5, 5]
    w = np.zeros((3, 5))
    w[0, 1] = w[2, 1] = w[1, 4] = 1.0
    np.savez(tmp_path / "w.npz", subints=np.zeros((3, 1, 5, 8)), weights=w)
    assert archive.good_channel_counts(str(tmp_path / "w.npz"), tscrunch=True) == [2]
    assert archive.good_channel_counts(str(tmp_path / "w.npz")) == [1, 1, 1]
    np.savez(tmp_path / "g.npz", subints=np.zeros((3, 1, 5, 8)))
    assert archive.good_channel_counts(str(tmp_path / "g.npz"), tscrunch=True) == [5]


class _ZapEngine(NumpyEngine):
    """... plus the two calls that follow a scrunched fit: the residual chi^2 per channel and the narrowband fit; both
    record what they were handed."""

    def channel_red_chi2(self, ports, freqs, P, params, nu_refs, scales, errs, slots=None):
        self.log.append(("chi2", np.array(ports), np.array(freqs), np.array(P), np.array(errs)))
        return np.ones(np.asarray(ports).shape[:2])

    def fit_phase_shift_batch(self, data, model, noise=None, bounds=(-0.5, 0.5), Ns=100, finish='newton'):
        self.log.append(("fps", np.array(data), np.array(noise)))
        out = np.zeros((len(data), 7))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = 0.25, 1e-4, 1.0, 0.1, 20.0, 1.0
        return out


def _intensity_bunch(seed, dead_first=False):
    d = _bunch(state="Intensity", dmc=0, seed=seed)
    d.subints = d.subints[:, :1]
    d.update(npol=1, noise_stds=d.noise_stds[:, :1], SNRs=d.SNRs[:, :1])
    if dead_first:
        w = d.weights.copy()
        w[0] = 0.0
        d = pptoas.data_from_arrays(d.subints, d.freqs, d.Ps, d.epochs, weights=w, noise_stds=d.noise_stds, SNRs=d.SNRs,
                                    DM=d.DM, dmc=0, doppler_factors=d.doppler_factors, bw=d.bw, nu0=d.nu0,
                                    subtimes=d.subtimes, parallactic_angles=d.parallactic_angles, filename="dead0.npz")
        d.state = "Intensity"
    return d


def test_get_channels_to_zap_after_a_scrunched_fit_takes_the_scrunched_archive():
    """Subint 0 of the raw archive is fully zapped: taking it (its frequencies, noise, good channels) for the one fitted
    subint would divide by zero; the residuals are those of the scrunched archive."""
    d = _intensity_bunch(5, dead_first=True)
    gt = _StubGetTOAs([d], MODEL, quiet=True)
    gt.eng = _ZapEngine()
    gt.get_TOAs(tscrunch=True, quiet=True, seed="device")
    gt.get_channels_to_zap(SNR_threshold=0.0, rchi2_threshold=1.3)
    want = scrunch.tscrunch(d, engine=NumpyEngine())
    calls = [c for c in gt.eng.log if c[0] == "chi2"]
    assert len(calls) == 1
    _, port, freqs, P, errs = calls[0]
    assert port.shape == (1, 6, 16) and np.array_equal(port, want.subints[:, 0])
    assert np.array_equal(freqs, want.freqs) and np.array_equal(P, want.Ps) and np.array_equal(errs, want.noise_stds[:, 0])
    assert len(gt.zap_channels) == 1 and gt.zap_channels[0] == [[]]
    assert [len(r) for r in gt.channel_red_chi2s[0]] == [len(want.ok_ichans[0])]


def test_get_narrowband_TOAs_tscrunch_fits_the_channels_of_one_subint():
    d = _intensity_bunch(6)
    gt = _StubGetTOAs([d], MODEL, quiet=True)
    gt.eng = _ZapEngine()
    gt._model_for = lambda freqs_row, nbin, P, unscattered=False: np.ones((len(freqs_row), nbin))
    gt.get_narrowband_TOAs(tscrunch=True, quiet=True)
    want = scrunch.tscrunch(d, engine=NumpyEngine())
    ich = want.ok_ichans[0]
    calls = [c for c in gt.eng.log if c[0] == "fps"]
    assert len(calls) == 1 and np.array_equal(calls[0][1], want.subints[0, 0, ich])
    assert np.array_equal(calls[0][2], want.noise_stds[0, 0, ich])
    assert len(gt.TOA_list) == len(ich) and gt.phis[0].shape == (1, 6) and gt.tscrunch
    assert all(t.flags["subint"] == 0 for t in gt.TOA_list)
    # every TOA is the scrunched subint's epoch plus the fitted phase
    toa = want.epochs[0] + MJD(0, 0.25 * want.Ps[0] / 86400.0)
    assert all(abs((t.MJD - toa).in_days()) < 1e-15 for t in gt.TOA_list)
    gt2 = _StubGetTOAs([d], MODEL, quiet=True)
    gt2.eng = _ZapEngine()
    gt2._model_for = gt._model_for
    gt2.get_narrowband_TOAs(quiet=True)
    assert len(gt2.TOA_list) == sum(len(c) for c in d.ok_ichans) and gt2.phis[0].shape == (5, 6)


def test_fscrunch_of_a_dispersed_archive_rotates_each_channel_to_its_groups_frequency():
    """One rotation call, and the rows it leaves are each channel delayed by Dconst DM (nu_c^-2 - nu_g^-2) / P."""
    eng, d = NumpyEngine(), _bunch(dmc=0)
    f = scrunch.fscrunch(d, nchan=3, engine=eng)
    assert sum(1 for c in eng.log if c[0] == "rotate") == 1
    k = np.arange(9)
    rot = np.empty_like(d.subints)
    for i in range(5):
        for c in range(6):
            delay = pplib.Dconst * d.DM * (d.freqs[i, c] ** -2.0 - f.freqs[i, c // 2] ** -2.0) / d.Ps[i]
            rot[i, :, c] = np.fft.irfft(np.fft.rfft(d.subints[i, :, c], axis=-1) * np.exp(2j * np.pi * k * delay), n=16, axis=-1)
    want, wwant, _ = sr.scrunch_ref(rot, d.weights, None, [0, 2, 4, 6], "keep")
    # (the frequency handed to the rotation rounds the delay by some 1e-14 rot here: 2 pi k dphi |X_k| < 1e-12 at k <= 8)
    assert np.allclose(f.subints, want, rtol=0, atol=1e-12) and np.array_equal(f.weights, wwant)
