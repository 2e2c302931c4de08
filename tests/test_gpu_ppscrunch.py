"""pp_scrunch / Engine.scrunch on the device against the sequential restatement of tests/scrunch_refs.py, its bitwise
promises and its refusals; then the callers: get_TOAs(tscrunch=True), ppscrunch_run -T | pptoas_run, and
align_archives(tscrunch=True).

Bars.  Samples: per element (n + 2) 2^-53 sum|w x| / sum w, n the cell's member count -- a sequential f64 sum of n
products and one division under any contraction of its multiply-adds, nothing more; the test works it out from its own
inputs.  Total weights, the identity and the four ways of cutting a call up: bit for bit.  Callers: phi within 1e-9
rot and DM within the same relative bar (the README's caller-level parity bar), TOA strings identical."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import scrunch_refs as sr
from tests.gpu_support import eng, run_module  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB, NCHAN = 5, 6
T_OFF, F_OFF = [0, 3, 5], [0, 1, 4, 6]
POLS = [(1, "keep"), (1, "first"), (2, "keep"), (2, "sum01"), (2, "first"), (4, "keep"), (4, "sum01"), (4, "first")]


_inputs = {}


def _case(npol, nbin):
    """ports[5,npol,6,nbin] (f64; the f32 cases use its rounding), weights with zeros, one NaN and a negative one, one
    output cell -- time group 1, channel group 0 -- of zero total weight, and NaN samples in every row that is skipped."""
    key = (npol, nbin)
    if key not in _inputs:
        rng = np.random.default_rng(7 * nbin + npol)
        x = rng.normal(size=(NSUB, npol, NCHAN, nbin)) + 0.3
        w = rng.uniform(0.5, 2.0, size=(NSUB, NCHAN))
        w[0, 2] = w[1, 5] = w[2, 1] = w[4, 4] = 0.0
        w[3, 0] = w[4, 0] = 0.0          # the dead cell
        w[1, 3] = np.nan
        w[2, 4] = -0.25
        for s in range(NSUB):
            for c in range(NCHAN):
                if not sr.live(w[s, c]):
                    x[s, :, c] = np.nan
        _inputs[key] = (x, w)
    return _inputs[key]


_refs = {}


def _ref(npol, nbin, pol_mode, dtype):
    key = (npol, nbin, pol_mode, dtype)
    if key not in _refs:
        x, w = _case(npol, nbin)
        _refs[key] = sr.scrunch_ref(x.astype(dtype), w, T_OFF, F_OFF, pol_mode)
    return _refs[key]


# ---- case 1: against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nbin", [8, 102, 4096])
@pytest.mark.parametrize("npol,pol_mode", POLS)
def test_scrunch_matches_the_sequential_sum(eng, npol, pol_mode, nbin, dtype):
    x, w = _case(npol, nbin)
    want, wwant, bound = _ref(npol, nbin, pol_mode, dtype)
    out, wout = eng.scrunch(x.astype(dtype), w, T_OFF, F_OFF, pol_mode)
    assert out.shape == want.shape and out.dtype == np.float64
    assert not np.isnan(out).any() and not np.isnan(wout).any()
    assert np.array_equal(wout, wwant)
    assert wout[1, 0] == 0.0 and not out[1, :, 0].any()
    excess = np.abs(out - want) - bound
    print("max |out - ref| %.3e, largest excess over the bound %.3e" % (np.abs(out - want).max(), excess.max()))
    assert (excess <= 0.0).all()


# ---- case 2: identity -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nbin", [8, 102, 4096])
def test_singleton_groups_of_weight_one_return_the_input(eng, nbin, dtype):
    x = np.random.default_rng(nbin).normal(size=(NSUB, 2, NCHAN, nbin)).astype(dtype)
    out, wout = eng.scrunch(x, np.ones((NSUB, NCHAN)))
    assert np.array_equal(out, x.astype(np.float64)) and np.array_equal(wout, np.ones((NSUB, NCHAN)))


# ---- case 3: the bits do not depend on how the call is cut up ---------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nbin", [102, 4096])
@pytest.mark.parametrize("npol,pol_mode", [(2, "keep"), (2, "sum01")])
def test_scrunch_bits_do_not_depend_on_runs_device_or_other_groups(eng, npol, pol_mode, nbin, dtype):
    import torch
    x, w = _case(npol, nbin)
    x = x.astype(dtype)
    one, wone = eng.scrunch(x, w, T_OFF, F_OFF, pol_mode)
    # runs of two subints: [0, 1] [2, 3] [4] -- both time groups straddle a run boundary
    npo = npol if pol_mode == "keep" else 1
    per_sub = npol * NCHAN * nbin * x.itemsize + npo * (len(F_OFF) - 1) * nbin * 8 + 24 * NCHAN
    with eng.options(max_work_bytes=2.5 * per_sub):
        cut, wcut = eng.scrunch(x, w, T_OFF, F_OFF, pol_mode)
    assert np.array_equal(cut, one) and np.array_equal(wcut, wone)
    dev, wdev = eng.scrunch(torch.from_numpy(x).to("cuda:0"), w, T_OFF, F_OFF, pol_mode)
    assert dev.is_cuda and dev.dtype == torch.float64
    assert np.array_equal(dev.cpu().numpy(), one) and np.array_equal(wdev, wone)
    # time group 0, channel group 1 in a call of its own
    own, wown = eng.scrunch(x[0:3, :, 1:4], w[0:3, 1:4], [0, 3], [0, 3], pol_mode)
    assert np.array_equal(own[0, :, 0], one[0, :, 1]) and wown[0, 0] == wone[0, 1]


# ---- case 4: refusals -------------------------------------------------------------------------------
def test_scrunch_refusals_launch_nothing_and_leave_the_context_usable(eng):
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import EngineError
    x, w = _case(2, 8)
    good = eng.scrunch(x, w, T_OFF, F_OFF, "sum01")[0]
    for t_off, f_off in (([1, 3, 5], F_OFF), ([0, 3, 3, 5], F_OFF), ([0, 3, 4], F_OFF), ([0, 3, 6], F_OFF),
                         (T_OFF, [0, 4, 1, 6]), (T_OFF, [0, 1, 4, 7])):
        with pytest.raises(EngineError, match="off must ascend"):
            eng.scrunch(x, w, t_off, f_off)
    with pytest.raises(EngineError, match="two polarisations"):
        eng.scrunch(x[:, :1], w, T_OFF, F_OFF, "sum01")
    with pytest.raises(EngineError, match="nbin"):
        eng.scrunch(np.zeros((NSUB, 1, NCHAN, 9)), w)
    lib = eng._lib
    x64 = np.ascontiguousarray(x)
    out, wout = np.full((2, 2, 3, 8), 7.0), np.full((2, 3), 7.0)
    to = np.asarray(T_OFF, dtype=np.int32)
    fo = np.asarray(F_OFF, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    args = lambda **kw: [kw.get(k, v) for k, v in (
        ("ctx", eng._ctx), ("src", C.c_void_p(x64.ctypes.data)), ("dtype", _lib.PP_F64), ("dev", 0), ("nsub", NSUB),
        ("npol", 2), ("nchan", NCHAN), ("nbin", 8), ("w", dp(w)), ("ngt", 2), ("t", ip(to)), ("ngf", 3), ("f", ip(fo)),
        ("mode", 0), ("dst", C.c_void_p(out.ctypes.data)), ("wout", dp(wout)))]
    for bad in (dict(src=None), dict(w=None), dict(t=None), dict(f=None), dict(dst=None), dict(wout=None), dict(dtype=2),
                dict(mode=3), dict(nsub=0), dict(ngt=0)):
        assert lib.pp_scrunch(*args(**bad)) == _lib.PP_EINVAL, bad
    assert (out == 7.0).all() and (wout == 7.0).all()          # nothing was written
    assert lib.pp_scrunch(*args()) == 0
    assert np.array_equal(eng.scrunch(x, w, T_OFF, F_OFF, "sum01")[0], good)


# ---- cases 5 and 6: the callers ---------------------------------------------------------------------
GMODEL = os.path.join(ROOT, "tests", "golden", "example.gmodel")
PARFILE = os.path.join(ROOT, "tests", "golden", "example.par")
NU_REF = 1500.0


def _scrunched_by_the_test(eng, d):
    """The DataBunch of archive d scrunched to one subint with nothing of the product's scrunch module: the samples by
    the sequential restatement, the bookkeeping by the rules the issue states, written out here -- subtimes add, Ps and
    doppler factors are means weighted by the subints' summed weights, freqs the weighted-mean frequencies (the plain mean
    where the weight is 0), the epoch a whole number of periods from the good member nearest the weighted-mean epoch --
    and noise and S/N measured on the device from the rows (they set the fit's weights and frequencies).  Returns
    (bunch, anchor subint)."""
    from pulseportraiture_amd import pptoas
    w = np.asarray(d.weights, dtype=np.float64)
    nsub, nchan = w.shape
    out, wout, _ = sr.scrunch_ref(np.asarray(d.subints), w, [0, nsub], None, "keep")
    Ws = w.sum(axis=1)
    good = [s for s in range(nsub) if Ws[s] > 0]
    mean = lambda x: float(sum(Ws[s] * x[s] for s in good) / sum(Ws[s] for s in good))
    freqs = np.array([[(w[:, c] * d.freqs[:, c]).sum() / w[:, c].sum() if w[:, c].sum() > 0 else d.freqs[:, c].mean()
                       for c in range(nchan)]])
    P = mean(d.Ps)
    ebar = d.epochs[0] + pptoas.MJD(0, mean([(e - d.epochs[0]).in_days() for e in d.epochs]))
    anchor = min(good, key=lambda s: abs((d.epochs[s] - ebar).in_days()))
    k = np.round((ebar - d.epochs[anchor]).in_days() * 86400.0 / P)
    epoch = d.epochs[anchor] + pptoas.MJD(0, float(k * P / 86400.0))
    rows = out.reshape(-1, out.shape[-1])
    bunch = pptoas.data_from_arrays(
        out, freqs, [P], [epoch], weights=wout, noise_stds=eng.channel_noise(rows)[0].reshape(out.shape[:3]),
        SNRs=np.nan_to_num(eng.channel_snrs(rows)).reshape(out.shape[:3]), DM=d.DM, dmc=d.dmc,
        doppler_factors=[mean(d.doppler_factors)], backend_delay=d.backend_delay, telescope=d.telescope,
        telescope_code=d.telescope_code, backend=d.backend, frontend=d.frontend, bw=d.bw, nu0=d.nu0,
        subtimes=[float(np.sum(d.subtimes))], parallactic_angles=[mean(d.parallactic_angles)], source=d.source,
        filename="scrunched_by_the_test")
    return bunch, anchor


def _fake_archive(path, seed):
    """nsub 4 x nchan 16 x nbin 128 from example.gmodel: channels 2, 9, 10 zapped, subint 1 zapped, noise 1e-4 of the peak."""
    from pulseportraiture_amd.engine import default_engine
    from pulseportraiture_amd.gmodel import gaussian_portrait, read_gmodel
    from pulseportraiture_amd.parfile import psr_par
    from pulseportraiture_amd.pplib import make_fake_pulsar
    w = np.ones((4, 16))
    w[:, [2, 9, 10]] = 0.0
    w[1] = 0.0
    w[0, 5] = 0.0
    w[2] *= 0.5
    peak = gaussian_portrait(read_gmodel(GMODEL), np.linspace(1125.0, 1875.0, 16), 128, psr_par(PARFILE).P0).max()
    make_fake_pulsar(GMODEL, PARFILE, outfile=str(path), nsub=4, nchan=16, nbin=128, weights=w, noise_stds=1e-4 * peak,
                     seed=seed, quiet=True, engine=default_engine())
    return str(path)


def _mjd_string(line):
    return line.split()[2]


def _periods_apart(a, b, P):
    d = a - b
    return (d.intday() * 86400.0 + d.fracday() * 86400.0) / P


def test_get_TOAs_tscrunch_end_to_end(tmp_path):
    from pulseportraiture_amd import archive, pptoas, scrunch
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    name = _fake_archive(tmp_path / "fake.npz", seed=11)
    kw = dict(quiet=True, nu_refs=(NU_REF, None))
    gt = pptoas.GetTOAs([name], GMODEL, quiet=True)
    gt.get_TOAs(tscrunch=True, **kw)
    assert len(gt.TOA_list) == 1 and len(gt.phis[0]) == 1
    # the same archive scrunched by the sequential restatement, through the path that was there before
    d, _ = archive.load_bunch(name)
    ref, anchor = _scrunched_by_the_test(eng, d)
    own = scrunch.tscrunch(d, engine=eng)
    # the product's bookkeeping against the test's
    # (two ways of writing the same weighted means may round differently: two units in the last place, and for the epoch
    # the 1e-16 d the MJD class's fraction resolves, ten times over)
    ulp2 = dict(rtol=2.0 ** -51, atol=0.0)
    assert abs((own.epochs[0] - ref.epochs[0]).in_days()) <= 1e-15 and np.isclose(own.Ps[0], ref.Ps[0], **ulp2)
    assert np.allclose(own.freqs, ref.freqs, **ulp2) and np.isclose(own.doppler_factors[0], ref.doppler_factors[0], **ulp2)
    assert np.array_equal(own.weights, ref.weights) and own.subtimes[0] == ref.subtimes[0]
    assert list(own.ok_ichans[0]) == list(ref.ok_ichans[0]) and list(own.ok_isubs) == list(ref.ok_isubs) == [0]
    gr = pptoas.GetTOAs([ref], GMODEL, quiet=True)
    gr.get_TOAs(**kw)
    dphi = abs(gt.phis[0][0] - gr.phis[0][0])
    dDM = abs(gt.DMs[0][0] - gr.DMs[0][0]) / abs(gr.DMs[0][0])
    print("|dphi| %.3e rot, |dDM| / DM %.3e (bars 1e-9)" % (dphi, dDM))
    assert dphi <= 1e-9 and dDM <= 1e-9
    assert _mjd_string(pptoas.toa_string(gt.TOA_list[0])) == _mjd_string(pptoas.toa_string(gr.TOA_list[0]))
    # a whole number of periods from the anchor subint's own TOA
    g0 = pptoas.GetTOAs([name], GMODEL, quiet=True)
    g0.get_TOAs(**kw)
    P = float(ref.Ps[0])
    tol = 3.0 * np.spacing(d.epochs[anchor].in_days()) * 86400.0 / P
    turns = _periods_apart(gt.TOAs[0][0], g0.TOAs[0][anchor], P)
    print("anchor subint %d: %.9f periods apart, tolerance %.3e" % (anchor, turns, tol))
    assert abs(turns - np.round(turns)) <= tol and np.round(turns) != 0
    # ... and through the commands, in child processes
    run_module("ppscrunch_run", ["-d", name, "-T", "--quiet"], tmp_path, 120)
    scr = str(tmp_path / "fake.scr.npz")
    assert os.path.exists(scr)
    out = run_module("pptoas_run", ["-d", scr, "-m", GMODEL, "--nu_ref", "%g" % NU_REF, "--quiet"], tmp_path, 120)
    lines = [ln for ln in out.splitlines() if "-pp_dm " in ln]
    assert len(lines) == 1, out
    day, frac = _mjd_string(lines[0]).split(".")
    turns = _periods_apart(pptoas.MJD(int(day), float("0." + frac)), g0.TOAs[0][anchor], P)
    print("commands: %.9f periods apart, tolerance %.3e" % (turns, tol))
    assert abs(turns - np.round(turns)) <= tol and np.round(turns) != 0
    parts = lines[0].split()
    assert abs(float(parts[parts.index("-pp_dm") + 1]) - gr.DMs[0][0]) <= 1e-7 + 1e-9 * abs(gr.DMs[0][0])      # (%.7f)


def test_align_archives_tscrunch_equals_prescrunched_copies(tmp_path):
    from pulseportraiture_amd import archive, ppalign, scrunch
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    names = [_fake_archive(tmp_path / ("fake%d.npz" % i), seed=20 + i) for i in range(2)]
    got, gotw = ppalign.align_archives(names, names[0], tscrunch=True, outfile=str(tmp_path / "a.npz"), quiet=True, engine=eng)
    copies = [scrunch.tscrunch(archive.load_archive(n, eng)[0], engine=eng) for n in names]
    assert all(c.nsub == 1 for c in copies)
    want, wantw = ppalign.align_archives(copies, names[0], outfile=str(tmp_path / "b.npz"), quiet=True, engine=eng)
    assert np.array_equal(got, want) and np.array_equal(gotw, wantw) and got.any()


def test_archive_operations_on_host_arrays_and_device_tensors_agree(tmp_path):
    """Every archive operation on a dispersed two-polarisation archive, from host subints and from a device tensor: the
    same kernels in the same order, so the same bits; and load_data's fully scrunched profile is the restatement's."""
    import torch
    from pulseportraiture_amd import archive, pplib, ppalign, scrunch
    from pulseportraiture_amd.engine import default_engine
    from pulseportraiture_amd.pplib import DataBunch, make_fake_pulsar
    eng = default_engine()
    w = np.ones((4, 16))
    w[:, [2, 9]] = 0.0
    w[1] = 0.0
    name = str(tmp_path / "coh.npz")
    make_fake_pulsar(GMODEL, PARFILE, outfile=name, nsub=4, npol=2, nchan=16, nbin=128, weights=w, noise_stds=0.01,
                     state="Coherence", seed=5, quiet=True, engine=eng)
    host, _ = archive.load_archive(name, eng)
    host.state = "Coherence"
    dev = DataBunch(**{k: v for k, v in host.items()})
    dev.subints = torch.from_numpy(np.ascontiguousarray(host.subints)).to("cuda:0")
    ops = (lambda d: scrunch.tscrunch(d, nsub=2, engine=eng), lambda d: scrunch.fscrunch(d, nchan=4, engine=eng),
           lambda d: scrunch.pscrunch(d, engine=eng), lambda d: scrunch.dedisperse(d, engine=eng),
           lambda d: scrunch.fscrunch(scrunch.dedisperse(d, engine=eng), engine=eng),
           lambda d: pplib.load_data(d, dedisperse=True, tscrunch=True, pscrunch=True, fscrunch=True, quiet=True, engine=eng))
    for i, op in enumerate(ops):
        a, b = op(host), op(dev)
        assert isinstance(a.subints, np.ndarray) and b.subints.is_cuda, i
        assert a.subints.shape == (a.nsub, a.npol, a.nchan, a.nbin)
        assert np.array_equal(a.subints, b.subints.cpu().numpy()), i
        for k in ("weights", "freqs", "noise_stds", "SNRs", "Ps"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (i, k)
    assert dev.subints.shape == (4, 2, 16, 128) and np.array_equal(dev.subints.cpu().numpy(), host.subints)   # untouched
    # the profile of the fully scrunched archive against the restatement applied to the dedispersed rows
    ded = scrunch.dedisperse(host, engine=eng)
    want, wwant, bound = sr.scrunch_ref(ded.subints, host.weights, [0, 4], [0, 16], "sum01")
    full = ops[-1](host)
    # (three sums in a row -- time 3 members, polarisation 1, frequency 14 -- against one of 42: their bounds, (n + 2) 2^-53
    # each on the same sum of |w x|, add up to less than the one sum's, and the restatement has that error itself: twice it)
    assert full.subints.shape == (1, 1, 1, 128)
    excess = np.abs(full.prof - want[0, 0, 0]) - 2.0 * bound[0, 0, 0]
    print("profile: max |prof - ref| %.3e, largest excess over twice the bound %.3e" % (np.abs(full.prof - want[0, 0, 0]).max(), excess.max()))
    assert (excess <= 0.0).all()
