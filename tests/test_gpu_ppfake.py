"""Simulated observations on the device: pp_fake_portraits / Engine.fake_portraits, pplib.make_fake_pulsar on top of it,
and the command line, against the reference's own composition (tests/golden/ppfake_rows.npz), the kernel's bitwise
promises, the statistics of its noise, its refusals, and the closed loop of the reference's examples/example.py.

Bars.  Parity is held to max(10 self_dev, 1e-12) of the rows' peak, self_dev being the reference's own scatter under a
reversal of the channel order (0 here: its rows do not depend on each other, so the bar is 1e-12).  The noise bars are
5-sigma sampling bounds of N = 8192 independent unit normals per moment: the mean of N of them scatters by 1 / sqrt(N),
their variance by sqrt(2 / N), and the sample correlation of two independent sets, or of a set with itself one bin on,
by 1 / sqrt(N).  All were fixed before the first run; every measured figure is printed beside its bar."""
import os

import numpy as np
import pytest

from tests import ppfake_cases as pc
from tests.gpu_support import eng, run_module  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB, NCHAN = 3, 5
PARITY_BAR = 1e-12


def _template(nchan, nbin):
    """Two Gaussians per channel, drifting and narrowing across the band, on a baseline."""
    x = (np.arange(nbin) + 0.5) / nbin
    n = np.arange(nchan)[:, None] / max(nchan - 1, 1)
    return 0.05 + np.exp(-0.5 * ((x[None] - 0.4 - 0.05 * n) / (0.03 - 0.01 * n)) ** 2) \
        + 0.4 * np.exp(-0.5 * ((x[None] - 0.62) / 0.05) ** 2) * (1.0 + n)


def _fake(eng, shape, delays, dtype=np.float64, **kw):
    import torch
    dst = torch.full(shape, float("nan"), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0")
    eng.fake_portraits(dst, delays, **kw)
    return dst.cpu().numpy()


# =====================================================================================================
# make_fake_pulsar against the reference's composition
# =====================================================================================================
@pytest.mark.parametrize("name", pc.NAMES)
def test_make_fake_pulsar_gives_the_reference_rows(eng, tmp_path, name):
    from pulseportraiture_amd.pplib import make_fake_pulsar
    case = pc.cases()[name]
    modelfile = tmp_path / "case.gmodel"
    modelfile.write_text(case["gmodel"])
    d = make_fake_pulsar(str(modelfile), pc.PARFILE, outfile=None, nsub=2, npol=2, noise_stds=0.0, quiet=True, seed=1,
                         dtype=np.float64, engine=eng, **case["kwargs"])
    want = case["rows"]
    assert d.subints.shape == (2, 2) + want.shape and d.subints.dtype == np.float64
    assert d.dmc == (1 if case["kwargs"].get("dedispersed") else 0) and d.DM == 34.56789
    dev = max(np.abs(d.subints[i, p] - want).max() for i in range(2) for p in range(2)) / np.abs(want).max()
    print("%s: dev %.3e of the peak, bar %.1e" % (name, dev, case["bar"]))
    assert dev <= case["bar"]


# =====================================================================================================
# the kernel's edges
# =====================================================================================================
_edge_cache = {}


def _edge(eng, npol, nbin):
    """One set of calls per (npol, nbin), shared by the edge tests: inputs and the f64 outputs with noise, without, and
    with the template switched off."""
    key = (npol, nbin)
    if key not in _edge_cache:
        rng = np.random.default_rng(100 * nbin + npol)
        eng.set_model(_template(NCHAN, nbin), slot=0)
        shape = (NSUB, npol, NCHAN, nbin)
        delays = rng.uniform(-0.7, 0.7, (NSUB, NCHAN))
        amps = rng.uniform(0.3, 2.0, (NSUB, npol, NCHAN))
        sigmas = np.array([0.5, 0.0, 1.0, 0.0, 2.0])       # two channels without noise
        kw = dict(seed=20260101, first_subint=5)
        c = dict(shape=shape, delays=delays, amps=amps, sigmas=sigmas, kw=kw)
        c["noisy"] = _fake(eng, shape, delays, amps=amps, sigmas=sigmas, **kw)
        c["clean"] = _fake(eng, shape, delays, amps=amps, **kw)
        for a in (c["noisy"], c["clean"]):
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _edge_cache.clear()           # (the slot holds this row length's template now)
        _edge_cache[key] = c
    else:
        eng.set_model(_template(NCHAN, nbin), slot=0)
    return _edge_cache[key]


EDGES = [(npol, nbin) for nbin in (32, 100, 2048) for npol in (1, 4)]


@pytest.mark.parametrize("npol,nbin", EDGES)
def test_f32_rows_are_the_rounded_f64_rows(eng, npol, nbin):
    c = _edge(eng, npol, nbin)
    f32 = _fake(eng, c["shape"], c["delays"], dtype=np.float32, amps=c["amps"], sigmas=c["sigmas"], **c["kw"])
    assert f32.dtype == np.float32 and f32.tobytes() == c["noisy"].astype(np.float32).tobytes()
    # [nsub, nchan, nbin] is npol = 1
    if npol == 1:
        flat = _fake(eng, (NSUB, NCHAN, nbin), c["delays"], amps=c["amps"], sigmas=c["sigmas"], **c["kw"])
        assert flat.tobytes() == c["noisy"].tobytes()


@pytest.mark.parametrize("npol,nbin", EDGES)
def test_zero_sigma_rows_are_the_noise_free_rows(eng, npol, nbin):
    c = _edge(eng, npol, nbin)
    quiet = c["sigmas"] == 0.0
    assert c["noisy"][:, :, quiet].tobytes() == c["clean"][:, :, quiet].tobytes()
    assert not np.array_equal(c["noisy"][:, :, ~quiet], c["clean"][:, :, ~quiet])
    zeros = _fake(eng, c["shape"], c["delays"], amps=c["amps"], sigmas=np.zeros(NCHAN), **c["kw"])
    assert zeros.tobytes() == c["clean"].tobytes()
    # amps None is an amplitude of one
    ones = _fake(eng, c["shape"], c["delays"], amps=np.ones_like(c["amps"]), **c["kw"])
    none = _fake(eng, c["shape"], c["delays"], **c["kw"])
    assert ones.tobytes() == none.tobytes()


@pytest.mark.parametrize("npol,nbin", EDGES)
def test_zero_amplitude_rows_are_sigma_times_the_deviates(eng, npol, nbin):
    c = _edge(eng, npol, nbin)
    off = np.zeros_like(c["amps"])
    z = _fake(eng, c["shape"], c["delays"], amps=off, sigmas=np.ones(NCHAN), **c["kw"])
    got = _fake(eng, c["shape"], c["delays"], amps=off, sigmas=c["sigmas"], **c["kw"])
    assert np.isfinite(z).all() and np.array_equal(got, c["sigmas"][None, None, :, None] * z)
    assert not got[:, :, c["sigmas"] == 0.0].any()
    # ... and they are what the noisy rows carry on top of the noise-free ones, to the rounding of one fma
    resid = c["noisy"] - c["clean"] - got
    assert np.abs(resid).max() <= 2.0 ** -51 * np.abs(c["noisy"]).max()
    # no two polarisations, channels or subints share deviates
    flat = z.reshape(-1, nbin)
    assert len(np.unique(flat[:, :8], axis=0)) == len(flat)


@pytest.mark.parametrize("npol,nbin", EDGES)
def test_a_subint_does_not_depend_on_how_the_call_is_cut(eng, npol, nbin):
    c = _edge(eng, npol, nbin)
    for i in range(NSUB):
        one = _fake(eng, (1,) + c["shape"][1:], c["delays"][i:i + 1], amps=c["amps"][i:i + 1], sigmas=c["sigmas"],
                    seed=c["kw"]["seed"], first_subint=c["kw"]["first_subint"] + i)
        assert one[0].tobytes() == c["noisy"][i].tobytes(), i
    other = _fake(eng, c["shape"], c["delays"], amps=c["amps"], sigmas=c["sigmas"], seed=c["kw"]["seed"] + 1, first_subint=5)
    assert not np.array_equal(other[:, :, 0], c["noisy"][:, :, 0])


@pytest.mark.parametrize("npol,nbin", EDGES)
def test_a_delay_of_one_bin_is_a_roll(eng, npol, nbin):
    _edge(eng, npol, nbin)
    shape = (NSUB, npol, NCHAN, nbin)
    still = _fake(eng, shape, np.zeros((NSUB, NCHAN)))
    bins = np.array([1, -3, nbin + 2])[:, None] * np.ones((1, NCHAN))        # per subint
    moved = _fake(eng, shape, bins / nbin)
    want = _template(NCHAN, nbin)
    peak = np.abs(want).max()
    dev0 = np.abs(still - want[None, None]).max() / peak
    dev = max(np.abs(moved[i] - np.roll(still[i], int(bins[i, 0]), axis=-1)).max() for i in range(NSUB)) / peak
    print("nbin %d npol %d: zero delay %.3e, whole-bin delays %.3e of the peak, bar %.1e" % (nbin, npol, dev0, dev, PARITY_BAR))
    assert dev0 <= PARITY_BAR and dev <= PARITY_BAR


@pytest.mark.parametrize("nbin", [32, 100])
def test_an_archive_does_not_depend_on_the_chunk_size(eng, tmp_path, monkeypatch, nbin):
    from pulseportraiture_amd import pplib
    from pulseportraiture_amd.archive import load_bunch as _load
    out = []
    for chunk in (1, 3, None):
        monkeypatch.setattr(pplib, "fake_chunk_subints", chunk)
        name = str(tmp_path / ("chunk%s.npz" % chunk))
        d = pplib.make_fake_pulsar(pc.GMODEL, pc.PARFILE, outfile=name, nsub=3, npol=2, nchan=NCHAN, nbin=nbin, tsub=60.0,
                                   phase=0.1, dDM=1e-3, noise_stds=0.3, scint=True, quiet=True, seed=11, engine=eng)
        back, _ = _load(name)
        assert back.subints.dtype == np.float32 and back.subints.tobytes() == d.subints.tobytes()
        assert back.dmc == 0 and back.DM == 34.56789 and back.nu0 == 1500.0 and back.bw == 800.0 and back.source == "J1234-5678"
        assert np.array_equal(back.Ps, np.full(3, 1.0 / 345.67890123456789)) and np.array_equal(back.subtimes, np.full(3, 60.0))
        np.testing.assert_allclose([e.in_days() for e in back.epochs], 50000.0 + (30.0 + 60.0 * np.arange(3)) / 86400.0,
                                   rtol=0, atol=1e-11)
        out.append(d.subints)
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes()
    assert np.isfinite(out[0]).all() and out[0].std() > 0.1


# =====================================================================================================
# the noise
# =====================================================================================================
def test_noise_moments_and_independence(eng):
    nsub, npol, nchan, nbin = 4, 2, 8, 2048
    N = nsub * nbin
    assert N == 8192
    eng.set_model(_template(nchan, nbin), slot=0)
    rng = np.random.default_rng(3)
    delays = rng.uniform(-0.5, 0.5, (nsub, nchan))
    amps = rng.uniform(0.5, 1.5, (nsub, npol, nchan))
    sigmas = np.linspace(0.5, 4.0, nchan)
    kw = dict(amps=amps, seed=987654321, first_subint=0)
    noisy = _fake(eng, (nsub, npol, nchan, nbin), delays, sigmas=sigmas, **kw)
    clean = _fake(eng, (nsub, npol, nchan, nbin), delays, **kw)
    z = (noisy - clean) / sigmas[None, None, :, None]         # unit deviates [nsub][npol][nchan][nbin]
    per = z.transpose(2, 1, 0, 3).reshape(nchan, npol, N)     # N samples per (channel, polarisation)
    mean, var = per.mean(-1), per.var(-1)
    b_mean, b_var, b_corr = 5.0 / np.sqrt(N), 5.0 * np.sqrt(2.0 / N), 5.0 / np.sqrt(N)
    lag1 = (z[..., 1:] * z[..., :-1]).sum((0, 3)).T / N                          # [nchan][npol]
    pol = (z[:, 0] * z[:, 1]).sum((0, 2)) / N                                    # [nchan]
    sub = (z[1:] * z[:-1]).sum((0, 3)).T / N                                     # [nchan][npol], 3 nbin products
    chan = (z[:, :, 1:] * z[:, :, :-1]).sum((0, 3)).T / N                        # [nchan - 1][npol]
    print("noise: |mean| %.3e (bar %.3e)  |var - 1| %.3e (bar %.3e)" % (np.abs(mean).max(), b_mean, np.abs(var - 1).max(), b_var))
    print("noise: lag-1 %.3e  pol 0-1 %.3e  subint i,i+1 %.3e  channel n,n+1 %.3e (bar %.3e)" %
          (np.abs(lag1).max(), np.abs(pol).max(), np.abs(sub).max(), np.abs(chan).max(), b_corr))
    assert np.abs(mean).max() <= b_mean          # (z is in units of sigma_n)
    assert np.abs(var - 1.0).max() <= b_var
    for c in (lag1, pol, sub, chan):
        assert np.abs(c).max() <= b_corr


# =====================================================================================================
# misuse
# =====================================================================================================
def test_misuse_is_refused_not_faulted():
    """An unset slot, npol < 1, null delays, negative or NaN sigmas, a delay that is not finite, a destination of the
    wrong size or on the host: refused on the host before anything is launched; the engine works on afterwards."""
    import ctypes as C
    import torch
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import Engine, EngineError
    e = Engine(0)
    try:
        nbin = 64
        shape = (2, 2, NCHAN, nbin)
        dst = torch.zeros(shape, dtype=torch.float64, device="cuda:0")
        delays = np.zeros((2, NCHAN))
        with pytest.raises(EngineError, match="not set"):
            e.fake_portraits(dst, delays)
        e.set_model(_template(NCHAN, nbin), slot=0)
        with pytest.raises(EngineError, match="not set"):
            e.fake_portraits(dst, delays, slot=7)
        lib, ptr = e._lib, C.c_void_p(dst.data_ptr())
        dp = delays.ctypes.data_as(_lib.c_double_p)
        assert lib.pp_fake_portraits(e._ctx, 7, ptr, _lib.PP_F64, 2, 2, dp, None, None, 1, 0) == _lib.PP_ESTATE
        assert lib.pp_fake_portraits(e._ctx, _lib.PP_MAX_SLOTS, ptr, _lib.PP_F64, 2, 2, dp, None, None, 1, 0) == _lib.PP_ESTATE
        for npol in (0, -1, 65537):
            assert lib.pp_fake_portraits(e._ctx, 0, ptr, _lib.PP_F64, 2, npol, dp, None, None, 1, 0) == _lib.PP_EINVAL
        assert lib.pp_fake_portraits(e._ctx, 0, ptr, _lib.PP_F64, 0, 2, dp, None, None, 1, 0) == _lib.PP_EINVAL
        assert lib.pp_fake_portraits(e._ctx, 0, ptr, _lib.PP_F64, 2, 2, None, None, None, 1, 0) == _lib.PP_EINVAL
        assert lib.pp_fake_portraits(e._ctx, 0, None, _lib.PP_F64, 2, 2, dp, None, None, 1, 0) == _lib.PP_EINVAL
        assert lib.pp_fake_portraits(e._ctx, 0, ptr, 7, 2, 2, dp, None, None, 1, 0) == _lib.PP_EINVAL
        assert "null" in _lib.last_error() or "dtype" in _lib.last_error()
        with pytest.raises(EngineError, match="delays"):
            e.fake_portraits(dst, None)
        for bad in (-1.0, np.nan, np.inf):
            s = np.ones(NCHAN)
            s[3] = bad
            with pytest.raises(EngineError, match="sigmas"):
                e.fake_portraits(dst, delays, sigmas=s)
            d = delays.copy()
            d[1, 2] = bad if bad != -1.0 else -np.inf
            with pytest.raises(EngineError, match="delays"):
                e.fake_portraits(dst, d)
        for wrong in ((2, 2, NCHAN, nbin // 2), (2, 2, NCHAN + 1, nbin), (2, 2, NCHAN - 1, nbin), (2, NCHAN, 2 * nbin),
                      (NCHAN, nbin), (2, 2, 2, NCHAN, nbin)):
            with pytest.raises(EngineError, match="dst"):
                e.fake_portraits(torch.zeros(wrong, dtype=torch.float64, device="cuda:0"), np.zeros((2, wrong[-2])))
        with pytest.raises(EngineError, match="CUDA"):
            e.fake_portraits(np.zeros(shape), delays)
        with pytest.raises(EngineError, match="CUDA"):
            e.fake_portraits(torch.zeros(shape, dtype=torch.float64), delays)
        with pytest.raises(EngineError, match="float"):
            e.fake_portraits(torch.zeros(shape, dtype=torch.int32, device="cuda:0"), delays)
        with pytest.raises(EngineError, match="contiguous"):
            e.fake_portraits(torch.zeros((2, 2, NCHAN, 2 * nbin), dtype=torch.float64, device="cuda:0")[..., ::2], delays)
        with pytest.raises(ValueError):
            e.fake_portraits(dst, np.zeros((3, NCHAN)))
        with pytest.raises(ValueError):
            e.fake_portraits(dst, delays, amps=np.ones((2, 3, NCHAN)))
        assert not dst.cpu().numpy().any()         # nothing was written by a refused call
        e.fake_portraits(dst, delays)
        got = dst.cpu().numpy()
        want = _template(NCHAN, nbin)
        assert np.abs(got - want[None, None]).max() <= PARITY_BAR * np.abs(want).max()
    finally:
        e.close()


# =====================================================================================================
# the closed loop of the reference's example, commands in child processes
# =====================================================================================================
def _flag(line, key):
    parts = line.split()
    return float(parts[parts.index(key) + 1])


DDMS = [6e-4, -6e-4, 0.0]
PHASE = 0.05


@pytest.mark.parametrize("leg", ["dispersed", "dedispersed", "npol4_scint"])
def test_the_examples_closed_loop(tmp_path, leg):
    """ppfake_run -> pptoas_run at 3 files x 2 subints x 16 channels x 256 bins from example.gmodel and example.par: six
    TOAs; every archive's Delta-DM and every TOA's phase (at its printed reference frequency) within 5 sigma of the
    injected ones by the reported errors.  The third leg (four polarisations, random scintillation) loads and fits."""
    from pulseportraiture_amd.gmodel import gaussian_portrait, read_gmodel
    from pulseportraiture_amd.parfile import psr_par
    from pulseportraiture_amd.pplib import Dconst
    par = psr_par(pc.PARFILE)
    freqs = np.linspace(1100.0 + 25.0, 1900.0 - 25.0, 16)
    peak = gaussian_portrait(read_gmodel(pc.GMODEL), freqs, 256, par.P0).max()
    args = ["-m", pc.GMODEL, "-e", pc.PARFILE, "-o", "fake-%d.npz", "--nfiles", "3", "--nsub", "2", "--nchan", "16",
            "--nbin", "256", "--dDM", ",".join("%g" % v for v in DDMS), "--phase", "%g" % PHASE, "--noise_std",
            "%.6g" % (0.02 * peak), "--seed", "4", "--metafile", "list.txt", "--quiet"]
    args += {"dispersed": [], "dedispersed": ["--dedispersed"], "npol4_scint": ["--npol", "4", "--scint"]}[leg]
    out = run_module("ppfake_run", args, tmp_path, 120)
    lines = [ln for ln in out.splitlines() if "dDM" in ln]
    assert [ln.split()[0] for ln in lines] == ["fake-1.npz", "fake-2.npz", "fake-3.npz"], out
    assert [float(ln.split()[-1]) for ln in lines] == DDMS
    assert (tmp_path / "list.txt").read_text().split() == ["fake-1.npz", "fake-2.npz", "fake-3.npz"]
    out = run_module("pptoas_run", ["-d", "list.txt", "-m", pc.GMODEL, "--DM", "34.56789", "--print_phase", "--quiet"],
                     tmp_path, 120)
    toas = [ln for ln in out.splitlines() if "-pp_dm " in ln]
    assert len(toas) == 6, out
    if leg == "npol4_scint":
        with np.load(str(tmp_path / "fake-1.npz")) as z:
            assert z["subints"].shape == (2, 4, 16, 256) and z["subints"].dtype == np.float32
        return
    dm = np.array([_flag(ln, "-pp_dm") for ln in toas]).reshape(3, 2)
    dme = np.array([_flag(ln, "-pp_dme") for ln in toas]).reshape(3, 2)
    phs = np.array([_flag(ln, "-phs") for ln in toas]).reshape(3, 2)
    phe = np.array([_flag(ln, "-phs_err") for ln in toas]).reshape(3, 2)
    nu = np.array([float(ln.split()[1]) for ln in toas]).reshape(3, 2)
    for ia in range(3):
        got, sigma = dm[ia].mean() - 34.56789, 0.5 * np.sqrt((dme[ia] ** 2).sum())
        print("%s file %d: Delta-DM %.3e (injected %.1e), sigma %.1e" % (leg, ia + 1, got, DDMS[ia], sigma))
        assert abs(got - DDMS[ia]) < 5.0 * sigma
        # the injected delay at the TOA's reference frequency: phase is given at nu0, the DMs disperse about nu0
        want = PHASE + Dconst * (34.56789 + DDMS[ia]) / par.P0 * (nu[ia] ** -2.0 - 1500.0 ** -2.0)
        diff = (phs[ia] - want + 0.5) % 1.0 - 0.5
        print("%s file %d: phase off by %s, sigma %s" % (leg, ia + 1, diff, phe[ia]))
        assert (np.abs(diff) < 5.0 * phe[ia]).all()
