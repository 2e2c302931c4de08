"""The 'fit' noise method on the device (pp_noisefit.h) against the NumPy restatement of tests/noisefit_refs.py
(pinned to the true reference's fixture in tests/test_noisefit_cpu.py) and against the fixture itself.

Bars.  kc and the winning cell are compared as integers, exactly, for every row whose margin -- how far the
reference's own choice of width is from a toss-up (noisefit_refs) -- is at least 1e-9; another summation order
moves a chi-squared by ~1e-13 of itself.  At most 2 % of a test's rows may fall below that, each test prints how
many did, and the seeds were chosen so that none do (tests/test_noisefit_cpu.py checks that without a GPU).  Noise,
norms and S/N: the suite's bars, relative and nothing else -- rtol 1e-12 for f64 input and 1e-5 for f32, atol 0 -- for
every row that has a value to compare.  Only where the expected value itself is below that rtol times the row's rms
is the device's value held to that absolute floor instead: the transform leaves rounding residue of ~1e-16 of the row
in harmonics that hold nothing, and a noise made of that residue alone (a constant row; exactly 0 for a row of zeros,
whose floor is 0) has no digits to compare.

One kind of row has no integer answer to compare: a constant row at a row length without a tuned plan.  All its
power above DC is rounding residue.  The reference's transform happens to leave exact zeros among it (log10 = -inf:
cell 0), the chirp transform leaves ~1e-32 everywhere, and the fit of either is a fit to rounding.  There the noise
is held to the absolute floor above and norm and S/N to their bars; at the tuned lengths the device's residue is
exactly zero too and the row is compared like any other.

With PP_NOISEFIT_PARITY_OUT set, every measured deviation is written there beside its bar as JSON
(profiles/noisefit_parity.json)."""
import functools
import os

import numpy as np
import pytest

from tests import aux_refs as ar
from tests import noisefit_refs as nf
from tests.gpu_support import default_eng, measured_writer

pytestmark = pytest.mark.gpu

MEASURED, _write_measured = measured_writer("PP_NOISEFIT_PARITY_OUT")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = np.load(os.path.join(GOLDEN, "noisefit.npz"))

# every plan the row kernel instantiates up to 4096 bins (nbin 32 ... 4096), and both ends of the any-even path
LENGTHS = nf.TEST_LENGTHS
NPULSE = nf.TEST_NPULSE
CONSTANT = NPULSE + nf.SPECIAL.index("constant")
RTOL = {"f64": 1e-12, "f32": 1e-5}


def _tuned(nbin):
    return nbin >= 32 and nbin & (nbin - 1) == 0


def _rec(section, key, deviation, bar):
    deviation, bar = float(deviation), float(bar)
    MEASURED.setdefault(section, {})[key] = dict(deviation=deviation, bar=bar,
                                                 of_bar=deviation / bar if bar > 0 else (0.0 if deviation == 0 else float("inf")))
    print("%-30s %-40s dev %.3e  bar %.3e" % (section, key, deviation, bar))


@functools.lru_cache(maxsize=None)
def _rows(nbin):
    """NPULSE pulses and the special rows, every value a float32: the f64 and the f32 input are the same numbers."""
    return nf.test_rows(nbin)


@functools.lru_cache(maxsize=None)
def _want(nbin, fn):
    """The restatement of _rows(nbin), computed once: (noise, kc, cell, margin)."""
    return nf.noise_fit_rows(_rows(nbin), fn=fn)


def _as_input(rows, dtype, place):
    x = np.ascontiguousarray(rows, dtype=np.float64 if dtype == "f64" else np.float32)
    if place == "device":
        import torch
        return torch.as_tensor(x, device="cuda")
    return x


def _dev(got, want, rows, rtol, label):
    """The largest relative deviation |got - want| / |want| over the rows that have a value to compare (the caller
    holds it to rtol).  Rows whose expected value is no larger than rtol rms(row) -- rounding residue, or exactly 0 --
    are held to that floor here, in absolute terms."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    floor = rtol * np.sqrt(np.mean(np.asarray(rows, dtype=np.float64) ** 2, axis=-1))
    small = np.abs(want) <= floor
    assert (np.abs(got[small]) <= floor[small]).all(), (label, got[small], floor[small])
    if small.all():
        return 0.0
    return float(np.max(np.abs(got[~small] - want[~small]) / np.abs(want[~small])))


def _compare(got, nbin, fn, idx, dtype, label):
    """got = (noise, kc, cell) of rows _rows(nbin)[idx] against the restatement."""
    noise, kc, cell, margin = (v[idx] for v in _want(nbin, fn))
    rows = _rows(nbin)[idx]
    residue = np.zeros(len(idx), dtype=bool) if _tuned(nbin) else (np.asarray(idx) == CONSTANT)
    low = (margin < nf.MARGIN_MIN) & ~residue
    print("%s: %d of %d rows below the margin" % (label, low.sum(), len(idx)))
    assert low.sum() <= 0.02 * len(idx), margin[low]
    cmp_ = ~low & ~residue
    np.testing.assert_array_equal(got[1][cmp_], kc[cmp_], err_msg=label)
    np.testing.assert_array_equal(got[2][cmp_], cell[cmp_], err_msg=label)
    dev = _dev(got[0][cmp_], noise[cmp_], rows[cmp_], RTOL[dtype], label)
    _rec("noise", label, dev, RTOL[dtype])
    assert dev <= RTOL[dtype], (label, got[0][cmp_], noise[cmp_])
    if residue.any():
        floor = RTOL[dtype] * np.sqrt(np.mean(rows[residue] ** 2, axis=-1))
        assert (got[0][residue] >= 0.0).all() and (got[0][residue] <= floor).all(), (label, got[0][residue], floor)


# =====================================================================================================
# the row kernel and its twin, called directly
# =====================================================================================================
@pytest.mark.parametrize("fn", nf.FNS)
@pytest.mark.parametrize("nbin", LENGTHS)
def test_rows_at_every_plan(nbin, fn):
    """3 rows and 700 (every row of _rows, over and over), f64 and f32, host and device input; the special rows are
    among the 700.  (700 rows are more than one pass of a workgroup over its rows only where the grid is smaller,
    at 4096 bins; test_a_workgroup_walks_several_rows takes the other kernels through their loops.)"""
    eng = default_eng()
    nrow = len(_rows(nbin))
    for dtype in ("f64", "f32"):
        for place in ("host", "device"):
            for idx in (np.arange(NPULSE), np.arange(700) % nrow):
                got = eng.noise_fit(_as_input(_rows(nbin)[idx], dtype, place), fn=fn)
                assert got[1].dtype == np.int32 and got[2].shape == (len(idx), 3)
                _compare(got, nbin, fn, idx, dtype, "nbin %d %s %s %s x%d" % (nbin, fn, dtype, place, len(idx)))


@pytest.mark.parametrize("nbin", LENGTHS)
def test_special_rows(nbin):
    """What the special rows pin, beyond equality with the restatement."""
    H = nbin // 2 + 1
    at = {name: NPULSE + i for i, name in enumerate(nf.SPECIAL)}
    noise, kc, cell = default_eng().noise_fit(_rows(nbin))
    for name in ("zeros", "zero_sum_int") + (("constant",) if _tuned(nbin) else ()):
        assert kc[at[name]] == H - 1 and tuple(cell[at[name]]) == (0, 0, 0), (name, kc[at[name]], cell[at[name]])
    assert noise[at["zeros"]] == 0.0
    assert tuple(cell[at["b0"]][:2]) == (0, 0) and tuple(_want(nbin, "exp_dc")[2][at["b0"]][:2]) == (0, 0)
    assert np.isfinite(noise).all()


@pytest.mark.parametrize("nbin", [256, 100])
def test_a_row_does_not_depend_on_its_batch(nbin):
    eng = default_eng()
    idx = np.arange(700) % len(_rows(nbin))
    for dtype in ("f64", "f32"):
        rows = _as_input(_rows(nbin)[idx], dtype, "host")
        for fn in nf.FNS:
            many, one = eng.noise_fit(rows, fn=fn), eng.noise_fit(rows[5:6], fn=fn)
            for a, b in zip(many, one):
                np.testing.assert_array_equal(a[5:6], b)
        a = eng.channel_noise(rows, norm='rms', method='fit')
        b = eng.channel_noise(rows[5:6], norm='rms', method='fit')
        np.testing.assert_array_equal(a[0][5:6], b[0])
        np.testing.assert_array_equal(a[1][5:6], b[1])


@pytest.mark.parametrize("nbin", [64, 100, 4096])
def test_a_workgroup_walks_several_rows(nbin):
    """4500 rows: more than the 2048 workgroups the twin and the power-spectrum entry launch, and more than the
    resident grid of a tuned plan, so every workgroup's loop runs again over the LDS the row before left.  Each row's
    bits are those of the same row in a call of its own."""
    eng = default_eng()
    rows = _rows(nbin)
    idx = (np.arange(4500) * 5) % len(rows)
    for fn in nf.FNS:
        alone = eng.noise_fit(rows, fn=fn)
        many = eng.noise_fit(np.ascontiguousarray(rows[idx]), fn=fn)
        for a, b in zip(many, alone):
            np.testing.assert_array_equal(a, b[idx])
    pows = np.array([nf.power_spectrum(r) for r in rows])
    alone = eng.find_kc(pows, return_cell=True, return_noise=True)
    many = eng.find_kc(np.ascontiguousarray(pows[idx]), return_cell=True, return_noise=True)
    for a, b in zip(many, alone):
        np.testing.assert_array_equal(a, b[idx])


def test_bad_arguments_are_refused():
    from pulseportraiture_amd.engine import EngineError
    eng = default_eng()
    x = _rows(64)
    with pytest.raises(ValueError):
        eng.channel_noise(x, method='median')
    with pytest.raises(ValueError):
        eng.channel_noise(x, method='fit', fn='gauss')
    with pytest.raises(EngineError):
        eng.channel_noise(x, method='fit', fact=-1.0)
    with pytest.raises(EngineError):
        eng.noise_fit(np.zeros((2, 4098)))
    with pytest.raises(ValueError):
        eng.find_kc(np.ones((2, 4)))


# =====================================================================================================
# the power-spectrum entry: find_kc itself
# =====================================================================================================
def test_find_kc_of_constructed_spectra():
    eng = default_eng()
    H = 1025
    a20, kc20 = nf.width_table(H, "exp_dc")
    k = np.arange(H)
    # an exact exponential on a grid point: exp(-a k) is 0 from k = 746 on, so min(data) = dc (idc = 0), max - min = b
    # (ib = 19), and a is the last width
    exact = 10.0 ** (-2.0 + 3.0 * np.exp(-a20[19] * k))
    flat = np.full(H, 2.5)                      # max = min: every b is 0, all 8000 cells tie
    hole = nf.power_spectrum(_rows(2048)[0])
    hole[300] = 0.0                             # one harmonic of no power
    pows = np.array([exact, flat, hole])
    assert nf.find_kc_full(exact)["cell"] == (19, 19, 0) and nf.find_kc_full(flat)["cell"] == (0, 0, 0)
    for place in ("host", "device"):
        kc, cell, noise = eng.find_kc(_as_input(pows, "f64", place), return_cell=True, return_noise=True)
        np.testing.assert_array_equal(cell, [(19, 19, 0), (0, 0, 0), (0, 0, 0)])
        np.testing.assert_array_equal(kc, [kc20[19], H - 1, H - 1])
        want = [nf.tail_noise(p, c) for p, c in zip(pows, kc)]
        np.testing.assert_allclose(noise, want, rtol=1e-12, atol=0.0)
    kc_tri, cell_tri = eng.find_kc(pows[1:], fn='half_tri', return_cell=True)
    np.testing.assert_array_equal(cell_tri, [(0, 0, 0), (0, 0, 0)])
    np.testing.assert_array_equal(kc_tri, [1, 1])


@pytest.mark.parametrize("H", nf.TEST_SPECTRA_H)
def test_find_kc_of_spectra_equals_the_restatement(H):
    """Any H from 5 to 2049 (odd and even: the spectrum entry has no row length behind it), both fn."""
    pows = nf.test_spectra(H)
    eng = default_eng()
    for fn in nf.FNS:
        want = [nf.find_kc_full(p, fn) for p in pows]
        margin = np.array([w["margin"] for w in want])
        ok = margin >= nf.MARGIN_MIN
        print("H %d %s: %d of %d rows below the margin" % (H, fn, (~ok).sum(), len(ok)))
        assert ok.all(), margin
        kc, cell = eng.find_kc(pows, fn=fn, return_cell=True)
        np.testing.assert_array_equal(kc, [w["kc"] for w in want])
        np.testing.assert_array_equal(cell, [w["cell"] for w in want])
    from pulseportraiture_amd import pplib
    assert pplib.find_kc(pows[0]) == nf.find_kc_full(pows[0])["kc"]
    assert pplib.find_kc(pows[0], errs=2.0, fn='half_tri') == nf.find_kc_full(pows[0], 'half_tri')["kc"]


# =====================================================================================================
# end to end
# =====================================================================================================
@pytest.mark.parametrize("nbin", nf.LENGTHS_FIXTURE)
def test_get_noise_fit_equals_the_reference(nbin):
    """pplib.get_noise(x, method='fit'), get_noise_fit(x) and get_noise_fit(port, chans=True) against the TRUE
    reference's values (on the parent commit get_noise printed 'Unknown get_noise method.' and returned 0)."""
    from pulseportraiture_amd import pplib
    rows = FIX["rows_%d" % nbin]
    got_get = np.array([pplib.get_noise(r, method='fit') for r in rows])
    got_1d = np.array([pplib.get_noise_fit(r) for r in rows])
    got_chans = pplib.get_noise_fit(rows, chans=True)
    for name, got, key in (("get_noise", got_get, "noise_get_%d"), ("get_noise_fit", got_1d, "noise_1d_%d"),
                           ("chans=True", got_chans, "noise_chans_%d")):
        dev = _dev(got, FIX[key % nbin], rows, 1e-12, name)
        _rec("fixture", "%s nbin %d" % (name, nbin), dev, 1e-12)
        assert dev <= 1e-12, (name, got, FIX[key % nbin])
    np.testing.assert_array_equal(got_get, got_1d)
    np.testing.assert_array_equal(got_get, got_chans)
    # the fitted cut-off itself, through the engine (the constant row of a length without a tuned plan: see above)
    noise, kc, cell = default_eng().noise_fit(rows)
    keep = np.ones(len(rows), dtype=bool)
    keep[8 + nf.SPECIAL.index("constant")] = _tuned(nbin)
    np.testing.assert_array_equal(kc[keep], FIX["kc_exp_dc_%d" % nbin][keep])
    np.testing.assert_array_equal(cell[keep], FIX["cell_exp_dc_%d" % nbin][keep])
    # a ravelled 2-D input is one transform
    two = rows[:2, :32] if nbin == 64 else rows[:2]
    want = nf.noise_fit_row(two.ravel())
    if want["margin"] >= nf.MARGIN_MIN:
        np.testing.assert_allclose(pplib.get_noise_fit(two), want["noise"], rtol=1e-12)


@pytest.mark.parametrize("nbin", [64, 100, 2048])
def test_engine_norms_and_snrs_with_the_fitted_noise(nbin):
    eng = default_eng()
    rows = _rows(nbin)
    noise, kc, cell, margin = _want(nbin, "exp_dc")
    live = rows.any(axis=1)
    keep = np.ones(len(rows), dtype=bool)
    keep[CONSTANT] = _tuned(nbin)
    for dtype in ("f64", "f32"):
        rtol = RTOL[dtype]
        x = _as_input(rows, dtype, "host")
        got_noise, got_norms = eng.channel_noise(x, norm='rms', method='fit')
        want_norms = np.where(live, noise, 1.0)
        dev = _dev(got_norms[keep & live], want_norms[keep & live], rows[keep & live], rtol, "rms norms")
        _rec("norms", "rms nbin %d %s" % (nbin, dtype), dev, rtol)
        assert dev <= rtol
        np.testing.assert_array_equal(got_norms[~live], 1.0)
        # noise / |norm|: 1 where there is noise, 0 for the rows without a sample
        np.testing.assert_allclose(got_noise[keep & live & (noise > 0)], 1.0, rtol=rtol)
        np.testing.assert_array_equal(got_noise[~live], 0.0)
        for norm, val in (("mean", rows.mean(axis=1)), ("max", rows.max(axis=1)), ("abs", np.sqrt((rows ** 2).sum(axis=1))),
                          (None, np.ones(len(rows)))):
            g_noise, g_norms = eng.channel_noise(x, norm=norm, method='fit')
            val = np.where(live, val, 1.0)
            np.testing.assert_allclose(g_norms, val, rtol=rtol)
            sel = keep & (val != 0.0)
            safe = np.abs(np.where(val == 0.0, 1.0, val))
            dev = _dev(g_noise[sel], (noise / safe)[sel], (rows / safe[:, None])[sel], rtol, str(norm))
            _rec("norms", "%s nbin %d %s" % (norm, nbin, dtype), dev, rtol)
            assert dev <= rtol, (norm, g_noise, noise / np.abs(val))
        # S/N: rows with noise to divide by
        sel = keep & live & (noise > 1e-9)
        got_snr = eng.channel_snrs(x, method='fit')
        want_snr = np.array([nf.snr_row(r, n) for r, n in zip(rows[sel], noise[sel])])
        np.testing.assert_allclose(got_snr[sel], want_snr, rtol=rtol, atol=0.0)
        _rec("snrs", "nbin %d %s" % (nbin, dtype), np.max(np.abs(got_snr[sel] - want_snr) / np.maximum(np.abs(want_snr), 1e-300)), rtol)
        # and the default is still the power-spectrum estimate
        np.testing.assert_array_equal(eng.channel_snrs(x), eng.channel_snrs(x, method='PS'))
        np.testing.assert_array_equal(eng.channel_noise(x)[0], eng.channel_noise(x, method='PS')[0])


def _bunch(nsub=4, nchan=16, nbin=64, loud=(3, 11), seed=99):
    """A tiny archive: pulses on unit noise, two channels ten times as noisy."""
    from pulseportraiture_amd.archive import data_from_arrays
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    prof = 30.0 * np.exp(-0.5 * ((ph - 0.4) / (0.05 / 2.355)) ** 2)
    sigma = np.ones(nchan)
    sigma[list(loud)] = 10.0
    sub = nf.f32_exact(prof[None, None, None, :] + rng.normal(0.0, 1.0, (nsub, 1, nchan, nbin)) * sigma[None, None, :, None])
    return data_from_arrays(sub, np.linspace(1200.0, 1600.0, nchan), np.full(nsub, 0.005), np.arange(nsub) + 55000.0), sub


def test_load_data_measures_with_the_chosen_method():
    from pulseportraiture_amd import pplib
    bunch, sub = _bunch()
    eng = default_eng()
    direct = eng.channel_noise(sub.reshape(-1, sub.shape[-1]), method='fit')[0].reshape(sub.shape[:-1])
    snrs = eng.channel_snrs(sub.reshape(-1, sub.shape[-1]), method='fit').reshape(sub.shape[:-1])
    d = pplib.load_data(bunch, noise_method='fit', quiet=True)
    np.testing.assert_array_equal(d.noise_stds, direct)
    np.testing.assert_array_equal(d.SNRs, np.nan_to_num(snrs, nan=0.0))
    # stored values give way to a chosen method, and stay without one
    stored = pplib.DataBunch(**dict(bunch, noise_stds=np.full(sub.shape[:-1], 7.0), SNRs=np.full(sub.shape[:-1], 3.0)))
    np.testing.assert_array_equal(pplib.load_data(stored, noise_method='fit', quiet=True).noise_stds, direct)
    np.testing.assert_array_equal(pplib.load_data(stored, quiet=True).noise_stds, 7.0)
    ps = pplib.load_data(bunch, quiet=True).noise_stds
    np.testing.assert_array_equal(ps, eng.channel_noise(sub.reshape(-1, sub.shape[-1]))[0].reshape(sub.shape[:-1]))
    assert not np.array_equal(ps, direct)
    assert pplib.get_SNR(sub[0, 0, 0], noise_method='fit') == snrs[0, 0, 0]


def test_ppzap_run_with_the_fitted_noise(tmp_path, monkeypatch, capsys):
    """ppzap_run --noise_method fit prints the paz commands of the restatement's zap lists."""
    from pulseportraiture_amd import ppzap_run
    bunch, sub = _bunch()
    np.savez(tmp_path / "tiny.npz", subints=sub, freqs=bunch.freqs, Ps=bunch.Ps, epochs=np.arange(4) + 55000.0,
             noise_stds=np.ones(sub.shape[:-1]), SNRs=np.ones(sub.shape[:-1]))       # (stored noise must not win)
    monkeypatch.chdir(tmp_path)
    noise = np.array([[nf.noise_fit_row(r)["noise"] for r in s[0]] for s in sub])
    margins = np.array([[nf.noise_fit_row(r)["margin"] for r in s[0]] for s in sub])
    assert (margins >= nf.MARGIN_MIN).all()
    lines = ["paz -e zap tiny.npz"]
    for isub in range(len(sub)):
        zap, rounds, margin = ar.clip(noise[isub], np.ones(sub.shape[2], dtype=bool), 3.0)
        assert margin >= 1e-9
        assert set(np.nonzero(zap)[0]) and set(np.nonzero(zap)[0]) <= {3, 11}
        lines += ["paz -m -I -z %d -w %d tiny.zap" % (n, isub) for n in np.nonzero(zap)[0]]
    assert ppzap_run.main(["-d", "tiny.npz", "-n", "3", "--noise_method", "fit", "--quiet"]) == 0
    assert capsys.readouterr().out.splitlines() == lines
    # without the option the stored noise (all ones) decides: nothing to zap
    assert ppzap_run.main(["-d", "tiny.npz", "-n", "3", "--quiet"]) == 0
    assert "paz -m" not in capsys.readouterr().out
