"""Wavelet smoothing on the GPU against the true reference run on the PyWavelets stand-in (tests/golden/ppsmooth_*.npz,
from make_golden_ppsmooth.py).

Decisions -- level, evaluation count, zeroing -- are compared exactly; every test first asserts, through the
restatement (tests/wavelet_ref.py), that no coefficient of its input lies within 1e-9 lopt of lopt at the factors it
uses, so that no decision hangs on rounding.  The bar of the smoothed values is ten times the disagreement of the
restatement's two inverse forms (time-domain even/odd averaging against the frame adjoint) on the same input, relative
to max |row|: the device's adjoint form is one more rearrangement of that kind.  With PP_PPSMOOTH_PARITY_OUT set, both
figures of every case are written there as JSON (profiles/ppsmooth_parity.json).
"""
import os

import numpy as np
import pytest

from tests import ppsmooth_cases as sc
from tests import wavelet_ref as wr
from tests.gpu_support import default_eng, measured_writer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TIE = 1e-9
MEASURED, _write_measured = measured_writer("PP_PPSMOOTH_PARITY_OUT")


def _g(name):
    return np.load(os.path.join(GOLDEN, "ppsmooth_%s.npz" % name))


def _record(key, dev, forms):
    MEASURED[key] = dict(device_vs_reference=float(dev), inverse_forms=float(forms), bar=float(10.0 * forms))
    print("%-28s device vs reference %.3e   inverse forms %.3e   bar %.3e" % (key, dev, forms, 10.0 * forms))


@pytest.mark.parametrize("nbin,nlevel", sc.WAVELET_CASES)
def test_wavelet_smooth_matches_the_reference(nbin, nlevel):
    g = _g("wavelet")
    x = g["in_%d" % nbin]
    assert np.array_equal(x, sc.wavelet_input(nbin))
    assert wr.tie_margin(x, nlevel, [f for f in sc.FACTS if f > 0]) > TIE
    forms = float(g["forms_%d_%d" % (nbin, nlevel)])
    rows = np.tile(x, (len(sc.FACTS), 1))
    worst = 0.0
    for tt in sc.THRESHTYPES:
        got = default_eng().wavelet_smooth(rows, nlevel=nlevel, threshtype=tt, fact=np.array(sc.FACTS))
        for i, fact in enumerate(sc.FACTS):
            want = g["out_%d_%d_%s_%g" % (nbin, nlevel, tt, fact)]
            worst = max(worst, np.abs(got[i] - want).max() / np.abs(x).max())
    _record("wavelet_%d_%d" % (nbin, nlevel), worst, forms)
    assert worst <= 10.0 * forms


def _smart_forms(x, level, fact, tt):
    a = wr.wavelet_smooth(x, level, tt, fact)
    b = wr.wavelet_smooth(x, level, tt, fact, inverse=wr.iswt_adjoint)
    return np.abs(a - b).max() / np.abs(x).max()


@pytest.mark.parametrize("name", list(sc.SMART_CASES))
def test_smart_smooth_matches_the_reference(name):
    from pulseportraiture_amd import pplib
    g = _g("smart")
    x = g["in_" + name]
    assert np.array_equal(x, sc.smart_input(name))
    tt = sc.SMART_CASES[name][3]
    got, info = pplib.smart_smooth(x, rchi2_tol=0.1, return_info=True, threshtype=tt)
    level, fact, nfev = int(g["level_" + name]), float(g["fact_" + name]), int(g["nfev_" + name])
    print(name, "level", info["level"][0], level, "fact", info["fact"][0], fact, "nfev", info["nfev"][0], nfev,
          "red_chi2", info["red_chi2"][0])
    assert tt == "soft" or wr.tie_margin(x, level, [fact]) > TIE
    assert info["level"][0] == level
    assert info["nfev"][0] == nfev
    assert (not np.any(got)) == bool(g["zeroed_" + name])
    assert abs(info["fact"][0] - fact) <= 1e-12
    forms = _smart_forms(x, level, fact, tt)
    dev = np.abs(got - g["out_" + name]).max() / np.abs(x).max()
    _record("smart_" + name, dev, forms)
    assert dev <= 10.0 * forms


def test_no_candidate_passes_at_64_bins_and_the_row_comes_back_zero():
    from pulseportraiture_amd import pplib
    g = _g("smart")
    assert bool(g["zeroed_64_snr1"]) and len(g["valid_levels_64_snr1"]) == 0
    got, info = pplib.smart_smooth(g["in_64_snr1"], return_info=True)
    assert got.shape == (64,) and not np.any(got)
    assert info["snr"][0] == 0.0


def test_valid_levels_are_those_of_the_issue():
    g = _g("smart")
    assert list(g["valid_levels_256_snr30"]) == [1, 2, 3, 4, 5]
    assert list(g["valid_levels_100_snr30"]) == [1]
    # (with the continuous soft threshold the finish moves the factor off the grid)
    j = float(g["fact_256_snr30_soft"]) * 29.0 / 3.0
    assert abs(j - round(j)) > 1e-6


def test_zero_and_odd_rows():
    from pulseportraiture_amd import pplib
    g = _g("smart")
    got, info = pplib.smart_smooth(g["in_zeros"], return_info=True)
    assert np.array_equal(got, g["out_zeros"]) and not np.any(got)
    assert info["level"][0] == 0 and info["nfev"][0] == 0
    # an odd length comes back as it is -- a single profile as the one-row portrait the reference has made of it by then
    odd = g["in_odd"]
    got = pplib.smart_smooth(odd)
    assert got.shape == g["out_odd"].shape == (1, 255) and np.array_equal(got, g["out_odd"]) and np.array_equal(got[0], odd)
    port = np.tile(odd, (3, 1))
    assert pplib.smart_smooth(port) is port
    assert pplib.smart_smooth(g["in_256_snr30"], try_nlevels=0) is not None


def test_a_row_gives_the_same_bits_alone_and_in_a_batch():
    rng = np.random.default_rng(4300)
    rows = np.array([sc.profile(256, snr, 4300 + i) for i, snr in enumerate(rng.choice([1.0, 3.0, 30.0, 300.0], 38))])
    rows[5] = 0.0
    rows[11] *= 1e-6
    rows[17] = rng.standard_normal(256)
    eng = default_eng()
    all_out, all_info = eng.smart_smooth(rows, 8)
    for i in (0, 5, 11, 17, 37):
        one_out, one_info = eng.smart_smooth(rows[i:i + 1], 8)
        assert np.array_equal(one_out[0], all_out[i]), i
        for k in ("level", "fact", "snr", "red_chi2", "nfev", "raw_noise"):
            assert np.array_equal(one_info[k][0], all_info[k][i]), (i, k)
        assert np.array_equal(one_info["stats"][0], all_info["stats"][i]), i
    assert len(set(all_info["level"])) > 2         # (mixed content: more than one outcome in the batch)
    ws_all = eng.wavelet_smooth(rows, nlevel=5, fact=0.7)
    assert np.array_equal(eng.wavelet_smooth(rows[17:18], nlevel=5, fact=0.7)[0], ws_all[17])


def test_f32_and_device_tensor_input():
    import torch
    eng = default_eng()
    x32 = np.array([sc.profile(256, 30.0, 4400 + i) for i in range(3)], dtype=np.float32)
    x64 = x32.astype(np.float64)
    want = eng.wavelet_smooth(x64, nlevel=4, fact=1.0)
    assert np.array_equal(eng.wavelet_smooth(x32, nlevel=4, fact=1.0), want)
    for host in (x32, x64):
        t = torch.from_numpy(host).to("cuda")
        out = eng.wavelet_smooth(t, nlevel=4, fact=1.0)
        assert isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.is_cuda
        assert np.array_equal(out.cpu().numpy(), want)
    s_host, i_host = eng.smart_smooth(x64, 8)
    s_dev, i_dev = eng.smart_smooth(torch.from_numpy(x32).to("cuda"), 8)
    assert np.array_equal(s_dev.cpu().numpy(), s_host) and np.array_equal(i_dev["fact"], i_host["fact"])


def test_argument_checks():
    from pulseportraiture_amd.engine import EngineError
    eng = default_eng()
    x = sc.profile(256, 30.0, 1)[None]
    with pytest.raises(EngineError):
        eng.wavelet_smooth(x[:, :255], nlevel=1)                 # odd nbin
    with pytest.raises(EngineError):
        eng.wavelet_smooth(sc.profile(100, 30.0, 1)[None], nlevel=3)        # 8 does not divide 100
    with pytest.raises(EngineError):
        eng.smart_smooth(x, 9)                                  # 2^9 > 256
    with pytest.raises(EngineError):
        eng.smart_smooth(x[:, :8], 1)                           # nbin < 16
    with pytest.raises(ValueError):
        eng.wavelet_smooth(x, threshtype="garrote")
