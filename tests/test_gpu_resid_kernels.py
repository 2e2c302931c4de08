"""Engine.fit_residuals (pp_resid.h: k_resid, k_resid_harm) called directly at every row plan -- nbin 32, 64, 1024, 2048,
8192 -- and both ends of the chirp-z classes -- 8, 62, 250, 1026 --, 2 subints x 3 channels, against the plain
references of tests/resid_refs.py (which tests/test_resid_cpu.py pins to the reference's show_fit): long double for the
rows resid_refs.ld_rows picks, the f64 restatement for every row.

Bars (none is taken from the device's output)
  rows      rot_bar(nbin) x (max |data row| + |a_n| max |model row|): port and model are each a rounding-level transform
            of their own row (rot_refs.rot_bar is the project's bar of one rotation), resid carries both.  f32 input:
            plus 2^-24 of the same scale, the one rounding of the store.
  resid     against port - model of the same call: twice that bar.
  red_chi2  equal to the last bit to Engine.channel_red_chi2 on the same inputs; rtol 1e-10 against chan_red_chi2_ld
            (the bar tests/test_gpu_rot_kernels.py holds that kernel to).
  DM = 80   a last-place difference of the f64 phi_n (26 - 40 turns) costs the highest harmonic 2 pi M u, u = 8 x 2^-53 x
            the summed absolute terms of phi_n: added to the bar, as test_gpu_rot_kernels.py does under the delay law.
  the rest  zero tolerance (bits).
With PP_RESID_PARITY_OUT set, every measured deviation is written there beside its bar
(profiles/resid_kernels_parity.json)."""
import math

import numpy as np
import pytest

from tests import resid_refs as rf
from tests import rot_refs as rr
from tests.gpu_support import eng, measured_writer  # noqa: F401

pytestmark = pytest.mark.gpu

MEASURED, _write_measured = measured_writer("PP_RESID_PARITY_OUT")
LD = np.longdouble
DTYPES = [np.float64, np.float32]
ROWS = ("port", "model", "resid")
ALL4 = ROWS + ("red_chi2",)


def _record(kind, tag, dev, bar, **extra):
    """The worst deviation of a case beside its bar; printed before anything is asserted."""
    of = float(dev / bar) if bar > 0 else (0.0 if dev == 0 else math.inf)
    e = MEASURED.setdefault(kind, {}).get(tag)
    if e is None or of >= e["of_bar"]:
        MEASURED[kind][tag] = dict(deviation=float(dev), bar=float(bar), of_bar=of, **extra)
    print(kind, tag, "deviation %.3e, bar %.3e: %.3f of the bar" % (dev, bar, of), extra or "")


def _tag(nbin, dtype, *more):
    return "-".join([str(nbin), np.dtype(dtype).name] + [str(m) for m in more])


def _bar(nbin, dtype, scale):
    return (rr.rot_bar(nbin) + (2.0 ** -24 if dtype == np.float32 else 0.0)) * scale


def _hold(kind, tag, got, want, bar):
    """Rows got[..., nbin] within bar[...] (absolute, per row) of want; records the worst row."""
    dev = np.abs(got.astype(LD) - np.asarray(want, dtype=LD)).max(axis=-1).astype(np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), dev.shape)
    ratio = dev / bar
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
    _record(kind, tag, float(dev[w]), float(bar[w]))
    assert np.all(np.isfinite(got))
    assert np.all(dev <= bar), (kind, tag, float(ratio.max()))


def _set_templates(eng, tm):
    with eng.options(harm_eps=0.0):          # every harmonic kept: the Nyquist term of the model matters
        for s in range(len(tm)):
            assert eng.set_model(tm[s], slot=s) >= tm.shape[-1] // 2


def _call(eng, c, dtype=np.float64, frame="model", want=ALL4, subs=slice(None), data=None, **kw):
    data = c["data"] if data is None else data
    args = dict(errs=c["sigma"][subs], slots=c["slots"][subs], frame=frame, want=want)
    args.update(kw)
    return eng.fit_residuals(data[subs].astype(dtype), c["freqs"][subs], c["P"][subs], c["params"][subs],
                             c["nu_refs"][subs], c["scales"][subs], **args)


def _bits(a):
    return (a.cpu().numpy() if hasattr(a, "is_cuda") else a).tobytes()


# ==== every row plan ===========================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", rf.FRAMES)
@pytest.mark.parametrize("nbin", rf.POW2 + rf.ANY)
def test_rows_and_chi2_at_every_row_plan(eng, nbin, frame, dtype):
    """port, model and resid of two fitted subints (phi + DM on one template; phi + DM + tau, alpha on the other;
    per-subint frequency rows, a negative scale) against the references; resid against port - model; red_chi2 bitwise
    against channel_red_chi2 and to rtol 1e-10 against the long-double time-domain sum."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    got = _call(eng, c, dtype, frame)
    full, ld = rf.reference(nbin, frame)
    bar = _bar(nbin, dtype, rf.scale_of(c))
    tag = _tag(nbin, dtype, frame)
    for w in ROWS:
        assert got[w].dtype == dtype and got[w].shape == c["data"].shape
        for p, ref in ld.items():
            _hold(w + " long double", tag, got[w][p], ref[w], bar[p])
        _hold(w + " f64", tag, got[w], full[w], bar)
    _hold("resid vs port - model", tag, got["resid"], got["port"].astype(LD) - got["model"].astype(LD), 2 * bar)
    chi2 = eng.channel_red_chi2(c["data"].astype(dtype), c["freqs"], c["P"], c["params"], c["nu_refs"], c["scales"],
                                c["sigma"], slots=c["slots"])
    assert got["red_chi2"].dtype == np.float64
    differ = int((got["red_chi2"] != chi2).sum())
    _record("red_chi2 vs channel_red_chi2 (rows that differ)", tag, differ, 0)
    assert got["red_chi2"].tobytes() == chi2.tobytes()
    for p, v in rr.b1_reference(nbin).items():
        if p[0] in rf.SUBS and p[1] < rf.NCHAN:
            q = (rf.SUBS.index(p[0]), p[1])
            _record("red_chi2 long double", tag, abs(got["red_chi2"][q] - float(v)) / float(v), 1e-10)
            np.testing.assert_allclose(got["red_chi2"][q], float(v), rtol=1e-10)


# ==== edge cases ===============================================================================================
EDGE = [64, 2048, 250]       # a one-wave plan, a multi-wave plan, the chirp-z route


@pytest.mark.parametrize("nbin", EDGE)
def test_tau_zero_next_to_tau_in_one_call_with_a_slot_per_subint(eng, nbin):
    """The case itself holds tau = 0 on slot 1 next to tau != 0 on slot 0; with the slots swapped both subints
    change, with tau removed only the scattered subint's model does -- and it is then the unscattered template."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    got = _call(eng, c, want=("model",))["model"]
    swapped = dict(c, slots=c["slots"][::-1])
    other = _call(eng, swapped, want=("model",))["model"]
    assert not np.array_equal(got[0], other[0]) and not np.array_equal(got[1], other[1])
    p0 = c["params"].copy()
    p0[:, 3] = 0.0
    plain = _call(eng, dict(c, params=p0), want=("model",))["model"]
    assert plain[0].tobytes() == got[0].tobytes() and not np.array_equal(plain[1], got[1])
    want = c["scales"][1][:, None] * c["templates"][c["slots"][1]]
    _hold("tau = 0: the scaled template", _tag(nbin, np.float64), plain[1], want, _bar(nbin, np.float64, rf.scale_of(c)[1]))


@pytest.mark.parametrize("nbin", EDGE)
def test_freqs_stride_0_and_nchan(eng, nbin):
    """One frequency row for all subints (stride 0) gives the bits of the same row repeated per subint (stride nchan)."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    one = dict(c, freqs=c["freqs"][0])
    rep = dict(c, freqs=np.tile(c["freqs"][0], (rf.NSUB, 1)))
    a, b = _call(eng, one), _call(eng, rep)
    for w in ALL4:
        assert a[w].tobytes() == b[w].tobytes(), w
    assert not np.array_equal(a["port"][1], _call(eng, c)["port"][1])       # (subint 1 has another row in the case)


@pytest.mark.parametrize("nbin", EDGE)
def test_infinite_reference_frequencies(eng, nbin):
    """nu_DM = nu_GM = inf: phi_n = phi + Dconst DM nu^-2 / P, against the f64 restatement at that delay."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    refs = c["nu_refs"].copy()
    refs[:, :2] = np.inf
    params = c["params"].copy()
    params[:, 1] *= 1e-2                 # (keeps phi_n small: the delay is no longer taken relative to the band)
    phin = np.array([[float(rr.delay_ld(params[i, 0], params[i, 1], params[i, 2], c["freqs"][i, n], np.inf, np.inf,
                                        c["P"][i])) for n in range(rf.NCHAN)] for i in range(rf.NSUB)])
    got = _call(eng, dict(c, nu_refs=refs, params=params), want=ROWS)
    full = rf.portrait_f64(c["data"], c["templates"], c["slots"], phin, c["taun"], c["scales"], "model")
    for w in ROWS:
        _hold(w + " infinite nu_DM, nu_GM", _tag(nbin, np.float64), got[w], full[w], _bar(nbin, np.float64, rf.scale_of(c)))


@pytest.mark.parametrize("nbin", [2048, 8192, 1026])
def test_large_dispersive_delay(eng, nbin):
    """A DM that was never taken out -- 80 pc cm^-3 at 3 - 5 ms, phi_n 26 - 40 turns, k phi_n up to 10^5 turns at 8192
    bins --: the phasors' k phi_n mod 1 must be exact.  The bar carries 2 pi M u for the last place of the f64 phi_n."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    params = c["params"].copy()
    params[:, 1] = 80.0
    refs = c["nu_refs"].copy()
    refs[:, 0] = np.inf
    phin, u = np.empty((rf.NSUB, rf.NCHAN)), np.empty((rf.NSUB, rf.NCHAN))
    for i in range(rf.NSUB):
        for n in range(rf.NCHAN):
            t = rr.delay_terms_ld(params[i, 0], params[i, 1], params[i, 2], c["freqs"][i, n], np.inf, refs[i, 1], c["P"][i])
            phin[i, n] = float(t[0] + (t[1] + t[2]) + (t[3] + t[4]))
            u[i, n] = 8 * 2.0 ** -53 * float(sum(abs(v) for v in t))
    assert np.abs(phin).min() * (nbin // 2) > (1e5 if nbin == 8192 else 1e4)
    scale = rf.scale_of(c)
    bar = (rr.rot_bar(nbin) + 2 * np.pi * (nbin // 2) * u) * scale
    for frame in rf.FRAMES:
        got = _call(eng, dict(c, nu_refs=refs, params=params), frame=frame, want=ROWS)
        full = rf.portrait_f64(c["data"], c["templates"], c["slots"], phin, c["taun"], c["scales"], frame)
        for w in ROWS:
            _hold(w + " DM = 80", _tag(nbin, np.float64, frame), got[w], full[w], bar)


@pytest.mark.parametrize("nbin", EDGE)
def test_scale_zero(eng, nbin):
    """A channel of scale 0: its model row is zero, its resid row is its port row, bit for bit."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    sc = c["scales"].copy()
    sc[1, 1] = 0.0
    got = _call(eng, dict(c, scales=sc))
    assert not got["model"][1, 1].any()
    assert got["resid"][1, 1].tobytes() == got["port"][1, 1].tobytes()
    assert np.isfinite(got["red_chi2"]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", EDGE)
def test_masked_rows(eng, nbin, dtype):
    """Rows of weight 0 and NaN: zeros out, chi^2 NaN, and NaN-filled data there change nothing anywhere."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    mask = np.ones((rf.NSUB, rf.NCHAN))
    mask[0, 1], mask[1, 2] = 0.0, np.nan
    dead = ~(mask == 1.0)
    clean = _call(eng, c, dtype, mask=mask)
    poisoned = c["data"].copy()
    poisoned[dead] = np.nan
    got = _call(eng, c, dtype, mask=mask, data=poisoned)
    free = _call(eng, c, dtype)
    for w in ROWS:
        assert not got[w][dead].any() and np.isfinite(got[w]).all(), w
        assert got[w].tobytes() == clean[w].tobytes(), w
        assert got[w][~dead].tobytes() == free[w][~dead].tobytes(), w
    assert np.isnan(got["red_chi2"][dead]).all()
    assert got["red_chi2"][~dead].tobytes() == free["red_chi2"][~dead].tobytes()


@pytest.mark.parametrize("frame", rf.FRAMES)
@pytest.mark.parametrize("nbin", EDGE)
def test_each_output_alone_has_the_bits_of_all_four(eng, nbin, frame):
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    everything = _call(eng, c, frame=frame)
    for w in ALL4:
        alone = _call(eng, c, frame=frame, want=(w,))
        assert list(alone) == [w]
        assert alone[w].tobytes() == everything[w].tobytes(), w
    # ... and the chi^2 is one figure in both frames
    assert everything["red_chi2"].tobytes() == _call(eng, c, frame=rf.FRAMES[1 - rf.FRAMES.index(frame)],
                                                     want=("red_chi2",))["red_chi2"].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", EDGE)
def test_host_input_in_runs_has_the_bits_of_one_run(eng, nbin, dtype):
    """max_work_bytes small enough for one subint per run."""
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    mask = np.ones((rf.NSUB, rf.NCHAN))
    mask[1, 0] = 0.0
    whole = _call(eng, c, dtype, mask=mask)
    with eng.options(max_work_bytes=1.0):
        cut = _call(eng, c, dtype, mask=mask)
    for w in ALL4:
        assert cut[w].tobytes() == whole[w].tobytes(), w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", EDGE)
def test_device_tensors_give_device_tensors_with_the_host_routes_bits(eng, nbin, dtype):
    import torch
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    host = _call(eng, c, dtype)
    src = torch.as_tensor(c["data"].astype(dtype), device="cuda:0")
    before = src.clone()
    dev = eng.fit_residuals(src, c["freqs"], c["P"], c["params"], c["nu_refs"], c["scales"], errs=c["sigma"],
                            slots=c["slots"], want=ALL4)
    assert torch.equal(src, before)                       # (the input is not written)
    for w in ALL4:
        assert dev[w].is_cuda and dev[w].dtype == (torch.float64 if w == "red_chi2" else src.dtype)
        assert _bits(dev[w]) == host[w].tobytes(), w


@pytest.mark.parametrize("nbin", EDGE)
def test_a_rows_bits_do_not_depend_on_the_batch(eng, nbin):
    c = rf.case(nbin)
    _set_templates(eng, c["templates"])
    both = _call(eng, c)
    for i in range(rf.NSUB):
        alone = _call(eng, c, subs=slice(i, i + 1))
        for w in ALL4:
            assert alone[w].tobytes() == both[w][i:i + 1].tobytes(), (w, i)


def test_arguments_are_checked(eng):
    from pulseportraiture_amd.engine import EngineError
    c = rf.case(64)
    _set_templates(eng, c["templates"])
    with pytest.raises(ValueError):
        _call(eng, c, want=())
    with pytest.raises(ValueError):
        _call(eng, c, frame="sky")
    with pytest.raises(ValueError, match="needs errs"):
        _call(eng, c, errs=None)
    with eng.options(harm_eps=0.0):
        eng.set_model(rr.b_templates(128)[1][:rf.NCHAN], slot=1)
    with pytest.raises(EngineError, match="not a 3 x 64 template"):
        _call(eng, c)
