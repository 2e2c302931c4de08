"""rotate_portraits (k_rotate, k_rotate_any), channel_red_chi2 (k_chan_chi2, k_chan_chi2_harm) and
fit_phase_shift_batch (k_fps) called directly at every row plan -- nbin 32 ... 8192 and both ends of every chirp-z
class -- against the plain long-double references of tests/rot_refs.py, which tests/test_rot_refs_cpu.py pins to the
oracle, to closed forms and to the reference's fixtures; and every row-loop entry point with one more row than its
launch can have workgroups, bit for bit against the same rows in two calls.

Bars (none is taken from the device's output)
  A  rotation       2e-13 of the row's maximum at a power of two, 2e-12 on the chirp-z route: the rounding-level bars
                    tests/test_gpu_ppalign.py holds the same arithmetic to.  Under the delay law 2 pi M u is added,
                    u = 8 * 2^-53 * (the summed absolute terms of phi_n): what a last-place difference in the f64
                    phi_n costs the highest harmonic.  An f32 result must be the f32 rounding of SOME value within the
                    bar of the expectation (_need: the distance from the expectation to the interval of reals that
                    round to the value returned).  DM = 15 at 3 ms against the oracle: 5e-10 (NumPy's k * phi).
  B  chi^2          rtol 1e-10 against the time-domain references; the structured rows from their formulas.
  C  phase fit      |f' / f''| <= 1e-13 in the long-double objective, the other columns rtol 1e-9 at the device's
                    phase, the simplex phase 1e-12 mod 1 from the oracle.
  D  row loops      zero tolerance.
With PP_ROT_PARITY_OUT set, every measured deviation is written there beside its bar
(profiles/rot_kernels_parity.json)."""
import math

import numpy as np
import pytest

from oracle import pptoas_oracle as orc
from tests import rot_refs as rr
from tests.gpu_support import eng, measured_writer  # noqa: F401

pytestmark = pytest.mark.gpu

MEASURED, _write_measured = measured_writer("PP_ROT_PARITY_OUT")
LD = np.longdouble
DTYPES = [np.float64, np.float32]
INF5 = np.full(5, np.inf)


def _record(kind, tag, dev, bar, **extra):
    """The worst deviation of a case beside its bar; printed before anything is asserted."""
    of = float(dev / bar) if bar > 0 else (0.0 if dev == 0 else math.inf)
    e = MEASURED.setdefault(kind, {}).get(tag)
    if e is None or of >= e["of_bar"]:
        MEASURED[kind][tag] = dict(deviation=float(dev), bar=float(bar), of_bar=of, **extra)
    print(kind, tag, "deviation %.3e, bar %.3e: %.3f of the bar" % (dev, bar, of), extra or "")


def _need(got, want):
    """How far `want` is from a real that rounds to `got`: |got - want| for f64 results; for f32 results the distance
    from want to the interval between the midpoints of got and its two neighbours."""
    want = np.asarray(want, dtype=LD)
    if got.dtype == np.float64:
        return np.abs(got.astype(LD) - want)
    g = got.astype(LD)
    lo = (g + np.nextafter(got, np.float32(-np.inf)).astype(LD)) / 2
    hi = (g + np.nextafter(got, np.float32(np.inf)).astype(LD)) / 2
    return np.maximum(0, np.maximum(lo - want, want - hi))


def _hold_rows(kind, tag, got, want, bar, **extra):
    """Rows got[..., nbin] within bar[...] (absolute, per row) of want; records the worst row."""
    need = _need(got, want).max(axis=-1).astype(np.float64)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), need.shape)
    ratio = np.where(bar > 0, need / np.where(bar > 0, bar, 1), np.where(need > 0, np.inf, 0.0))
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
    _record(kind, tag, float(need[w]), float(bar[w]), **extra)
    assert np.all(np.isfinite(got))
    assert np.all(need <= bar), (kind, tag, float(ratio.max()))


def _tag(nbin, dtype, *more):
    return "-".join([str(nbin), np.dtype(dtype).name] + [str(m) for m in more])


# ==== A. rotate_portraits ======================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.ALL)
def test_a1_pure_phase(eng, nbin, dtype):
    """P = 1, DM = GM = 0, freqs = inf (ppalign's call): phi_n is phi exactly on the device.  Every row against the
    oracle, the long-double rows against rotate_ld."""
    x64, phis = rr.a1_cube(nbin), rr.a1_phis(nbin)
    got = eng.rotate_portraits(x64.astype(dtype), INF5, 1.0, phi=phis)
    assert got.dtype == dtype and got.shape == x64.shape
    bar = rr.rot_bar(nbin) * np.abs(x64).max(axis=-1)
    ref = rr.a1_reference(nbin)
    for (i, n), want in ref.items():
        _hold_rows("A1 long double", _tag(nbin, dtype), got[i, n], want, bar[i, n])
    oracle = np.stack([orc.rotate_data(x64[i], phis[i]) for i in range(3)])
    own = max(float(np.abs(want - oracle[p]).max() / np.abs(x64[p]).max()) for p, want in ref.items())
    _hold_rows("A1 oracle", _tag(nbin, dtype), got, oracle, bar, oracle_own_distance_of_row_max=own)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.ALL)
def test_a2_special_rows(eng, nbin, dtype):
    """DC, the Nyquist row at 0 / half a bin / one bin, the k = 1 and k = M - 1 cosines and an all-zero row in one
    call, against their closed forms.  The half-bin Nyquist row must vanish: the bar holds in absolute terms (its
    maximum is 1); the all-zero row stays all zero."""
    rows, want = rr.a2_rows(nbin, dtype)
    got = eng.rotate_portraits(rows, np.full(2, np.inf), 1.0, phi=rr.a2_phis(nbin))
    bar = rr.rot_bar(nbin) * np.abs(rows.astype(np.float64)).max(axis=-1)
    for i, name in enumerate(rr.A2_NAMES):
        _hold_rows("A2 " + name, _tag(nbin, dtype), got[i], want[i], bar[i])
    assert np.abs(got[2, 0]).max() <= rr.rot_bar(nbin)
    assert not got[6].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("iref", [0, 1])
@pytest.mark.parametrize("nbin", rr.A3_NBINS)
def test_a3_delay_law(eng, nbin, iref, dtype):
    """Per-subint frequency rows, P, DM and GM, finite and infinite reference frequencies, against
    rotate_ld(row, float(delay_ld(...)))."""
    nu_DM, nu_GM = rr.A3_REFS[iref]
    x64 = rr.a1_cube(nbin)
    phin, u = rr.a3_delays(nu_DM, nu_GM)
    got = eng.rotate_portraits(x64.astype(dtype), rr.a3_freqs(), rr.A3_P, phi=rr.A3_PHI, DM=rr.A3_DM, GM=rr.A3_GM,
                               nu_DM=nu_DM, nu_GM=nu_GM)
    for p, want in rr.a3_reference(nbin, iref).items():
        second = 2 * np.pi * (nbin // 2) * u[p]
        print("row %s: phi_n %+.6f, u %.2e, 2 pi M u %.2e" % (p, phin[p], u[p], second))
        _hold_rows("A3 delay law", _tag(nbin, dtype, "nu_DM", nu_DM), got[p], want,
                   (rr.rot_bar(nbin) + second) * np.abs(x64[p]).max(), second_part=second)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.A3_NBINS)
def test_a3_large_dm_against_the_oracle(eng, nbin, dtype):
    """DM = 15 at P = 3 ms is thousands of turns: NumPy's k * phi_n costs the oracle up to 5e-10 (the standing bar)."""
    x64 = rr.a1_cube(nbin)[:1]
    got = eng.rotate_portraits(x64.astype(dtype), rr.ROT_FREQS, 0.003, phi=0.2, DM=15.0, nu_DM=1400.0)
    want = orc.rotate_portrait_full(x64[0], 0.2, 15.0, 0.0, rr.ROT_FREQS, 1400.0, np.inf, 0.003)
    _hold_rows("A3 DM 15", _tag(nbin, dtype), got[0], want, 5e-10 * np.abs(x64[0]).max(axis=-1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.ALL)
def test_a4_in_place_and_round_trip(eng, nbin, dtype):
    """A device tensor is rotated in place to the bits of the host call; a rotation followed by its inverse restores
    every harmonic but the Nyquist one, which keeps cos^2(2 pi M phi_n) of itself (1e-9: the standing figure)."""
    import torch
    nu_DM, nu_GM = rr.A3_REFS[0]
    x = rr.a1_cube(nbin).astype(dtype)
    kw = dict(nu_DM=nu_DM, nu_GM=nu_GM)
    host = eng.rotate_portraits(x, rr.a3_freqs(), rr.A3_P, phi=rr.A3_PHI, DM=rr.A3_DM, GM=rr.A3_GM, **kw)
    t = torch.from_numpy(x.copy()).to("cuda:0")
    eng.rotate_portraits(t, rr.a3_freqs(), rr.A3_P, phi=rr.A3_PHI, DM=rr.A3_DM, GM=rr.A3_GM, **kw)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == host.tobytes()
    if dtype != np.float64:
        return
    back = eng.rotate_portraits(host, rr.a3_freqs(), rr.A3_P, phi=-rr.A3_PHI, DM=-rr.A3_DM, GM=-rr.A3_GM, **kw)
    d = np.fft.rfft(back - x, axis=-1)
    M = nbin // 2
    phin, _ = rr.a3_delays(nu_DM, nu_GM)
    sin2 = np.array([[float(np.sin(rr.PI2 * rr.turns_ld(np.array([M]), phin[i, n])[0]) ** 2) for n in range(5)]
                     for i in range(3)])
    xm = np.fft.rfft(x, axis=-1)[..., -1].real
    scale = np.abs(x).max() * nbin
    _record("A4 round trip", _tag(nbin, dtype), float(np.abs(d[..., :-1]).max()), 1e-9)
    assert np.abs(d[..., :-1]).max() < 1e-9
    assert np.abs(d[..., -1].real + xm * sin2).max() < 1e-9 * scale
    assert np.abs(d[..., -1]).max() > 1e-3


# ==== B. channel_red_chi2 ======================================================================================
def _set_templates(eng, tm):
    with eng.options(harm_eps=0.0):          # every harmonic kept: the Nyquist term of the model matters
        for s in range(len(tm)):
            assert eng.set_model(tm[s], slot=s) >= tm.shape[-1] // 2     # (a general length's count is padded)


def _b1_call(eng, c, dtype, subs=slice(None)):
    return eng.channel_red_chi2(c["data"][subs].astype(dtype), c["freqs"][subs], c["P"][subs], c["params"][subs],
                                c["nu_refs"][subs], c["scales"][subs], c["sigma"][subs],
                                slots=rr.B_SLOTS[subs])


def _b1_oracle(c):
    return np.stack([orc.channel_red_chi2s(c["data"][i], c["templates"][rr.B_SLOTS[i]], *c["params"][i],
                                           c["freqs"][i], c["nu_refs"][i], c["P"][i], c["scales"][i], c["sigma"][i])
                     for i in range(rr.B_NSUB)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.ALL)
def test_b1_fitted_subints(eng, nbin, dtype):
    """Four subints (phi; phi, DM; phi, DM, GM; phi, DM, tau) on two templates, per-subint frequency rows, a negative
    and a zero scale: every row against the oracle, the long-double rows against chan_red_chi2_ld, rtol 1e-10.  A
    subint's row of chi^2 has the same bits alone and in the batch."""
    c = rr.b1_case(nbin)
    _set_templates(eng, c["templates"])
    got = _b1_call(eng, c, dtype)
    want = _b1_oracle(c)
    regular = np.ones(want.shape, dtype=bool)
    regular[1, 2] = regular[2, 3] = False
    assert 0.5 < np.median(want[regular]) < 2
    np.testing.assert_allclose(want[2, 3], rr.zero_scale_chi2(c["data"][2, 3], c["phin"][2, 3], c["sigma"][2, 3]),
                               rtol=1e-11)
    for p, v in rr.b1_reference(nbin).items():
        _record("B1 long double", _tag(nbin, dtype), abs(got[p] - float(v)) / float(v), 1e-10,
                oracle_own_distance=abs(want[p] - float(v)) / float(v))
        np.testing.assert_allclose(got[p], float(v), rtol=1e-10)
    _record("B1 oracle", _tag(nbin, dtype), float(np.abs(got / want - 1).max()), 1e-10)
    np.testing.assert_allclose(got, want, rtol=1e-10)
    for i in range(rr.B_NSUB):                                                  # B3
        alone = _b1_call(eng, c, dtype, slice(i, i + 1))
        assert alone.tobytes() == got[i:i + 1].tobytes(), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nbin", rr.ALL)
def test_b2_structured_rows(eng, nbin, dtype):
    """Rows with known answers, all reference frequencies infinite and tau = 0 (phi_n = phi):
    (0) data = 0, scale 1: the template's own sum m^2 / sigma^2 / (nbin - 2);
    (1) the alternating row, scale 0, turned by half a bin: nothing is left (Nyquist keeps its real part only) -- each
        bin of the rotated row is within the rotation's bar of 0, so chi^2 <= nbin (bar x max)^2 / sigma^2 / (nbin - 2);
    (2) the same turned by one bin: sum data^2 / sigma^2 / (nbin - 2);
    (3) a row equal to its template, phi = 0, scale 1: each bin's residual is at most nbin 2^-52 of the template there,
        so chi^2 <= (nbin 2^-52)^2 sum m^2 / sigma^2 / (nbin - 2)."""
    tm = rr.b_templates(nbin)
    _set_templates(eng, tm)
    nc = rr.B_NCHAN
    amp = 1.0 + np.arange(nc)
    alt = np.where(np.arange(nbin) % 2 == 0, 1.0, -1.0) * amp[:, None]
    data = np.stack([np.zeros((nc, nbin)), alt, alt, tm[1]]).astype(dtype)
    assert np.array_equal(data[3].astype(np.float64), tm[1])                     # (the templates are f32-exact)
    sigma = np.tile(np.linspace(0.05, 0.2, nc), (4, 1))
    params = np.zeros((4, 5))
    params[:, 0] = [0.1234, 0.5 / nbin, 1.0 / nbin, 0.0]
    scales = np.array([np.ones(nc), np.zeros(nc), np.zeros(nc), np.ones(nc)])
    got = eng.channel_red_chi2(data, np.full(nc, 1400.0), 1.0, params, np.full((4, 3), np.inf), scales, sigma,
                               slots=[0, 0, 0, 1])
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    dof = nbin - 2
    sm = [np.sum(tm[s].astype(LD) ** 2, axis=-1).astype(np.float64) / sigma[0] ** 2 / dof for s in (0, 1)]
    _record("B2 zero data", _tag(nbin, dtype), float(np.abs(got[0] / sm[0] - 1).max()), 1e-10)
    np.testing.assert_allclose(got[0], sm[0], rtol=1e-10)
    bar1 = nbin * (rr.rot_bar(nbin) * amp) ** 2 / sigma[1] ** 2 / dof
    _record("B2 nyquist half bin", _tag(nbin, dtype), float((got[1] / bar1).max()), 1.0)
    assert np.all(got[1] <= bar1)
    want2 = nbin * amp ** 2 / sigma[2] ** 2 / dof
    _record("B2 nyquist one bin", _tag(nbin, dtype), float(np.abs(got[2] / want2 - 1).max()), 1e-10)
    np.testing.assert_allclose(got[2], want2, rtol=1e-10)
    bar3 = (nbin * 2.0 ** -52) ** 2 * sm[1]
    _record("B2 own template", _tag(nbin, dtype), float((got[3] / bar3).max()), 1.0)
    assert np.all(got[3] <= bar3)


def test_b3_wrong_template_shape_is_refused(eng):
    """A slot whose template has another nchan or nbin than the portraits is refused on the host, before a launch."""
    from pulseportraiture_amd.engine import EngineError
    c = rr.b1_case(64)
    _set_templates(eng, c["templates"])
    with eng.options(harm_eps=0.0):
        eng.set_model(np.concatenate([c["templates"][1], c["templates"][1][:1]]), slot=1)        # nchan + 1
    with pytest.raises(EngineError, match="not a 6 x 64 template"):
        _b1_call(eng, c, np.float64)
    with eng.options(harm_eps=0.0):
        eng.set_model(rr.b_templates(128)[1], slot=1)                                           # another nbin
    with pytest.raises(EngineError, match="not a 6 x 64 template"):
        _b1_call(eng, c, np.float64)
    _set_templates(eng, c["templates"])
    assert _b1_call(eng, c, np.float64).shape == (rr.B_NSUB, rr.B_NCHAN)


# ==== C. fit_phase_shift_batch =================================================================================
@pytest.mark.parametrize("nbin", rr.C_NBINS)
def test_c1_newton(eng, nbin):
    """finish = 'newton' for Ns in {1, 2, 100, 257, nbin} and both bounds: the phase is a minimum of the long-double
    objective, |f' / f''| <= 1e-13, and columns 1 ... 5 are fps_columns at the device's phase, rtol 1e-9.  (With one or
    two grid points the start is far from the best alignment and the polish settles in whichever local minimum its
    bracket holds; both assertions hold at any of them.)"""
    data, model, sigma = rr.c_case(nbin)
    for kind, bounds in rr.C_BOUNDS.items():
        for Ns in sorted(set(rr.C_NS(nbin))):
            out = eng.fit_phase_shift_batch(data, model, noise=sigma, bounds=bounds, Ns=Ns, finish="newton")
            assert out.shape == (5, 7) and np.all(np.isfinite(out[:, 0]))
            for i in range(5):
                ld = i in rr.c_ld_pairs(nbin)
                f, f1, f2 = rr.fps_objective_ld(data[i], model[i], out[i, 0], ld=ld)
                step = abs(float(f1 / f2))
                _record("C1 optimum", "%d-Ns%d-%s" % (nbin, Ns, kind), step, 1e-13, pair=i)
                assert f2 > 0 and step <= 1e-13, (kind, Ns, i, step)
                cols = rr.fps_columns(data[i], model[i], sigma[i], out[i, 0], ld=ld).astype(np.float64)
                _record("C1 columns", "%d-Ns%d-%s" % (nbin, Ns, kind), float(np.nanmax(np.abs(out[i, 1:6] / cols - 1))),
                        1e-9, pair=i)
                np.testing.assert_allclose(out[i, 1:6], cols, rtol=1e-9)


C2_NOISE = ["none", "given", "mixed"]


def _c2_noise(mode, sigma):
    """(what the device gets, what the oracle gets per pair); NaN and -1 are measured: !(sig >= 0)."""
    if mode == "none":
        return None, [None] * 5
    if mode == "given":
        return sigma, list(sigma)
    return np.array([sigma[0], np.nan, -1.0, sigma[3], np.nan]), [sigma[0], None, None, sigma[3], None]


@pytest.mark.parametrize("mode", C2_NOISE)
@pytest.mark.parametrize("nbin", rr.C_NBINS)
def test_c2_simplex(eng, nbin, mode):
    """finish = 'simplex', Ns = 100: the reference's phase to 1e-12 mod 1 and its other columns to 1e-9, with the noise
    missing, given, and a value, NaN and -1 mixed in one batch."""
    data, model, sigma = rr.c_case(nbin)
    dev_noise, orc_noise = _c2_noise(mode, sigma)
    out = eng.fit_phase_shift_batch(data, model, noise=dev_noise, Ns=100, finish="simplex")
    for i in range(5):
        r = orc.fit_phase_shift(data[i], model[i], noise=orc_noise[i], Ns=100)
        dphi = abs((out[i, 0] - r.phase + 0.5) % 1.0 - 0.5)
        _record("C2 simplex phase", "%d-%s" % (nbin, mode), dphi, 1e-12, pair=i)
        assert dphi < 1e-12, (i, dphi)
        want = np.array([r.phase_err, r.scale, r.scale_err, r.snr, r.red_chi2])
        _record("C2 simplex columns", "%d-%s" % (nbin, mode), float(np.abs(out[i, 1:6] / want - 1).max()), 1e-9, pair=i)
        np.testing.assert_allclose(out[i, 1:6], want, rtol=1e-9)


@pytest.mark.parametrize("nbin,nprof", [(8192, 3), (32, 300)])
@pytest.mark.parametrize("finish", ["newton", "simplex"])
def test_c3_a_pair_alone_has_its_bits_in_the_batch(eng, nbin, nprof, finish):
    """8192 bins: the cross-spectrum of pair i lives at xwork + i M in global memory; 32 bins: M = 16 < 256, most threads
    hold no harmonic."""
    data0, model0, sigma0 = rr.c_case(nbin)
    rng = np.random.default_rng(nprof)
    data = np.tile(data0, (nprof // 5 + 1, 1))[:nprof] + rng.normal(0, 0.01, (nprof, nbin))
    model = np.tile(model0[:1], (nprof, 1))
    noise = np.where(np.arange(nprof) % 3 == 0, np.nan, np.tile(sigma0, nprof // 5 + 1)[:nprof])
    batch = eng.fit_phase_shift_batch(data, model, noise=noise, finish=finish)[:, :6]
    picks = range(nprof) if nprof <= 3 else [0, 1, 2, 63, 64, 255, 256, 257, 298, 299]
    for i in picks:
        alone = eng.fit_phase_shift_batch(data[i], model[i], noise=noise[i:i + 1], finish=finish)[:, :6]
        assert alone.tobytes() == batch[i:i + 1].tobytes(), i


# ==== D. beyond one row per workgroup ==========================================================================
# A workgroup takes a second row only when the call has more rows than the launch has workgroups.  Where each cap is set:
#   launch                          cap                                    source
#   fft_grid(T, nrows)              256 x 8 = 2048 (T = 64: nbin <= 2048)  csrc/pp_toas.hip:641-645
#                                   256 x 4 = 1024 (T = 256: nbin 4096)
#                                   256 x 2 = 512  (T = 512: nbin 8192)
#   any_grid(nrows)                 2048                                   csrc/pp_toas.hip:691
#   k_chan_chi2_harm                4096                                   csrc/pp_extra_api.h:583
#   resident_grid (channel_noise)   CUs x workgroups resident per CU       csrc/pp_toas.hip:896-910
#                                   <= CUs x (2048 // T): a CU holds at most 2048 threads
D_ANY = [62, 254, 1022, 4094]


def _threads(nbin):
    return 64 if nbin <= 2048 else (256 if nbin == 4096 else 512)


def _rows_beyond(nbin, launch="fft"):
    """One more row than the largest grid the launch can have."""
    if launch == "chi2_harm":
        return 4097
    if launch == "resident":
        import torch
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        return ncu * (2048 // _threads(nbin)) + 1
    if not rr.is_pow2(nbin) or nbin < 32:
        return 2049
    return {64: 2049, 256: 1025, 512: 513}[_threads(nbin)]


def _halves(n):
    """Two runs that each stay below the cap n - 1."""
    return [slice(0, n // 2), slice(n // 2, n)]


@pytest.mark.parametrize("nbin", rr.POW2 + D_ANY)
def test_d_rfft_rows(eng, nbin):
    n = _rows_beyond(nbin)
    x = np.random.default_rng(nbin).standard_normal((n, nbin), dtype=np.float32)
    one = eng.rfft_rows(x)
    two = np.concatenate([eng.rfft_rows(x[s]) for s in _halves(n)])
    assert one.tobytes() == two.tobytes()


def _d_rot_args(nbin, nsub, nchan, rng):
    fr = np.linspace(1200.0, 1700.0, nchan) + rng.uniform(-5, 5, (nsub, 1))
    return dict(freqs=fr, P=rng.uniform(0.003, 0.01, nsub), phi=rng.uniform(-0.5, 0.5, nsub),
                DM=rng.uniform(-3e-3, 3e-3, nsub), GM=rng.uniform(-0.2, 0.2, nsub))


@pytest.mark.parametrize("nbin", rr.POW2 + D_ANY)
def test_d_rotate_portraits(eng, nbin):
    nchan = 3
    nsub = -(-_rows_beyond(nbin) // nchan)
    rng = np.random.default_rng(nbin)
    x = rng.standard_normal((nsub, nchan, nbin), dtype=np.float32)
    a = _d_rot_args(nbin, nsub, nchan, rng)

    def call(s):
        return eng.rotate_portraits(x[s], a["freqs"][s], a["P"][s], phi=a["phi"][s], DM=a["DM"][s], GM=a["GM"][s],
                                    nu_DM=1400.0, nu_GM=1300.0)
    one = call(slice(None))
    assert one.tobytes() == np.concatenate([call(s) for s in _halves(nsub)]).tobytes()
    i = nsub - 1                                   # three rows of the second pass
    x64 = x[i].astype(np.float64)
    want = orc.rotate_portrait_full(x64, a["phi"][i], a["DM"][i], a["GM"][i], a["freqs"][i], 1400.0, 1300.0, a["P"][i])
    u = np.array([8 * 2.0 ** -53 * float(sum(abs(t) for t in rr.delay_terms_ld(
        a["phi"][i], a["DM"][i], a["GM"][i], nu, 1400.0, 1300.0, a["P"][i]))) for nu in a["freqs"][i]])
    _hold_rows("D rotate second pass", str(nbin), one[i], want,
               (rr.rot_bar(nbin) + 2 * np.pi * (nbin // 2) * u) * np.abs(x64).max(axis=-1))


@pytest.mark.parametrize("nbin", rr.POW2 + D_ANY)
def test_d_channel_red_chi2(eng, nbin):
    nchan = 17
    nsub = -(-_rows_beyond(nbin, "fft" if rr.is_pow2(nbin) else "chi2_harm") // nchan)
    rng = np.random.default_rng(nbin)
    tm = np.stack([rr.f32_exact(0.3 + (1 + 0.05 * np.arange(nchan))[:, None] * rr.gauss_profile(nbin, 0.4, w))
                   for w in (0.05, 0.1)])
    _set_templates(eng, tm)
    x = rng.standard_normal((nsub, nchan, nbin), dtype=np.float32)       # noise of sigma 1: chi^2 near 1
    a = _d_rot_args(nbin, nsub, nchan, rng)
    params = np.stack([a["phi"], a["DM"], a["GM"], np.where(np.arange(nsub) % 2, 0.01, 0.0), np.full(nsub, -4.0)], axis=1)
    nu_refs = np.stack([np.full(nsub, 1400.0), np.where(np.arange(nsub) % 3, 1300.0, np.inf), np.full(nsub, 1500.0)], axis=1)
    scales = rng.uniform(-0.2, 0.5, (nsub, nchan))
    sigma = rng.uniform(0.8, 1.2, (nsub, nchan))
    slots = (np.arange(nsub) // 2) % 2

    def call(s):
        return eng.channel_red_chi2(x[s], a["freqs"][s], a["P"][s], params[s], nu_refs[s], scales[s], sigma[s],
                                    slots=slots[s])
    one = call(slice(None))
    assert one.tobytes() == np.concatenate([call(s) for s in _halves(nsub)]).tobytes()
    i = nsub - 1
    want = orc.channel_red_chi2s(x[i].astype(np.float64), tm[slots[i]], *params[i], a["freqs"][i], nu_refs[i], a["P"][i],
                                 scales[i], sigma[i])
    assert 0.5 < np.median(want) < 2
    _record("D chi2 second pass", str(nbin), float(np.abs(one[i] / want - 1).max()), 1e-10)
    np.testing.assert_allclose(one[i], want, rtol=1e-10)


def _d_template(eng, nbin, nchan=3):
    tm = 0.2 + (1 + 0.1 * np.arange(nchan))[:, None] * rr.gauss_profile(nbin, 0.4, 0.06)
    eng.set_model(tm, slot=0)
    return nchan


@pytest.mark.parametrize("nbin", rr.POW2 + D_ANY)
def test_d_fake_portraits(eng, nbin):
    import torch
    nchan = _d_template(eng, nbin)
    nsub = -(-_rows_beyond(nbin) // nchan)
    rng = np.random.default_rng(nbin)
    delays, amps = rng.uniform(-0.5, 0.5, (nsub, nchan)), rng.uniform(0.5, 2.0, (nsub, 1, nchan))
    sigmas = np.array([0.1, 0.2, 0.3])
    dst = torch.empty((nsub, nchan, nbin), dtype=torch.float32, device="cuda:0")
    eng.fake_portraits(dst, delays, amps=amps, sigmas=sigmas, seed=77, first_subint=5)
    torch.cuda.synchronize()
    one = dst.cpu().numpy().tobytes()
    dst.zero_()
    for s in _halves(nsub):
        eng.fake_portraits(dst[s], delays[s], amps=amps[s], sigmas=sigmas, seed=77, first_subint=5 + s.start)
    torch.cuda.synchronize()
    assert one == dst.cpu().numpy().tobytes()


@pytest.mark.parametrize("nbin", rr.POW2 + D_ANY)
def test_d_synth_portraits(eng, nbin):
    import torch
    nchan = _d_template(eng, nbin)
    nsub = -(-_rows_beyond(nbin) // nchan)
    rng = np.random.default_rng(nbin)
    freqs = np.linspace(1200.0, 1700.0, nchan)
    P = rng.uniform(0.003, 0.01, nsub)
    inj = np.stack([rng.uniform(-0.5, 0.5, nsub), rng.uniform(-3e-3, 3e-3, nsub), rng.uniform(-0.2, 0.2, nsub)], axis=1)
    gains = rng.uniform(0.5, 2.0, (nsub, nchan))
    dst = torch.empty((nsub, nchan, nbin), dtype=torch.float32, device="cuda:0")
    eng.synth_portraits(dst, freqs, P, inj, 0.05, seed=99, first_subint=3, gains=gains)
    torch.cuda.synchronize()
    one = dst.cpu().numpy().tobytes()
    dst.zero_()
    for s in _halves(nsub):
        eng.synth_portraits(dst[s], freqs, P[s], inj[s], 0.05, seed=99, first_subint=3 + s.start, gains=gains[s])
    torch.cuda.synchronize()
    assert one == dst.cpu().numpy().tobytes()


@pytest.mark.parametrize("nbin", [n for n in rr.POW2 if n <= 4096] + D_ANY)
def test_d_channel_noise_and_snrs(eng, nbin):
    """f32 rows.  (At the general lengths the noise kernel takes one row per workgroup; its harmonics come from the
    transform launched through any_grid.)"""
    n = _rows_beyond(nbin, "resident") if rr.is_pow2(nbin) else _rows_beyond(nbin)
    x = np.random.default_rng(nbin).standard_normal((n, nbin), dtype=np.float32)
    x += np.float32(2.0)                              # (a positive mean: 'mean' norms and S/N away from 0)
    noise, norms = eng.channel_noise(x, norm="mean")
    snrs = eng.channel_snrs(x)
    parts = [eng.channel_noise(x[s], norm="mean") for s in _halves(n)]
    assert noise.tobytes() == np.concatenate([p[0] for p in parts]).tobytes()
    assert norms.tobytes() == np.concatenate([p[1] for p in parts]).tobytes()
    assert snrs.tobytes() == np.concatenate([eng.channel_snrs(x[s]) for s in _halves(n)]).tobytes()
    assert np.all(np.isfinite(noise)) and np.all(noise > 0) and np.all(np.isfinite(snrs))
