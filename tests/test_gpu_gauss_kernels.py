"""The ppgauss device kernels (pp_gaussfit.h, and the row code shared with the template synthesis in pp_extra.h) held
directly against the plain long-double reference of tests/gauss_refs.py, which tests/test_gauss_refs_cpu.py pins to
the true reference's fixtures: residual rows at every row plan (M = 16 ... 4096) and on the general-length route,
unjoined and joined, with a component 1.2 bins wide that carries power up to the Nyquist harmonic; the extremes of the
scattering filter; set indexing; f32 and device input; the template synthesis on the same row code; and the
normal-equation reduction on integer rows, where the answer is exact.

Bars
  rows (a to f)   per channel the larger of the standing device-vs-host bar of tests/test_gpu_ppgauss.py, 2e-14
                  max|model| / sigma_n + spacing(max|data| / sigma_n), and 10 x the distance of the f64 host
                  construction (gaussfit.host_residuals) from the long-double reference on the same case
                  (gauss_refs.Case.reference; the device's transform is one more f64 arrangement of the same
                  arithmetic).  Never taken from the device's output.
  decisions       every case asserts peak_margin >= 1e-9 for every component whose loc is on no bin edge
  exact           normal equations of integer rows, resident against fetched rows, a channel in no band against the
                  unjoined launch, a set alone against the set among a hundred, f32 and device data against the f64
                  host call: zero tolerance
With PP_GAUSS_KERNELS_PARITY_OUT set, every case's device deviation, host distance and bar are written there as JSON
(profiles/gauss_kernels_parity.json)."""
import math

import numpy as np
import pytest

from tests import gauss_refs as gr
from tests.gpu_support import eng, measured_writer  # noqa: F401
from tests.test_gpu_ppgauss import _cancelling_rows, _fsum_reference

pytestmark = pytest.mark.gpu

MEASURED, _write_measured = measured_writer("PP_GAUSS_KERNELS_PARITY_OUT")
LD = np.longdouble
ALL_NBIN = gr.POW2_NBIN + gr.ANY_NBIN


def _args(sets, nbin):
    sets = np.atleast_2d(sets)
    return sets[:, 0], sets[:, 1] / nbin, sets[:, -1], sets[:, 2:-1].reshape(len(sets), -1, 6)


def _launch(eng, c, sets=None, join=None):
    sets = c.sets if sets is None else sets
    kw = {} if join is None else dict(join=join)
    got = eng.gauss_residuals(c.code, gr.NU_REF, *_args(sets, c.nbin), fetch=True, **kw)
    assert got.shape == (len(sets), len(c.freqs), c.nbin)
    return got


def _hold(c, got, rows, bar, host, kind, tag=None):
    """got within bar[nchan] of the long-double rows; the worst channel's figures are recorded (and printed first)."""
    dev = np.abs(got.astype(LD) - rows).max(axis=(0, 2)).astype(np.float64)
    n = int(np.argmax(dev / bar))
    entry = dict(device_deviation=float(dev[n]), host_distance=float(host[n]), bar=float(bar[n]),
                 of_bar=float(dev[n] / bar[n]), widened=bool(np.any(10 * host >= bar)))
    MEASURED.setdefault(kind, {})[tag or c.name] = entry
    print(kind, tag or c.name, "deviation %.3e, host distance %.3e, bar %.3e: %.3f of the bar" %
          (entry["device_deviation"], entry["host_distance"], entry["bar"], entry["of_bar"]))
    assert np.all(np.isfinite(got))
    assert np.all(dev <= bar), (c.name, float((dev / bar).max()))


def _hold_rows(c, got, kind, pick=slice(None)):
    r = c.reference()
    _hold(c, got, r["rows"][pick], r["bar"], r["host"], kind)


# ---- a. residual rows at every plan ----------------------------------------------------------------------
@pytest.mark.parametrize("code", gr.CODES)
@pytest.mark.parametrize("nbin", ALL_NBIN)
def test_residual_rows_at_every_plan(eng, nbin, code):
    """nchan = 5; one launch of four sets: the base point, tau stepped from 0 (so scattered and unscattered sets share
    the launch), alpha stepped, a loc stepped."""
    c = gr.case("rows", nbin, code)
    assert c.margins_ok()
    r = c.reference()
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        got = _launch(eng, c)
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "rows")


# ---- b. the same sizes joined ----------------------------------------------------------------------------
@pytest.mark.parametrize("code", gr.CODES)
@pytest.mark.parametrize("nbin", ALL_NBIN)
def test_joined_rows_at_every_plan(eng, nbin, code):
    """Two bands and a channel in none; one launch of five sets: unjoined (an all-zero join), rotated with tau = 0,
    rotated and scattered, phase-only, Delta-DM-only.  The rows of the channel in no band are the unjoined launch's, bit
    for bit, in every set."""
    c = gr.case("joined", nbin, code)
    assert c.margins_ok()
    r = c.reference()
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        plain = _launch(eng, c)
        eng.gauss_fit_join(c.band, gr.PERIOD)
        got = _launch(eng, c, join=c.join)
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "joined")
    none = np.flatnonzero(c.band < 0)
    assert len(none) == 1
    np.testing.assert_array_equal(got[:, none], plain[:, none])
    np.testing.assert_array_equal(got[0], plain[0])             # (and the all-zero set is the unjoined one)
    # every row with a rotation is rotated; one without -- also band 1's channel at nu_ref in the Delta-DM-only set --
    # keeps the bits it has without a band map
    phi = np.array([gr.rotations(c.join[s], c.band, c.freqs, gr.NU_REF, gr.PERIOD) for s in range(len(c.sets))])
    assert (phi == 0).sum() == len(c.freqs) + (len(c.sets) - 1) + 1
    moved = np.abs(got - plain).max(axis=-1) > 0
    assert np.array_equal(moved, phi != 0)


# ---- c. extremes of the filter ---------------------------------------------------------------------------
@pytest.mark.parametrize("code", gr.CODES)
@pytest.mark.parametrize("nbin", [2048, 250])
def test_extremes_of_the_filter(eng, nbin, code):
    """2 pi M tau_n ~ 1e6; tau = 1e-12 rot; tau = 0; alpha = 0 and alpha = -4.4.  The true rows of tau = 1e-12 and
    tau = 0 differ by thousands of bars with a component 1.2 bins wide (tests/test_gauss_refs_cpu.py measures it), so
    the device's two sets of rows cannot lie within the bar of each other; their deviations from their own references
    must: the step from no transform to a transform adds no error of its own."""
    c = gr.case("extreme", nbin, code)
    assert c.margins_ok()
    r = c.reference()
    x = 2 * np.pi * (nbin // 2) * c.sets[0, 1] / nbin * (c.freqs / gr.NU_REF) ** gr.ALPHA
    assert np.all(x > 3e5) and np.all(x < 3e6)
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        got = _launch(eng, c)
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "extreme")
    d = (got[1].astype(LD) - r["rows"][1]) - (got[2].astype(LD) - r["rows"][2])
    step = np.abs(d).max(axis=-1).astype(np.float64)
    MEASURED["extreme"][c.name]["tiny_tau_step_of_bar"] = float((step / r["bar"]).max())
    assert np.all(step <= r["bar"]), float((step / r["bar"]).max())


@pytest.mark.parametrize("code", gr.CODES)
@pytest.mark.parametrize("ngauss", [1, 16])
@pytest.mark.parametrize("nbin", [2048, 250])
def test_one_and_sixteen_components(eng, nbin, ngauss, code):
    c = gr.case("extreme", nbin, code, ngauss)
    assert c.margins_ok() and c.sets.shape[1] == 3 + 6 * ngauss
    r = c.reference()
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        got = _launch(eng, c)
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "extreme")


# ---- d. set indexing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [32, 100])
def test_a_hundred_sets_each_its_own(eng, nbin):
    """100 sets, nchan = 2, every set with a dc, tau, alpha and one component value of its own: each against the
    reference, and sets 0, 57 and 99 launched alone give the bits they have among the hundred."""
    c = gr.case("indexed", nbin, "000")
    assert c.margins_ok() and len(c.sets) == 100
    for col in (0, 1, -1):
        assert len(np.unique(c.sets[:, col])) == 100
    r = c.reference()
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        got = _launch(eng, c)
        alone = [_launch(eng, c, sets=c.sets[s:s + 1])[0] for s in (0, 57, 99)]
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "indexed")
    dev = np.abs(got.astype(LD) - r["rows"]).max(axis=2).astype(np.float64)
    assert np.all(dev <= r["bar"][None]), int(np.argmax((dev / r["bar"][None]).max(axis=1)))       # set by set
    for s, rows in zip((0, 57, 99), alone):
        np.testing.assert_array_equal(rows, got[s])


# ---- e. f32 and device input -----------------------------------------------------------------------------
def _four_ways(eng, data, freqs, errs, code, sets, nbin):
    import torch
    out = []
    for d in (data, data.astype(np.float32), torch.as_tensor(data.astype(np.float32), device="cuda"),
              torch.as_tensor(data, device="cuda")):
        eng.gauss_fit_begin(d, freqs, errs)
        try:
            out.append(eng.gauss_residuals(code, gr.NU_REF, *_args(sets, nbin), fetch=True))
        finally:
            eng.gauss_fit_end()
    return out


def test_f32_and_device_data_give_the_f64_host_bits(eng):
    """nbin = 2048 x nchan = 5: data as f32 host, f32 device and f64 device against the f64 host call (the data sits on
    a grid of 2^-20, so f32 holds it exactly and the widened values are the f64 ones)."""
    c = gr.case("rows", 2048, "000")
    r = c.reference()
    assert np.array_equal(r["data"].astype(np.float32).astype(np.float64), r["data"])
    host64, host32, dev32, dev64 = _four_ways(eng, r["data"], c.freqs, c.errs, c.code, c.sets, c.nbin)
    _hold_rows(c, host32, "f32")
    for other in (host32, dev32, dev64):
        np.testing.assert_array_equal(other, host64)


def test_f32_widening_takes_a_second_trip(eng):
    """160 x 8192 = 1 310 720 elements, more than the 4096 x 256 threads of the widening launch: every element of the
    second trip of its stride loop must arrive.  One scattered set; the data a f32-exact grid of values of its own."""
    nchan, nbin = 160, 8192
    assert nchan * nbin > 4096 * 256
    rng = np.random.default_rng(160)
    data = np.rint(rng.standard_normal((nchan, nbin)) * 2.0 ** 20) / 2.0 ** 20
    assert np.array_equal(data.astype(np.float32).astype(np.float64), data) and len(np.unique(data)) > nchan * nbin // 2
    freqs = np.linspace(1100.0, 1900.0, nchan)
    errs = 0.05 + 0.001 * np.arange(nchan)
    sets = gr.row_sets(nbin)[1:2]
    host64, host32, dev32, dev64 = _four_ways(eng, data, freqs, errs, "000", sets, nbin)
    for other in (host32, dev32, dev64):
        np.testing.assert_array_equal(other, host64)
    # (the rows are residuals of this data: the model is bounded, so they follow the data)
    assert np.abs(host64[0] * errs[:, None] - data).max() < 20.0 and np.all(np.isfinite(host64))


# ---- f. template synthesis on the shared row code -------------------------------------------------------
@pytest.mark.parametrize("code", gr.CODES)
@pytest.mark.parametrize("nbin", [32, 128, 2048, 8192])
def test_template_synthesis_on_the_shared_row_code(eng, nbin, code):
    """eng.gaussian_portrait of the family's model, unscattered and scattered, against gauss_refs.portrait: the rows
    bar in model units (sigma_n taken out, the data's ulp replaced by the model's)."""
    c = gr.case("rows", nbin, code)
    assert c.margins_ok()
    r = c.reference()
    peak = float(np.abs(r["model"]).max())
    host = r["host"] * c.errs
    bar = np.maximum(2e-14 * peak + np.spacing(peak), 10 * host)
    for s, what in ((0, "plain"), (1, "scattered")):
        v = c.sets[s]
        mdl = dict(params=v[:-1], code=code, nu_ref=gr.NU_REF, alpha=v[-1], ngauss=(len(v) - 3) // 6)
        got = eng.gaussian_portrait(mdl, c.freqs, nbin, P=float(nbin))
        assert got.shape == (len(c.freqs), nbin)
        _hold(c, got[None], r["model"][s:s + 1], bar, host, "template", "%s_%s" % (c.name, what))


# ---- g. normal equations, exact --------------------------------------------------------------------------
def _exact_normal(eng, nsets, nrow):
    import torch
    R_int, shifts = gr.integer_rows(nsets, nrow, 100 * nsets + nrow % 9973)
    assert np.all(R_int != 0) and np.abs(R_int).max() <= 512 and nrow * 512 ** 2 < 2 ** 53
    chi2, g, G = gr.gram_exact(R_int, shifts)
    R, h = gr.gram_rows(R_int, shifts)
    a = eng.gauss_normal(h, rows=R)
    bad = dict(chi2=abs(a[0] - float(chi2)), g=float(np.abs(a[1] - g).max()) if nsets > 1 else 0.0,
               G=float(np.abs(a[2] - G).max()) if nsets > 1 else 0.0)
    MEASURED.setdefault("normal_exact", {})["nsets%d_nrow%d" % (nsets, nrow)] = dict(deviation=max(bad.values()))
    assert a[0] == float(chi2), bad
    assert a[1].shape == (nsets - 1,) and a[2].shape == (nsets - 1, nsets - 1)
    assert np.array_equal(a[1], g.astype(np.float64)), bad
    assert np.array_equal(a[2], G.astype(np.float64)), bad
    b = eng.gauss_normal(h, rows=R)
    d = eng.gauss_normal(h, rows=torch.as_tensor(R, device="cuda"))
    for other in (b, d):
        assert other[0] == a[0] and np.array_equal(other[1], a[1]) and np.array_equal(other[2], a[2])


@pytest.mark.parametrize("nrow", [1, 31, 32, 33, 255, 256, 257, 256 * 3 + 33, 262144, 262145, 524288])
def test_normal_equations_exact_at_every_chunk_edge(eng, nrow):
    """nsets = 3.  Integer rows and power-of-two steps: every product and every partial sum is an integer below 2^53, so
    any order of summation gives gram_exact's integers; one dropped, doubled or misattributed sample is off by >= 1.
    Up to 262 144 samples the chunks hold 256, above they grow; 262 145 leaves a last chunk of one sample."""
    _exact_normal(eng, 3, nrow)


@pytest.mark.parametrize("nsets", [1, 2, 16, 17, 22, 23, 100])
def test_normal_equations_exact_at_every_pair_regime(eng, nsets):
    """nrow = 801.  nsets^2 <= 256: at most one pair per thread; 257 ... 512: two; above: up to GN_ACC."""
    _exact_normal(eng, nsets, 801)


# ---- h. normal equations, rounded ------------------------------------------------------------------------
@pytest.mark.parametrize("nrow", [4096, 262145])
def test_normal_equations_of_cancelling_rows(eng, nrow):
    """tests/test_gpu_ppgauss.py's cancelling rows (R_a - R_0 loses seven digits) against math.fsum, to its derived bar
    nrow 2^-53 sum|terms|."""
    nsets = 3
    R, h = _cancelling_rows(nsets, nrow, 1000 * nsets + nrow)
    chi2, gvec, G = eng.gauss_normal(h, rows=R)
    S, A = _fsum_reference(R, h)
    bar = nrow * 2.0 ** -53 * A
    got = np.empty((nsets, nsets))
    got[0, 0], got[0, 1:], got[1:, 0], got[1:, 1:] = chi2, gvec, gvec, G
    worst = float((np.abs(got - S) / bar).max())
    MEASURED.setdefault("normal_rounded", {})["nrow%d" % nrow] = dict(of_bar=worst)
    print("nrow", nrow, "worst %.3e of the bar" % worst)
    assert math.isfinite(worst) and np.all(np.abs(got - S) <= bar), worst
    np.testing.assert_array_equal(G, G.T)


# ---- i. resident rows ------------------------------------------------------------------------------------
def test_resident_rows_at_4096_bins_are_the_fetched_rows(eng):
    """After (a)'s launch at nbin = 4096, gauss_normal on the resident rows is gauss_normal on the fetched rows, bit
    for bit."""
    c = gr.case("rows", 4096, "011")
    r = c.reference()
    h = np.array([0.3, 0.05, 1e-3])
    eng.gauss_fit_begin(r["data"], c.freqs, c.errs)
    try:
        got = _launch(eng, c)
        a = eng.gauss_normal(h)
        b = eng.gauss_normal(h, rows=got.reshape(len(c.sets), -1))
    finally:
        eng.gauss_fit_end()
    _hold_rows(c, got, "resident")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0] > 0 and np.all(np.isfinite(a[2]))
    MEASURED.setdefault("resident", {})[c.name]["normal_deviation"] = 0.0
