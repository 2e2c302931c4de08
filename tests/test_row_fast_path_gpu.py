"""The short row top of k_xspec_q1024<double, false> (pp_xspec1024q.h, FASTROW) against the general row walk.

A chunk is 32 consecutive rows in the kernel's channel-major row order (row = channel * nsub + subint).  Rows 1..30 of
a chunk take the short top when the chunk is full, lies in one channel and the launch walks without mask words, an
`act` list or per-subint templates; every other row takes RowWalk::next + next_row_of as before.  Both must visit the
same rows in the same order and address the same memory, so every output is compared bit for bit.

Common shape: 2048 bins, f64 portraits, phase + DM, the example template, noise given.  Every array of
Engine.fit_batch's result and the 18-column device records are compared with assert_array_equal.

(Engine.fit_batch has no argument that hands the transform a list of subints -- XspecArgs::act is set by the driver
alone, for the re-transform of subints that need evaluations -- so the fast-against-general test has no such leg.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 2048
FLAGS = [1, 1, 0, 0, 0]


def _case(nchan, nsub, seed=5):
    """An engine holding the example template, nsub synthetic subints on the device and caller-quality guesses."""
    import torch
    from pulseportraiture_amd.engine import Engine
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.pplib import guess_fit_freq, Dconst
    e = Engine(0)
    freqs, model, P0 = gmodel.example_model(nchan, B)
    e.set_model(model)
    rng = np.random.default_rng(seed)
    P = np.full(nsub, P0)
    inj = np.zeros((nsub, 3))
    inj[:, 0] = rng.uniform(-0.5, 0.5, nsub)
    inj[:, 1] = 34.56789 + rng.normal(3e-4, 2e-4, nsub)
    data = torch.empty((nsub, nchan, B), dtype=torch.float64, device="cuda:0")
    e.synth_portraits(data, freqs, P, inj, 0.05, 20260101 + seed, 0)
    nu_fit = float(guess_fit_freq(freqs))
    x0 = np.zeros((nsub, 5))
    x0[:, 0] = (inj[:, 0] + Dconst * inj[:, 1] / P / nu_fit ** 2 + 1e-4 * rng.standard_normal(nsub) + 0.5) % 1.0 - 0.5
    x0[:, 1] = 34.56789
    kw = dict(errs=np.full((nsub, nchan), 0.05), nu_fits=np.full((nsub, 3), nu_fit), fit_flags=FLAGS)
    return e, data, freqs, P, x0, kw


def _rows(kw, sl):
    """The per-subint arguments of kw for the subints sl."""
    return {k: (v[sl] if isinstance(v, np.ndarray) and k in ("errs", "nu_fits", "chan_mask") else v) for k, v in kw.items()}


def _fit(e, data, freqs, P, x0, kw):
    """fit_batch with device records: (its result, the records)."""
    import torch
    rec = torch.zeros((data.shape[0], 18), dtype=torch.float64, device="cuda:0")
    return e.fit_batch(data, freqs, P, x0, records=rec, **kw), rec


def _arrays(r, rec):
    out = {"records": rec.cpu().numpy()}
    for k, v in r.items():
        if hasattr(v, "cpu"):
            out[k] = v.cpu().numpy()
        elif isinstance(v, np.ndarray):
            out[k] = v
    assert {"params", "param_errs", "chi2", "nfeval", "scales"} <= set(out)
    return out


def _same(a, b, what=""):
    assert set(a) == set(b)
    for k in sorted(a):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))


def _one_by_one(e, data, freqs, P, x0, kw):
    """The batch fitted one subint per call, stacked."""
    parts = []
    for j in range(data.shape[0]):
        sl = slice(j, j + 1)
        parts.append(_arrays(*_fit(e, data[sl], freqs, P[sl], x0[sl], _rows(kw, sl))))
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def test_full_chunks_short_top_equals_general_walk():
    """3 channels x 64 subints: six full single-channel chunks.  Without a mask rows 1..30 of every chunk take the short
    top; with an all-ones chan_mask the launch carries mask words and every row takes the general walk."""
    e, data, freqs, P, x0, kw = _case(3, 64)
    fast = _arrays(*_fit(e, data, freqs, P, x0, kw))
    general = _arrays(*_fit(e, data, freqs, P, x0, dict(kw, chan_mask=np.ones((64, 3), dtype=np.uint8))))
    e.close()
    assert np.isfinite(fast["params"][:, :2]).all()
    _same(fast, general, "no mask / all-ones mask")


@pytest.mark.parametrize("nchan,nsub", [(3, 33), (2, 1)])
def test_chunk_edges_equal_subints_one_by_one(nchan, nsub):
    """3 x 33: 99 rows, chunks that straddle channels (33 is no multiple of 32) and a ragged last chunk -- no chunk may
    take the short top past a channel's end.  2 x 1: two rows, one ragged chunk."""
    e, data, freqs, P, x0, kw = _case(nchan, nsub, seed=7)
    whole = _arrays(*_fit(e, data, freqs, P, x0, kw))
    single = _one_by_one(e, data, freqs, P, x0, kw)
    e.close()
    _same(whole, single, "%d x %d" % (nchan, nsub))


def test_full_partial_and_empty_chunks_in_one_launch():
    """4 channels x 64 subints (eight chunks); the mask removes channel 1 of subint 40 (a partial chunk) and channel 2
    of subints 0..31 (an empty chunk).  Against per-subint calls with the same mask rows."""
    e, data, freqs, P, x0, kw = _case(4, 64, seed=9)
    mask = np.ones((64, 4), dtype=np.uint8)
    mask[40, 1] = 0
    mask[:32, 2] = 0
    kwm = dict(kw, chan_mask=mask)
    whole = _arrays(*_fit(e, data, freqs, P, x0, kwm))
    single = _one_by_one(e, data, freqs, P, x0, kwm)
    # ... and the unmasked batch (short tops) agrees with the masked one wherever the mask took nothing away
    plain = _arrays(*_fit(e, data, freqs, P, x0, kw))
    e.close()
    _same(whole, single, "masked")
    untouched = np.r_[32:40, 41:64]
    for k in ("params", "param_errs", "chi2", "nfeval", "scales", "records"):
        np.testing.assert_array_equal(plain[k][untouched], whole[k][untouched], err_msg="untouched subints " + k)


def test_enqueued_launches_equal_synchronous_ones():
    """Three batches of 64 channels x 32 subints through enqueue / collect: the second and third transform carry the
    previous batch's solve as tail tickets (tail_work between two rows, after which the chunk in hand is finished by
    general rows).  Against three synchronous fit_batch calls."""
    import torch
    e, data, freqs, P, x0, kw = _case(64, 32, seed=11)
    batches = [(data, x0)]
    for s in (1, 2):
        d = torch.roll(data, shifts=s, dims=0).contiguous()
        batches.append((d, np.roll(x0, s, axis=0)))
    sync = [_arrays(*_fit(e, d, freqs, P, x, kw)) for d, x in batches]
    recs = []
    for d, x in batches:
        rec = torch.zeros((32, 18), dtype=torch.float64, device="cuda:0")
        e.enqueue(d, freqs, P, x, records=rec, **kw)
        recs.append(rec)
    got = [_arrays(e.collect(), rec) for rec in recs]
    e.close()
    for j, (a, b) in enumerate(zip(sync, got)):
        _same(a, b, "batch %d" % j)
    np.testing.assert_array_equal(sync[1]["params"], np.roll(sync[0]["params"], 1, axis=0))
