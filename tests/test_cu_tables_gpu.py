"""k_xspec_cu1024 (engine option cu_tables, default 1) against k_xspec_q1024<double, false> (cu_tables = 0), bit for bit.

The new kernel is the old row with the stage-1 twiddle powers and the split-twiddle steps read from LDS tables that
the CU's eight waves share; the tables are filled once with the operations the row used, so every f64 result is the
same.  What can go wrong is around that: a wave's identity in the walk, waves that have no row, the lane that owns
lambda = 0, the tables after a ticket (the previous batch's solve and post-fit stage inside the kernel), and the
dispatch -- masked batches and batches whose noise is measured stay on the old kernels.

Portraits are made on the host as in tests/test_headline_rows_bits.py; every case is a few small fits."""
import numpy as np
import pytest

from tests.gpu_support import eng  # noqa: F401
from tests.test_headline_rows_bits import lane0_template, set_example_template

pytestmark = pytest.mark.gpu

B = 2048
DM0, SIGMA = 34.56789, 0.05
BITWISE = ("params", "param_errs", "chi2", "scales", "nfeval")


def _portraits(model, freqs, P0, nu_fit, nsub, seed):
    """(data [nsub, C, B] f64, x0 [nsub, 5]): the template rotated by a phase and a DM per subint + white noise."""
    from oracle import pptoas_oracle as orc
    rng = np.random.default_rng(seed)
    shift = rng.uniform(-0.45, 0.45, nsub)
    dm = DM0 + rng.normal(3e-4, 2e-4, nsub)
    data = np.array([orc.rotate_data(model, -shift[i], -dm[i], P0, freqs, nu_fit) for i in range(nsub)])
    data += SIGMA * rng.standard_normal(data.shape)
    x0 = np.zeros((nsub, 5))
    x0[:, 0] = (shift + 1e-4 * rng.standard_normal(nsub) + 0.5) % 1.0 - 0.5
    x0[:, 1] = DM0
    return np.ascontiguousarray(data), x0


def _batch(model, freqs, P0, nsub, seed):
    """Arguments of fit_batch for `nsub` portraits of `model`: (data, freqs, P, x0), keywords."""
    from pulseportraiture_amd.pplib import guess_fit_freq
    nu_fit = float(guess_fit_freq(freqs))
    data, x0 = _portraits(model, freqs, P0, nu_fit, nsub, seed)
    kw = dict(errs=np.full((nsub, len(freqs)), SIGMA), nu_fits=np.full((nsub, 3), nu_fit), fit_flags=[1, 1, 0, 0, 0])
    return (data, freqs, np.full(nsub, P0), x0), kw


def _both(e, args, kw):
    """The fit with cu_tables = 0 and with cu_tables = 1."""
    with e.options(cu_tables=0):
        a = e.fit_batch(*args, **kw)
    with e.options(cu_tables=1):
        b = e.fit_batch(*args, **kw)
    return a, b


def _assert_same(a, b, what):
    for k in BITWISE:
        np.testing.assert_array_equal(b[k], a[k], err_msg="%s: %s" % (what, k))


@pytest.fixture(scope="module")
def example16(eng):
    """16 channels x 40 subints of the example template (a full chunk on the short row top and a ragged chunk per
    channel), made once: (args, kw, model)."""
    from pulseportraiture_amd import gmodel
    freqs, model, P0 = gmodel.example_model(16, B)
    args, kw = _batch(model, freqs, P0, 40, 20481640)
    return args, kw, model


def test_option_is_on_by_default(eng):
    assert eng.get_option("cu_tables") == 1
    assert eng.get_option("cu_grid_cap") == 0


def test_all_seven_slots_and_one_slot(eng, example16):
    """The cut of tests/test_headline_rows_bits.py, at which a channel keeps all seven slots (every table row of the
    split twiddle is read), and a cut that keeps one slot (none but the first)."""
    args, kw, model = example16
    eps0 = eng.get_option("harm_eps")
    try:
        set_example_template(eng)
        a, b = _both(eng, args, kw)
        _assert_same(a, b, "seven slots")
        eps, nharm = eps0, 0
        for _ in range(40):
            eng.set_option("harm_eps", eps)
            nharm = eng.set_model(model)
            if nharm <= 64:
                break
            eps *= 4.0
        assert nharm == 64, (nharm, eps)
        a, b = _both(eng, args, kw)
        _assert_same(a, b, "one slot")
    finally:
        eng.set_option("harm_eps", eps0)


@pytest.mark.parametrize("C,nsub", [(3, 1), (9, 33)])
def test_fewer_rows_than_waves_and_ragged_chunks(eng, C, nsub):
    """3 rows: one wave has work, the others -- seven of the same workgroup among them -- pass the barrier and leave.
    9 x 33: every channel is a full chunk and a chunk of one row, and the channel count is no multiple of eight."""
    from pulseportraiture_amd import gmodel
    freqs, model, P0 = gmodel.example_model(C, B)
    assert 2 * eng.set_model(model) < B // 2         # (the headline kernels' template cut)
    args, kw = _batch(model, freqs, P0, nsub, 1000 * C + nsub)
    a, b = _both(eng, args, kw)
    _assert_same(a, b, "%d x %d" % (C, nsub))


def test_lane_zero_harmonics(eng):
    """Power at harmonics 1 and 64 j alone: all but the first live in the lane that owns lambda = 0, whose split
    twiddle starts at W^64."""
    from pulseportraiture_amd import gmodel
    freqs, _, P0 = gmodel.example_model(16, B)
    model = lane0_template()
    with eng.options(harm_eps=1e-12):
        assert eng.set_model(model) == 64 * 7
        args, kw = _batch(model, freqs, P0, 40, 64448)
        a, b = _both(eng, args, kw)
    _assert_same(a, b, "lane 0")


@pytest.mark.parametrize("cap", [1, 0])
def test_tables_survive_the_tail_inside_the_kernel(eng, example16, cap):
    """Three batches enqueued three deep with fuse_tail on: the second and third transform work off their predecessor's
    solve and post-fit stage as tickets, in the waves' own images.  Against the three fitted synchronously by
    k_xspec_q1024.
    cap = 1 (option cu_grid_cap: ONE workgroup): 640 rows are 20 chunks for eight waves, so every wave has two or
    three chunks and asks for its ticket after 1 .. 61 of its ~80 rows (ticket_moment: share = 640 / 8 + 1) -- the ticket
    runs BETWEEN two rows, t2 is put back into the image behind it and the rows after it read the tables again.
    cap = 0 (one workgroup per CU): most waves have no row and take the tickets on their way out."""
    args, kw, model = example16
    assert 2 * eng.set_model(model) < B // 2
    data, freqs, P, x0 = args
    rng = np.random.default_rng(3)
    jobs = [data, data + 0.01 * rng.standard_normal(data.shape), data[::-1].copy()]
    xs = [x0, x0, x0[::-1].copy()]
    with eng.options(cu_tables=0, fuse_tail=0):
        sync = [eng.fit_batch(d, freqs, P, x, **kw) for d, x in zip(jobs, xs)]
    got = []
    with eng.options(cu_tables=1, fuse_tail=1, cu_grid_cap=cap):
        for d, x in zip(jobs, xs):
            eng.enqueue(d, freqs, P, x, **kw)
        for _ in jobs:
            got.append(eng.collect())
    for j, (a, g) in enumerate(zip(sync, got)):
        _assert_same(a, g, "cap %d, enqueued batch %d" % (cap, j))


def test_masked_and_measured_noise_batches_stay_on_the_old_kernels(eng, example16):
    """A channel mask and errs = None are not the new kernel's cases: the same results whatever cu_tables says."""
    args, kw, model = example16
    assert 2 * eng.set_model(model) < B // 2
    nsub, C = kw["errs"].shape
    mask = (np.random.default_rng(5).random((nsub, C)) > 0.2).astype(np.uint8)
    a, b = _both(eng, args, dict(kw, chan_mask=mask))
    _assert_same(a, b, "masked")
    a, b = _both(eng, args, dict(kw, errs=None))
    _assert_same(a, b, "errs = None")
