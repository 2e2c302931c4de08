"""The row loop of the headline transform kernel, k_xspec_q1024<double, false>, on a batch that takes both of its row
tops and every slot of its slot loop.

16 channels x 2048 bins (f64), 40 subints, noise given, (phi, DM): every channel is one full chunk of 32 rows -- rows
1..30 of it take the short row top -- and a ragged chunk of 8 rows on the general top.  The portraits are made on the
host (NumPy's Generator), so nothing but the fit itself runs on the code under test.

(a) bits: params, param_errs, chi2, scales and nfeval against tests/golden/headline_rows_bits.npz, recorded by
    tests/golden/make_golden_headline_rows_bits.py from the build BEFORE the row loop's selects, moves and lane index
    arithmetic were reworked.  Changes to that loop that touch no f64 operation leave every bit where it was; the
    fixture is never regenerated from the code under test.
(b) the lane that owns lambda = 0: a template whose only power is at harmonics 1 and 64, 128, .., 448 -- all but the
    first live in that one lane, which takes them from its registers 1..7 -- against the general kernel
    (one_exchange = 0) and against the oracle on one subint."""
import os

import numpy as np
import pytest

from tests.gpu_support import eng  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLDEN, "headline_rows_bits.npz")
PHI_BAR, DM_BAR = 1e-9, 1e-6          # (tests/test_gpu_parity.py)
C, B, NSUB = 16, 2048, 40
NSL = 7                               # slots of 64 harmonics in the headline kernel's slot loop
DM0, SIGMA = 34.56789, 0.05
BITWISE = ("params", "param_errs", "chi2", "scales", "nfeval")


def _portraits(model, freqs, P0, nu_fit, seed):
    """(data [NSUB, C, B] f64, x0 [NSUB, 5]): the template rotated by a phase and a DM per subint + white noise."""
    from oracle import pptoas_oracle as orc
    rng = np.random.default_rng(seed)
    shift = rng.uniform(-0.45, 0.45, NSUB)
    dm = DM0 + rng.normal(3e-4, 2e-4, NSUB)
    data = np.array([orc.rotate_data(model, -shift[i], -dm[i], P0, freqs, nu_fit) for i in range(NSUB)])
    data += SIGMA * rng.standard_normal(data.shape)
    x0 = np.zeros((NSUB, 5))
    x0[:, 0] = (shift + 1e-4 * rng.standard_normal(NSUB) + 0.5) % 1.0 - 0.5
    x0[:, 1] = DM0
    return np.ascontiguousarray(data), x0


def _fit_kw(nu_fit):
    return dict(errs=np.full((NSUB, C), SIGMA), nu_fits=np.full((NSUB, 3), nu_fit), fit_flags=[1, 1, 0, 0, 0])


def set_example_template(e):
    """The example template at C x B with a cut at which the headline kernel serves it (2 Kt < 1024) and at least one
    channel keeps all seven slots (Kt = 448); returns (freqs, model, P0, harm_eps).  The engine's default harm_eps
    is lowered by factors of four until a channel keeps the seventh slot (the caller restores the option)."""
    from pulseportraiture_amd import gmodel
    freqs, model, P0 = gmodel.example_model(C, B)
    eps = e.get_option("harm_eps")
    for _ in range(40):
        e.set_option("harm_eps", eps)
        nharm = e.set_model(model)
        if nharm >= 64 * NSL:
            break
        eps *= 0.25
    assert 2 * nharm < B // 2 and nharm == 64 * NSL, (nharm, eps)
    return freqs, model, P0, eps


def headline_rows_batch(e):
    """Part (a)'s fit on engine `e`: the result dict and the harm_eps it was made with."""
    from pulseportraiture_amd.pplib import guess_fit_freq
    eps0 = e.get_option("harm_eps")
    try:
        freqs, model, P0, eps = set_example_template(e)
        nu_fit = float(guess_fit_freq(freqs))
        data, x0 = _portraits(model, freqs, P0, nu_fit, 20481640)
        r = e.fit_batch(data, freqs, np.full(NSUB, P0), x0, **_fit_kw(nu_fit))
    finally:
        e.set_option("harm_eps", eps0)
    return r, eps


def test_headline_rows_are_bitwise_what_the_parent_build_computed(eng):
    g = np.load(FIXTURE)
    r, eps = headline_rows_batch(eng)
    # (the cut the fixture was recorded at: the same slots are kept)
    assert eps == float(g["harm_eps"]), (eps, float(g["harm_eps"]))
    for k in BITWISE:
        np.testing.assert_array_equal(r[k], g[k], err_msg=k)


def lane0_template():
    """A C x B template with power at harmonics 1 and 64 j (j = 1..7) alone, amplitudes and phases differing from
    channel to channel."""
    rng = np.random.default_rng(64)
    t = np.arange(B) / float(B)
    model = np.empty((C, B))
    for n in range(C):
        row = np.cos(2.0 * np.pi * (t - 0.3))
        for j in range(1, NSL + 1):
            row += rng.uniform(0.3, 1.0) * np.cos(2.0 * np.pi * (64 * j * t + rng.uniform(0.0, 1.0)))
        model[n] = rng.uniform(0.8, 1.2) * row
    return model


def test_lane_zero_harmonics_match_general_kernel_and_oracle(eng):
    from oracle import pptoas_oracle as orc
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.pplib import guess_fit_freq
    e = eng
    freqs, _, P0 = gmodel.example_model(C, B)
    model = lane0_template()
    nu_fit = float(guess_fit_freq(freqs))
    data, x0 = _portraits(model, freqs, P0, nu_fit, 64448)
    P = np.full(NSUB, P0)
    kw = _fit_kw(nu_fit)
    # (the cosines' rounding residue at the other harmonics, ~1e-16 of the lines, is above the default cut of 2^-50)
    with e.options(harm_eps=1e-12):
        assert e.set_model(model) == 64 * NSL      # every channel keeps all seven slots, 2 Kt < 1024
        with e.options(one_exchange=0):
            a = e.fit_batch(data, freqs, P, x0, **kw)
        b = e.fit_batch(data, freqs, P, x0, **kw)
    dphi = np.abs((a["params"][:, 0] - b["params"][:, 0] + 0.5) % 1.0 - 0.5)
    ddm = np.abs(a["params"][:, 1] - b["params"][:, 1])
    print("one_exchange 1 against 0: max |dphi| %.3e  max |dDM| %.3e  max chi2 rel %.3e" %
          (dphi.max(), ddm.max(), np.max(np.abs(b["chi2"] / a["chi2"] - 1.0))))
    assert dphi.max() < PHI_BAR
    assert ddm.max() < DM_BAR
    np.testing.assert_allclose(b["chi2"], a["chi2"], rtol=1e-11)
    i = 3
    o = orc.fit_portrait_full(data[i], model, x0[i], P[i], freqs, [nu_fit] * 3, [None] * 3, kw["errs"][i],
                              [1, 1, 0, 0, 0], log10_tau=False)
    dpo = abs(b["params"][i, 0] - o.phi)
    dpo = min(dpo, abs(dpo - 1.0))
    print("against the oracle, subint %d: |dphi| %.3e  |dDM| %.3e  chi2 rel %.3e" %
          (i, dpo, abs(b["params"][i, 1] - o.DM), abs(b["chi2"][i] / o.chi2 - 1.0)))
    assert dpo < PHI_BAR and abs(b["params"][i, 1] - o.DM) < DM_BAR
    np.testing.assert_allclose(b["chi2"][i], o.chi2, rtol=1e-10)
    np.testing.assert_allclose(b["scales"][i], o.scales, rtol=1e-7, atol=1e-9)
