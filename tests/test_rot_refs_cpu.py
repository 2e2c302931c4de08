"""tests/rot_refs.py pinned before anything on a GPU is judged by it: the long-double rotation against the oracle's
NumPy rotation (whose own distance, the rounding of k * phi, is printed and must stay under the GPU bars that stand on
it) and against closed forms; the time-domain chi^2 and the phase-fit columns against the reference's fixtures; and
every decision precondition of tests/test_gpu_rot_kernels.py, on the inputs that file uses."""
import os

import numpy as np
import pytest

from oracle import pptoas_oracle as orc
from tests import rot_refs as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


# ---- the rotation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [32, 1000, 2048])
def test_rotate_ld_against_the_oracle(nbin):
    x = rr.a1_cube(nbin)[0, 0]
    for phi in (0.1234, -0.31, 1.0 / nbin, 0.5 / nbin):
        got = rr.rotate_ld(x, phi)
        dist = float(np.abs(got - orc.rotate_data(x, phi)).max() / np.abs(x).max())
        print("nbin %d phi %+.6f: NumPy's distance %.2e of the row's maximum (bar %.0e)" %
              (nbin, phi, dist, rr.rot_bar(nbin)))
        assert dist < rr.rot_bar(nbin)
        if abs(phi) < 0.01:
            assert dist < 2e-15         # whole and half bins: k phi is exact in f64 at a power of two, ~1 ulp else


@pytest.mark.parametrize("nbin", rr.ALL)
def test_oracle_distance_on_the_gpu_inputs(nbin):
    """The rows the GPU file holds to the oracle alone: NumPy's distance from the long-double rows of the same cube,
    which bounds what the oracle takes of the A1 bar there."""
    x, phis = rr.a1_cube(nbin), rr.a1_phis(nbin)
    worst = 0.0
    for (i, n), want in rr.a1_reference(nbin).items():
        o = orc.rotate_data(x[i, n], phis[i])
        worst = max(worst, float(np.abs(want - o).max() / np.abs(x[i, n]).max()))
    print("nbin %d: NumPy's distance %.2e of the row's maximum (bar %.0e)" % (nbin, worst, rr.rot_bar(nbin)))
    assert worst < rr.rot_bar(nbin)


@pytest.mark.parametrize("nbin", [8, 32, 62, 250, 1000, 2048])
def test_closed_forms(nbin):
    """Exact to long-double rounding: a DC row is unchanged; a pure Nyquist row turned by half a bin is zero and by one
    bin is negated; cos(2 pi k j / nbin) turned by phi is the cosine moved by phi to earlier phase, k = 1 and M - 1."""
    M = nbin // 2
    tol = 64 * nbin * LD_EPS
    dc = np.full(nbin, 1.5)
    assert np.abs(rr.rotate_ld(dc, 0.1234) - 1.5).max() < tol
    alt = np.where(np.arange(nbin) % 2 == 0, 1.0, -1.0)
    # (0.5 / nbin is exact in f64 only at a power of two: the expectation carries the f64 value's own M phi)
    half = np.cos(rr.PI2 * rr.turns_ld(np.array([M]), 0.5 / nbin)[0])
    assert abs(float(half)) < 1e-15
    assert np.abs(rr.rotate_ld(alt, 0.5 / nbin) - half * alt).max() < tol
    one = np.cos(rr.PI2 * rr.turns_ld(np.array([M]), 1.0 / nbin)[0])
    assert abs(float(one) + 1) < 1e-15
    assert np.abs(rr.rotate_ld(alt, 1.0 / nbin) - one * alt).max() < tol
    j = np.arange(nbin, dtype=LD)
    for k in (1, M - 1):
        for phi in (0.1234, -0.31):
            row = rr._cos_ld(nbin, k, 0.0)          # a long-double row: no f64 rounding of the input
            want = np.cos(rr.PI2 * ((j * k / nbin) % 1 + rr.turns_ld(np.array([k]), phi)[0]))
            got = rr.irfft_ld(*_rot_spec(row, phi), nbin)
            assert np.abs(got - want).max() < tol, (k, phi)


def _rot_spec(row, phi):
    re, im = rr.rfft_ld(row)
    c, s = rr.phasor_ld(np.arange(len(re)), phi)
    return re * c - im * s, re * s + im * c


@pytest.mark.parametrize("nbin", [8, 250, 2048])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_rows_builder(nbin, dtype):
    """a2_rows' expectations (closed form + the rotated rounding residual) are what rotate_ld gives of the rows."""
    rows, want = rr.a2_rows(nbin, dtype)
    phis = rr.a2_phis(nbin)
    for i in range(len(rows)):
        got = rr.rotate_ld(rows[i, 0].astype(np.float64), phis[i])
        assert np.abs(got - want[i, 0]).max() < 1e-17 * nbin, (rr.A2_NAMES[i], float(np.abs(got - want[i, 0]).max()))
        assert np.array_equal(want[i, 1], -2 * want[i, 0])
    assert np.abs(want[2]).max() < 1e-15 and not rows[6].any() and not want[6].any()


def test_delay_law_builder():
    """|phi_n| < 2 everywhere, the f64 oracle's phase_shifts within u of the long-double delay, and an infinite
    reference frequency contributes nothing."""
    for nu_DM, nu_GM in rr.A3_REFS:
        phin, u = rr.a3_delays(nu_DM, nu_GM)
        assert np.abs(phin).max() < 2
        fr = rr.a3_freqs()
        for i in range(3):
            o = orc.phase_shifts(rr.A3_PHI[i], rr.A3_DM[i], rr.A3_GM[i], fr[i], nu_DM, nu_GM, rr.A3_P[i])
            assert np.all(np.abs(o - phin[i]) <= u[i])
    t = rr.delay_terms_ld(0.1, 3e-3, 0.2, 1400.0, np.inf, np.inf, 0.005)
    assert t[2] == 0 and t[4] == 0 and t[1] > 0 and t[3] > 0
    assert np.any(phin != rr.a3_delays(1400.0, 1300.0)[0])


# ---- the per-channel chi^2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fpf_64x256_phiDM", "fpf_64x256_phiDMGM", "fpf_64x256_scat_lin"])
def test_chan_red_chi2_ld_against_the_fixtures(name):
    g = _load(name)
    tau = float(g["out_tau"])
    if bool(g["log10_tau"]) and int(g["fit_flags"][3]):
        tau = 10.0 ** tau
    phi, DM, GM, alpha = (float(g[k]) for k in ("out_phi", "out_DM", "out_GM", "out_alpha"))
    nu_refs = [float(g[k]) for k in ("out_nu_DM", "out_nu_GM", "out_nu_tau")]
    P, freqs = float(g["P"]), g["freqs"]
    want = orc.channel_red_chi2s(g["data"], g["model"], phi, DM, GM, tau, alpha, freqs, nu_refs, P, g["out_scales"],
                                 g["errs"])
    for n in (0, 17, 40, 63):
        phin = float(rr.delay_ld(phi, DM, GM, freqs[n], nu_refs[0], nu_refs[1], P))
        taun = tau * (freqs[n] / nu_refs[2]) ** alpha if tau != 0 else 0.0
        got = rr.chan_red_chi2_ld(g["data"][n], g["model"][n], phin, taun, g["out_scales"][n], g["errs"][n])
        np.testing.assert_allclose(float(got), want[n], rtol=1e-10)


def _b_oracle(c):
    return np.stack([orc.channel_red_chi2s(c["data"][i], c["templates"][rr.B_SLOTS[i]], *c["params"][i], c["freqs"][i],
                                           c["nu_refs"][i], c["P"][i], c["scales"][i], c["sigma"][i])
                     for i in range(rr.B_NSUB)])


@pytest.mark.parametrize("nbin", rr.ALL)
def test_chi2_case_preconditions(nbin):
    """chi^2 near 1 on the regular channels, the zero-scale channel equal to sum data^2 / sigma^2 / (nbin - 2), the
    negative scale in place, and the oracle within 1e-10 of the long-double rows (which leaves the device its bar)."""
    c = rr.b1_case(nbin)
    want = _b_oracle(c)
    regular = np.ones(want.shape, dtype=bool)
    regular[1, 2] = regular[2, 3] = False
    assert 0.5 < np.median(want[regular]) < 2, np.median(want[regular])
    assert c["scales"][1, 2] < 0 and c["scales"][2, 3] == 0
    np.testing.assert_allclose(want[2, 3], rr.zero_scale_chi2(c["data"][2, 3], c["phin"][2, 3], c["sigma"][2, 3]),
                               rtol=1e-11)
    assert np.all(c["taun"][3] > 0) and not c["taun"][:3].any()
    for p, v in rr.b1_reference(nbin).items():
        rel = abs(float(v) - want[p]) / float(v)
        print("nbin %d row %s: oracle's distance %.2e" % (nbin, p, rel))
        assert rel < 0.5e-10


# ---- the 1-D phase fit ---------------------------------------------------------------------------------------
def test_fps_columns_against_the_fixture():
    g = _load("fit_phase_shift_256")
    for row in g["rows"]:
        shift, noise = row[0], (None if np.isnan(row[1]) else row[1])
        d = orc.rotate_data(g["prof"], -shift)
        for ld in (True, False):
            got = rr.fps_columns(d, g["model_prof"], noise, row[2], ld=ld)
            np.testing.assert_allclose(got.astype(np.float64), row[3:], rtol=1e-9)
        # NaN and a negative noise are "missing" too
        np.testing.assert_array_equal(rr.fps_columns(d, g["model_prof"], None, row[2]),
                                      rr.fps_columns(d, g["model_prof"], np.nan, row[2]))
        np.testing.assert_array_equal(rr.fps_columns(d, g["model_prof"], None, row[2]),
                                      rr.fps_columns(d, g["model_prof"], -1.0, row[2]))


@pytest.mark.parametrize("nbin", [32, 1000])
def test_fps_objective_derivatives(nbin):
    """f' and f'' are the derivatives of f (central differences in long double), and f is the oracle's function."""
    data, model, _ = rr.c_case(nbin)
    h = LD(2) ** -30                    # (phi +- h is exact in f64; truncation (2 pi M h)^2 ~ 1e-11, rounding ~ 1e-10)
    k, xr, xi, _, _ = rr._cross(data[0], model[0], True)
    s1 = rr.PI2 * np.sum(k * np.hypot(xr, xi))
    s2 = rr.PI2 ** 2 * np.sum(k * k * np.hypot(xr, xi))
    for phi in (0.1234, -0.31):
        f, f1, f2 = rr.fps_objective_ld(data[0], model[0], phi)
        fp, f1p, _ = rr.fps_objective_ld(data[0], model[0], phi + float(h))
        fm, f1m, _ = rr.fps_objective_ld(data[0], model[0], phi - float(h))
        assert abs((fp - fm) / (2 * h) - f1) < 1e-8 * s1
        assert abs((f1p - f1m) / (2 * h) - f2) < 1e-8 * s2
        dF, mF = np.fft.rfft(data[0]), np.fft.rfft(model[0])
        dF[0] = mF[0] = 0
        np.testing.assert_allclose(float(f), orc.fit_phase_shift_function(phi, mF, dF, 1.0), rtol=1e-11)
        np.testing.assert_allclose(float(f2), orc.fit_phase_shift_function_2deriv(phi, mF, dF, 1.0), rtol=1e-11)


@pytest.mark.parametrize("nbin", rr.C_NBINS)
def test_fps_grid_preconditions(nbin):
    """The grid decision does not hang on rounding: the best point leads by more than 1e-9 of |f| for every pair,
    bounds and Ns the GPU file uses; with bounds (-0.5, 0.5) the two ends are one phase and tie exactly, so the lower
    index stands for both (with Ns = 2 index 0 wins, with Ns = 1 the start is lo)."""
    for i in range(5):
        assert rr.c_ends_tie(nbin, i, *rr.C_BOUNDS["tie"])
        for kind, (lo, hi) in rr.C_BOUNDS.items():
            for Ns in sorted(set(rr.C_NS(nbin))):
                best, lead = rr.c_grid_margin(nbin, i, lo, hi, Ns)
                assert lead > 1e-9, (kind, Ns, i, best, lead)
                if Ns <= 2 and kind == "tie":
                    assert best == 0
    data, model, sigma = rr.c_case(nbin)
    assert data.shape == (5, nbin) and np.all(sigma > 0)
