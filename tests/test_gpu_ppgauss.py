"""ppgauss on the device against the TRUE reference (tests/golden/make_golden_ppgauss.py).

The reference fits with lmfit, which could not be run; the goldens pin the fit in two parts.  The objective is the
reference's own (fit_gaussian_portrait_function, gen_gaussian_portrait, ...).  Its minimum does not depend on the
optimiser: every golden fit was solved twice (MINPACK behind lmfit's bound transforms, and scipy's trf), and the
difference between the two solves in units of the 1-sigma errors -- the reference's self-scatter -- is stored.

Bars
  residual rows   the standing device-vs-host portrait bar (2e-14 max|model|) over sigma_n, plus one ulp of
                  |data| / sigma_n
  normal equations  nrow 2^-53 sum|terms| per entry against math.fsum: the bound of a recursive sum of correctly
                  rounded terms (derived, not tuned)
  fits            every parameter within 1e-3 of its golden 1 sigma, chi2 <= golden chi2 (1 + 1e-9), fit_errs within
                  1e-4; and every parameter within 10 x the recorded self-scatter, taken as the largest over the
                  parameters (one parameter's difference between two solves is a single draw and can be near zero
                  by chance; the largest is what the two reference solves guarantee of each other)
With PP_PPGAUSS_PARITY_OUT set, the achieved distances are written there as JSON (profiles/ppgauss_parity.json)."""
import math
import os

import numpy as np
import pytest

from tests.gpu_support import eng, measured_writer, run_module  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MEASURED, _write_measured = measured_writer("PP_PPGAUSS_PARITY_OUT")
PHI_BAR, DM_BAR = 1e-9, 1e-6        # the legacy fit_portrait golden test's bars (tests/test_gpu_parity.py)


def _g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _set_args(sets, nbin):
    sets = np.atleast_2d(sets)
    ng = (sets.shape[1] - 3) // 6
    return sets[:, 0], sets[:, 1] / nbin, sets[:, -1], sets[:, 2:-1].reshape(len(sets), ng, 6)


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_residual_rows_against_the_reference(eng, nbin, code, scattered):
    """fit_gaussian_portrait_function of the five-component edge model (wrap at phase 0/1, loc outside [0,1), a
    non-positive width), 1, 2 and 9 parameter sets per launch; the 9 sets step DC, tau, a loc, a loc slope, a wid, an
    amp, an amp index and the scattering index, so one launch holds sets that differ in tau and in alpha."""
    g = _g("ppgauss_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    sets, want = g[tag + "_sets"], g[tag + "_rows"].reshape(9, 3, nbin)
    data, errs, freqs = g["n%d_data" % nbin], g["n%d_errs" % nbin], g["n%d_freqs" % nbin]
    eng.gauss_fit_begin(data, freqs, errs)
    try:
        worst = 0.0
        for pick in ([0], [0, 2], list(range(9)), [1, 7, 0]):
            got = eng.gauss_residuals(code, float(g["nu_ref"]), *_set_args(sets[pick], nbin), fetch=True)
            assert got.shape == (len(pick), 3, nbin)
            model = data[None] - want[pick] * errs[None, :, None]
            bar = 2e-14 * np.abs(model).max() / errs + np.spacing(np.abs(data).max(axis=1) / errs)
            dev = np.abs(got - want[pick])
            worst = max(worst, float((dev / bar[None, :, None]).max()))
            assert np.all(dev <= bar[None, :, None]), (tag, pick, float((dev / bar[None, :, None]).max()))
        MEASURED.setdefault("residual_rows", {})[tag] = dict(of_bar=worst)
        print(tag, "worst deviation %.3f of the bar" % worst)
    finally:
        eng.gauss_fit_end()


def _cancelling_rows(nsets, nrow, seed):
    """R_0 of unit scale and R_a = R_0 + h_a D_a with h_a ~ 1e-7: R_a - R_0 loses seven digits."""
    rng = np.random.default_rng(seed)
    R0 = rng.standard_normal(nrow)
    h = 1e-7 * (1.0 + rng.uniform(size=nsets - 1))
    R = np.empty((nsets, nrow))
    R[0] = R0
    for a in range(1, nsets):
        R[a] = R0 + h[a - 1] * rng.standard_normal(nrow) * (1.0 + a)
    return R, h


def _fsum_reference(R, h):
    """The kernel's terms -- V_0 = R_0, V_a = (R_a - R_0) / h_a, each product rounded -- summed exactly."""
    V = np.vstack([R[:1], (R[1:] - R[0]) / h[:, None]]) if len(R) > 1 else R[:1]
    n = len(V)
    S, A = np.empty((n, n)), np.empty((n, n))
    for a in range(n):
        for b in range(a, n):
            t = V[a] * V[b]
            S[a, b] = S[b, a] = math.fsum(t)
            A[a, b] = A[b, a] = math.fsum(np.abs(t))
    return S, A


@pytest.mark.parametrize("nsets", [1, 2, 100])
@pytest.mark.parametrize("nrow", [3 * 64, 5 * 100])
def test_normal_equations_on_supplied_rows(eng, nsets, nrow):
    R, h = _cancelling_rows(nsets, nrow, 1000 * nsets + nrow)
    chi2, gvec, G = eng.gauss_normal(h, rows=R)
    S, A = _fsum_reference(R, h)
    bar = nrow * 2.0 ** -53 * A
    assert abs(chi2 - S[0, 0]) <= bar[0, 0]
    assert gvec.shape == (nsets - 1,) and G.shape == (nsets - 1, nsets - 1)
    if nsets > 1:
        assert np.all(np.abs(gvec - S[0, 1:]) <= bar[0, 1:]), float((np.abs(gvec - S[0, 1:]) / bar[0, 1:]).max())
        assert np.all(np.abs(G - S[1:, 1:]) <= bar[1:, 1:]), float((np.abs(G - S[1:, 1:]) / bar[1:, 1:]).max())
        np.testing.assert_array_equal(G, G.T)
    # the same call twice: the same bits (no floating-point atomics, a fixed summation order)
    chi2b, gb, Gb = eng.gauss_normal(h, rows=R)
    assert chi2b == chi2 and np.array_equal(gb, gvec) and np.array_equal(Gb, G)
    # rows that are already on the device give the host rows' bits
    import torch
    chi2c, gc, Gc = eng.gauss_normal(h, rows=torch.as_tensor(R, device="cuda"))
    assert chi2c == chi2 and np.array_equal(gc, gvec) and np.array_equal(Gc, G)


def test_normal_equations_of_resident_rows_repeat_bitwise(eng):
    g = _g("ppgauss_rows")
    nbin, tag = 100, "n100_c011_t1"
    sets = g[tag + "_sets"]
    eng.gauss_fit_begin(g["n100_data"], g["n100_freqs"], g["n100_errs"])
    try:
        R = eng.gauss_residuals("011", float(g["nu_ref"]), *_set_args(sets, nbin), fetch=True).reshape(9, -1)
        h = np.array([1e-3, 0.3, 1e-3, 1e-6, 1e-3, 1e-2, 1e-5, 0.05])      # the steps of the stored sets
        a = eng.gauss_normal(h)
        b = eng.gauss_normal(h)
        c = eng.gauss_normal(h, rows=R)
        for x, y in ((a, b), (a, c)):
            assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
        S, A = _fsum_reference(R, h)
        assert abs(a[0] - S[0, 0]) <= R.shape[1] * 2.0 ** -53 * A[0, 0]
    finally:
        eng.gauss_fit_end()


def test_refusals_return_messages_and_nothing_faults(eng):
    from pulseportraiture_amd.engine import EngineError
    g = _g("ppgauss_rows")
    z1 = np.zeros(1)
    eng.gauss_fit_end()         # (whatever an earlier test left resident)
    with pytest.raises(EngineError, match="pp_gauss_fit_begin first"):
        eng.gauss_residuals("000", 1500.0, z1, z1, z1, np.ones((1, 1, 6)))
    with pytest.raises(EngineError, match="no resident"):
        eng.gauss_normal(np.zeros(0), nsets=1, nrow=192)
    eng.gauss_fit_begin(g["n64_data"], g["n64_freqs"], g["n64_errs"])
    try:
        with pytest.raises(EngineError, match="no resident"):
            eng.gauss_normal(np.zeros(0))                   # begun, but no residuals yet
        with pytest.raises(EngineError, match="17 components"):
            eng.gauss_residuals("000", 1500.0, z1, z1, z1, np.full((1, 17, 6), 0.1))
        with pytest.raises(EngineError, match="101 parameter sets"):
            eng.gauss_residuals("000", 1500.0, np.zeros(101), np.zeros(101), np.zeros(101), np.full((101, 1, 6), 0.1))
        with pytest.raises(EngineError, match="101 parameter sets"):
            eng.gauss_normal(np.full(100, 1e-6), rows=np.zeros((101, 8)))
        with pytest.raises(EngineError, match="model code"):
            eng.gauss_residuals("0x0", 1500.0, z1, z1, z1, np.full((1, 1, 6), 0.1))
        with pytest.raises(EngineError, match="no noise level"):
            eng.gauss_fit_begin(g["n64_data"], g["n64_freqs"], [0.05, 0.0, 0.05])
        with pytest.raises(EngineError, match="pp_gauss_fit_begin first"):     # a refused begin leaves no fit open
            eng.gauss_residuals("000", 1500.0, z1, z1, z1, np.full((1, 1, 6), 0.1))
        # ... and the engine still works
        eng.gauss_fit_begin(g["n64_data"], g["n64_freqs"], g["n64_errs"])
        sets = g["n64_c000_t0_sets"][:1]
        got = eng.gauss_residuals("000", float(g["nu_ref"]), *_set_args(sets, 64), fetch=True)
        assert np.all(np.isfinite(got))
        with pytest.raises(EngineError, match="no resident"):
            eng.gauss_normal(np.full(2, 1e-6))              # three sets wanted, one is resident
    finally:
        eng.gauss_fit_end()


def _check_fit(name, fitted, fit_errs, chi2, dof, g, full_golden=None, full_errs=None):
    want = g["fitted_params"] if full_golden is None else full_golden
    sig = g["fit_errs"] if full_errs is None else full_errs
    v = sig > 0
    dist = np.abs(fitted - want)[v] / sig[v]
    scatter = float(np.max(g["self_scatter"]))
    rel = np.abs(fit_errs[v] / sig[v] - 1.0)
    MEASURED[name] = dict(max_distance_sigma=float(dist.max()), self_scatter_sigma=scatter, bar_sigma=10 * scatter,
                          chi2_rel=float(chi2 / float(g["chi2"]) - 1.0), fit_errs_rel=float(rel.max()))
    print(name, "max distance %.2e sigma (self-scatter %.2e), chi2 rel %.1e, errs rel %.1e" %
          (dist.max(), scatter, chi2 / float(g["chi2"]) - 1.0, rel.max()))
    assert np.all(fitted[~v] == want[~v])
    assert np.all(fit_errs[~v] == 0.0)
    assert dist.max() <= 1e-3
    assert dist.max() <= 10 * scatter
    assert chi2 <= float(g["chi2"]) * (1 + 1e-9)
    assert rel.max() <= 1e-4
    assert dof == int(g["dof"])


@pytest.mark.parametrize("name", ["16x256", "12x200"])
def test_golden_fits_through_the_engine(eng, name):
    from pulseportraiture_amd.pplib import fit_gaussian_portrait, get_bin_centers
    g = _g("ppgauss_fit_" + name)
    nchan, nbin = g["data"].shape
    with eng.profiled() as kt:
        r = fit_gaussian_portrait(str(g["code"]), g["data"], g["init_params"], float(g["scattering_index_in"]),
                                  np.outer(g["errs"], np.ones(nbin)), g["fit_flags"], False, get_bin_centers(nbin),
                                  g["freqs"], float(g["nu_ref"]), engine=eng)
    # one iteration is one gauss_residuals plus one gauss_normal, plus one of each per trial step
    lm = r.lm_results
    assert kt["gauss_resid"][1] == lm.niter + lm.nfev + 1 and kt["gauss_normal"][1] == lm.niter + lm.nfev
    assert r.scattering_index == float(g["scattering_index"]) and r.scattering_index_err == 0.0
    _check_fit("fit_" + name, r.fitted_params, r.fit_errs, r.chi2, r.dof, g)
    MEASURED["fit_" + name].update(jacobians=int(lm.niter), trial_steps=int(lm.nfev), message=lm.message)


def test_fit_gaussian_profile_against_the_reference(eng):
    from pulseportraiture_amd.pplib import fit_gaussian_profile
    g = _g("ppgauss_profile")
    n = len(g["profile"])
    r = fit_gaussian_profile(g["profile"], g["init_params"], np.zeros(n) + float(g["noise"]), engine=eng)
    _check_fit("fit_profile", r.fitted_params, r.fit_errs, r.chi2, r.dof, g)
    # residuals = data - model at the fitted parameters (pplib.py:1906-1908), the model to the device-vs-host bar
    from pulseportraiture_amd import gmodel
    p = r.fitted_params
    mdl = dict(params=np.array([p[0], p[1], p[2], 0.0, p[3], 0.0, p[4], 0.0]), code="111", nu_ref=1.0, alpha=0.0, ngauss=1)
    model = gmodel.gaussian_portrait(mdl, np.array([1.0]), n, P=float(n))[0]
    np.testing.assert_allclose(r.residuals, g["profile"] - model, rtol=0,
                               atol=2e-14 * np.abs(model).max() + np.spacing(np.abs(g["profile"]).max()))
    assert np.sum((r.residuals / float(g["noise"])) ** 2) == pytest.approx(r.chi2, rel=1e-12)


def _portrait(port, freqs, P, sigma, name="fake.npz"):
    from pulseportraiture_amd.ppgauss import DataPortrait
    from pulseportraiture_amd.pptoas import data_from_arrays
    nchan = len(freqs)
    data = data_from_arrays(port[None, None], freqs, [P], [55000.0], noise_stds=np.full((1, 1, nchan), sigma), bw=800.0,
                            source="PSR_1234-5678", filename=name)
    return DataPortrait(data, quiet=True)


def test_make_gaussian_model_rotates_and_refits_to_convergence(eng, tmp_path):
    """The 16 x 256 case rotated by a known phase and DM, from the case's start (through a model file): every pass's
    check_convergence against the reference's, within the legacy fit_portrait golden test's bars; the loop ends
    converged on the pass the reference's does."""
    from pulseportraiture_amd import gmodel
    g, c = _g("ppgauss_fit_16x256"), _g("ppgauss_convergence")
    start = tmp_path / "start.gmodel"
    gmodel.write_gmodel(str(start), "start", str(g["code"]), float(g["nu_ref"]), g["init_params"], g["fit_flags"],
                        float(g["scattering_index_in"]), 0, quiet=True)
    dp = _portrait(c["data"], g["freqs"], float(c["P"]), 0.05)
    dp.engine = eng
    dp.make_gaussian_model(modelfile=str(start), niter=2, writemodel=True, outfile=str(tmp_path / "out.gmodel"),
                           writeerrfile=True, quiet=True)
    assert abs(dp.nu_fit - float(c["nu_fit"])) < 1e-9
    want = c["passes"]
    got = np.array(dp.convergence_history, dtype=np.float64)
    print("passes\n", got, "\nreference\n", want)
    assert got.shape == want.shape
    for a, b in zip(got, want):
        assert abs((a[0] - b[0] + 0.5) % 1.0 - 0.5) < PHI_BAR and abs(a[2] - b[2]) < DM_BAR
        np.testing.assert_allclose([a[1], a[3], a[4]], [b[1], b[3], b[4]], rtol=1e-6)
        assert a[5] == b[5]
    assert dp.cnvrgnc == 1 and got[0, 5] == 0
    MEASURED["convergence"] = dict(dphi=float(np.abs(got[:, 0] - want[:, 0]).max()), dDM=float(np.abs(got[:, 2] - want[:, 2]).max()))
    # the first pass's parameters are not stored by the loop, the last pass's files are
    mdl = gmodel.read_gmodel(str(tmp_path / "out.gmodel"))
    assert mdl["ngauss"] == 3 and os.path.exists(str(tmp_path / "out.gmodel_errs"))
    np.testing.assert_allclose(mdl["params"], dp.model_params, rtol=0, atol=6e-9)


def test_command_line_round_trip_to_toas(tmp_path):
    """archive -> ppgauss_run --gauss ... -> .gmodel -> GetTOAs: the pipeline README describes."""
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.pptoas import GetTOAs
    g = _g("ppgauss_fit_16x256")
    nchan = len(g["freqs"])
    P = gmodel.EXAMPLE_PERIOD
    np.savez(tmp_path / "case.npz", subints=g["data"][None, None], freqs=g["freqs"][None], Ps=np.array([P]),
             epochs=np.array([55000.0]), noise_stds=np.full((1, 1, nchan), 0.05), bw=800.0, source="PSR_1234-5678")
    out = run_module("ppgauss_run", ["-d", "case.npz", "--gauss", "0.22,0.05,4.0", "--gauss", "0.234,0.016,7.0", "--gauss",
                                     "0.258,0.024,2.4", "-o", "out.gmodel", "-m", "made_here"], tmp_path, 300)
    assert "Fitting Gaussian model portrait..." in out
    mdl = gmodel.read_gmodel(str(tmp_path / "out.gmodel"))
    assert mdl["name"] == "made_here" and mdl["ngauss"] == 3 and mdl["code"] == "000"
    assert list(mdl["fit_flags"][3::6]) == [0, 0, 0] and list(mdl["fit_flags"][5::6]) == [1, 1, 1]     # fixloc is the default
    assert os.path.exists(str(tmp_path / "out.gmodel_errs"))
    port = gmodel.gaussian_portrait(mdl, g["freqs"], g["data"].shape[1], P)
    assert np.std(g["data"] - port) < 1.2 * 0.05
    gt = GetTOAs([str(tmp_path / "case.npz")], str(tmp_path / "out.gmodel"), quiet=True)
    gt.get_TOAs(quiet=True)
    assert len(gt.TOA_list) == 1 and np.all(np.isfinite(gt.phis[0]))
    assert abs(gt.phis[0][0]) < 1e-3        # the model was made from this very portrait
