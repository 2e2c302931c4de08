#!/usr/bin/env python3
"""ppgauss goldens from the TRUE reference: its pplib.py and ppgauss.py, converted to Python 3 in a
scratch directory (make_golden.import_reference), with one thing replaced.  The reference fits with
lmfit, which is not available; this script carries its own small stand-in for the part of lmfit the
reference uses (StandInLmfit below -- this project's code, not the reference's): Parameters.add(name,
value, vary, min, max), and minimize(fn, params, kws) built on scipy.optimize.leastsq (MINPACK lmdif at
SciPy's default tolerances) with lmfit's MINUIT bound transforms, scale_covar = True (covariance x chi^2 / nfree),
stderr = 0 for fixed parameters, and .params, .nfree, .chisqr, .redchi, .residual, .message.

The objective is the reference's own: fit_gaussian_portrait_function, fit_gaussian_profile_function,
gen_gaussian_portrait, gen_gaussian_profile, write_model and ppgauss.check_convergence all run unchanged.
Its minimum does not depend on the optimiser: every fit is solved a second time, the same reference
residual function through scipy.optimize.least_squares(method='trf', x_scale='jac') at tight tolerances,
and the difference between the two solves in units of the 1-sigma errors -- the reference's self-scatter
-- is stored beside the answer.

    ppgauss_rows.npz          fit_gaussian_portrait_function at 3 x 64 and 3 x 100, codes 000 and 011, the
                              five-component edge model with and without tau: a base vector and eight
                              vectors with one parameter stepped
    ppgauss_fit_16x256.npz    example pulsar, sigma 0.05, tau fixed at 0, fixloc: inputs, both solves, scatter
    ppgauss_fit_12x200.npz    ... tau fitted, all evolution free
    ppgauss_profile.npz       fit_gaussian_profile of the 16 x 256 case's band-averaged profile from
                              GaussianSelector's auto_gauss = 0.05 start
    ppgauss_convergence.npz   the 16 x 256 case rotated by a known phase and DM: the first fit, its
                              check_convergence, and the rotate-and-refit loop's later passes
    ppgauss_fit.gmodel(_errs) DataPortrait.write_model / write_errfile of the 12 x 200 fit

The script asserts what keeps the parity tests from being decided by the optimiser: both solves end with
chi^2/dof within 0.9 ... 1.1, no bounded parameter within 5 sigma of a bound, self-scatter < 1e-4 sigma, and
the two solves' errors within 1e-5 of each other.

Build-container only (needs the reference sources)."""
import collections
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import scipy.optimize as opt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

P_EXAMPLE = 1.0 / 345.67890123456789
SIGMA = 0.05


# ---- the stand-in for lmfit -------------------------------------------------------
class Parameter(object):
    def __init__(self, name, value, vary, lo, hi):
        self.name, self.value, self.vary, self.stderr = name, float(value), bool(vary), 0.0
        self.min = -np.inf if lo is None else float(lo)
        self.max = np.inf if hi is None else float(hi)

    def to_internal(self):
        if np.isinf(self.min) and np.isinf(self.max):
            return self.value
        if np.isinf(self.max):
            return np.sqrt((self.value - self.min + 1.0) ** 2 - 1.0)
        if np.isinf(self.min):
            return np.sqrt((self.max - self.value + 1.0) ** 2 - 1.0)
        return np.arcsin(2.0 * (self.value - self.min) / (self.max - self.min) - 1.0)

    def from_internal(self, p):
        if np.isinf(self.min) and np.isinf(self.max):
            return p
        if np.isinf(self.max):
            return self.min - 1.0 + np.sqrt(p * p + 1.0)
        if np.isinf(self.min):
            return self.max + 1.0 - np.sqrt(p * p + 1.0)
        return self.min + (np.sin(p) + 1.0) * (self.max - self.min) / 2.0

    def scale_gradient(self, p):
        if np.isinf(self.min) and np.isinf(self.max):
            return 1.0
        if np.isinf(self.max):
            return p / np.sqrt(p * p + 1.0)
        if np.isinf(self.min):
            return -p / np.sqrt(p * p + 1.0)
        return np.cos(p) * (self.max - self.min) / 2.0


class Parameters(collections.OrderedDict):
    def add(self, name, value=None, vary=True, min=None, max=None, expr=None):
        assert expr is None
        self[name] = Parameter(name, value, vary, min, max)


class MinimizerResult(object):
    pass


def _residual_of(fn, params, kws):
    names = [k for k, q in params.items() if q.vary]

    def resid(p):
        for k, v in zip(names, p):
            params[k].value = float(params[k].from_internal(v))
        return np.asarray(fn(params, **kws), dtype=np.float64)
    return names, resid


def _finish(params, names, resid, p, cov_internal, message):
    r = resid(p)
    out = MinimizerResult()
    out.params, out.residual, out.message = params, r, message
    out.chisqr = float((r * r).sum())
    out.nfree = len(r) - len(names)
    out.redchi = out.chisqr / out.nfree
    for q in params.values():
        q.stderr = 0.0
    if cov_internal is not None:
        grad = np.array([params[k].scale_gradient(v) for k, v in zip(names, p)])
        cov = cov_internal * np.outer(grad, grad) * out.redchi
        for i, k in enumerate(names):
            params[k].stderr = float(np.sqrt(cov[i, i]))
    return out


def minimize(fn, params, kws=None, **unused):
    """lmfit.minimize(method='leastsq') on scipy.optimize.leastsq's default tolerances (ftol = xtol =
    1.49e-8).  lmfit's own (1e-7) stop MINPACK one iteration earlier with 20 free parameters, 1e-4 ... 6e-4
    sigma from where the tight second solve ends (measured on six seeds of the 12 x 200 case): that is how
    far the reference's answers scatter in use, but as a pin of the minimum it would be the looser one."""
    names, resid = _residual_of(fn, params, kws or {})
    p0 = np.array([params[k].to_internal() for k in names])
    p, cov, info, mesg, ier = opt.leastsq(resid, p0, full_output=1, maxfev=2000 * (len(p0) + 1))
    return _finish(params, names, resid, p, cov, mesg)


def minimize_trf(fn, params, kws=None):
    """The second solve: the same residual function and transforms, another optimiser."""
    names, resid = _residual_of(fn, params, kws or {})
    p0 = np.array([params[k].to_internal() for k in names])
    sol = opt.least_squares(resid, p0, method='trf', x_scale='jac', ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=4000)
    J = sol.jac
    return _finish(params, names, resid, sol.x, np.linalg.inv(J.T @ J), sol.message)


def install_standin(refmod):
    lm = types.ModuleType("lmfit")
    lm.Parameters, lm.minimize = Parameters, minimize
    sys.modules["lmfit"] = lm
    refmod.lm = lm
    return lm


def import_ppgauss():
    ref, tmp = mg.import_reference()
    shutil.copy(os.path.join(mg.REF, "ppgauss.py"), tmp)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", "ppgauss.py"], cwd=tmp,
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    import pplib
    lm = install_standin(pplib)
    import ppgauss
    return pplib, ppgauss, lm, tmp


# ---- residual rows ----------------------------------------------------------------
EDGE = dict(dc=0.01, comps=[[0.02, -1e-5, 0.03, 2e-6, 3.0, -5e-4], [0.97, 2e-5, 0.012, -1e-6, 1.5, 1e-3],
                            [0.50, 0.0, 0.2, 1e-5, 0.4, 0.0], [1.30, 0.0, 0.05, 0.0, 1.0, 0.0],
                            [0.70, 0.0, -0.01, 0.0, 1.0, 0.0]], alpha=-3.7, nu_ref=1500.0)
# the stepped entries of [DC, tau, comps ..., scattering index]: DC, tau, a loc, a loc slope, a wid, an amp,
# an amp index, the scattering index -- and the size of each step
STEPS = [(0, 1e-3), (1, 0.3), (2 + 6, 1e-3), (2 + 3, 1e-6), (2 + 2 * 6 + 2, 1e-3), (2 + 4, 1e-2), (2 + 6 + 5, 1e-5),
         (-1, 0.05)]


def params_of(ref, vec):
    prm = ref.lm.Parameters()
    for i, v in enumerate(vec):
        prm.add("p%03d" % i, v, vary=False)
    return prm


def rows_golden(ref):
    store = {}
    rng = np.random.default_rng(mg.SEED + 700)
    for nbin in (64, 100):
        freqs = np.array([1180.0, 1500.0, 1820.0])
        errs1 = np.array([0.05, 0.07, 0.11])
        phases = ref.get_bin_centers(nbin)
        data = rng.standard_normal((3, nbin)) * errs1[:, None] + 0.3 * np.sin(2 * np.pi * phases)[None]
        errs = np.outer(errs1, np.ones(nbin))
        for code in ("000", "011"):
            for tau_bins in (0.0, 0.9):
                base = np.array([EDGE["dc"], tau_bins] + list(np.ravel(EDGE["comps"])) + [EDGE["alpha"]])
                sets = [base]
                for idx, step in STEPS:
                    v = base.copy()
                    v[idx] += step
                    sets.append(v)
                sets = np.array(sets)
                with np.errstate(invalid="ignore"):
                    rows = np.array([ref.fit_gaussian_portrait_function(
                        params_of(ref, v), code, phases, freqs, EDGE["nu_ref"], data=data, errs=errs, join_ichans=[],
                        P=None) for v in sets])
                assert np.all(np.isfinite(rows)), (nbin, code, tau_bins)
                tag = "n%d_c%s_t%d" % (nbin, code, int(tau_bins != 0.0))
                store[tag + "_sets"], store[tag + "_rows"] = sets, rows
        store["n%d_data" % nbin], store["n%d_errs" % nbin], store["n%d_freqs" % nbin] = data, errs1, freqs
    store["nu_ref"] = EDGE["nu_ref"]
    mg.save("ppgauss_rows", **store)


# ---- fits -------------------------------------------------------------------------
def example_truth(ref):
    (name, code, nu_ref, ngauss, params, flags, alpha, fit_alpha) = ref.read_model(
        os.path.join(mg.REF, "examples", "example.gmodel"), quiet=True)
    return code, float(nu_ref), np.array(params, dtype=np.float64), float(alpha)


def band(nchan, nu0=1500.0, bw=800.0):
    d = bw / nchan
    return np.linspace(nu0 - bw / 2 + d / 2, nu0 + bw / 2 - d / 2, nchan)


def fit_case(ref, nchan, nbin, tau_us, fixloc, seed):
    code, nu_ref, truth, alpha = example_truth(ref)
    truth = truth.copy()
    truth[1] = 0.0 if not tau_us else tau_us * 1e-6 / P_EXAMPLE * nbin       # [bin]
    freqs, phases = band(nchan), ref.get_bin_centers(nbin)
    rng = np.random.default_rng(seed)
    clean = ref.gen_gaussian_portrait(code, truth, alpha, phases, freqs, nu_ref)
    data = clean + SIGMA * rng.standard_normal(clean.shape)
    flags = np.ones(len(truth))
    flags[1] = 1.0 if tau_us else 0.0
    if fixloc:
        flags[3::6] = 0
    init = np.where(flags != 0, truth * (1.0 + 0.003 * rng.standard_normal(len(truth))), truth)
    errs = np.full(clean.shape, SIGMA)
    return dict(code=code, nu_ref=nu_ref, truth=truth, alpha=alpha, freqs=freqs, phases=phases, data=data, flags=flags,
                init=init, errs=errs)


def solve_both(ref, c, data=None):
    """fit_gaussian_portrait through the stand-in, then the same objective by trf.  Returns (stand-in
    result, trf vector, trf errors, trf chi2, self-scatter in sigma)."""
    data = c["data"] if data is None else data
    args = (c["code"], data, c["init"], c["alpha"], c["errs"], c["flags"], False, c["phases"], c["freqs"], c["nu_ref"])
    a = ref.fit_gaussian_portrait(*args, join_params=[], P=None, quiet=True)
    true_min = ref.lm.minimize
    box = {}

    def trf(fn, params, kws=None):
        box["r"] = minimize_trf(fn, params, kws)
        return box["r"]
    ref.lm.minimize = trf
    try:
        b = ref.fit_gaussian_portrait(*args, join_params=[], P=None, quiet=True)
    finally:
        ref.lm.minimize = true_min
    for r in (a, b):
        assert 0.9 < r.chi2 / r.dof < 1.1, r.chi2 / r.dof
    full_a = np.append(a.fitted_params, a.scattering_index)
    full_b = np.append(b.fitted_params, b.scattering_index)
    errs_a = np.append(a.fit_errs, a.scattering_index_err)
    varied = errs_a > 0
    scatter = np.zeros(len(full_a))
    scatter[varied] = np.abs(full_a - full_b)[varied] / errs_a[varied]
    assert scatter.max() < 1e-4, scatter
    # the two solves' errors agree to a tenth of the bar the tests hold fit_errs to (1e-4).  They do not on every
    # input: lmdif steps a parameter by sqrt(eps) |x|, and a slope the fit happens to put near zero (seed 703:
    # m_loc3 = -4e-5 +- 2e-3, step 6e-13) moves its component by less than the rounding of the evolved location;
    # that column of MINPACK's Jacobian, and with it the error, is then noise at the 1e-3 level
    errs_b = np.append(b.fit_errs, b.scattering_index_err)
    assert np.abs(errs_b[varied] / errs_a[varied] - 1.0).max() < 1e-5, errs_b[varied] / errs_a[varied] - 1.0
    # bounded parameters: tau >= 0, 0 <= wid <= wid_max, amp >= 0
    n = len(a.fitted_params)
    for idx, lo, hi in [([1], 0.0, np.inf), (range(4, n, 6), 0.0, ref.wid_max), (range(6, n, 6), 0.0, np.inf)]:
        for i in idx:
            if errs_a[i] > 0:
                assert full_a[i] - lo > 5 * errs_a[i] and hi - full_a[i] > 5 * errs_a[i], (i, full_a[i], errs_a[i])
    return a, b, scatter


def fit_golden(ref, name, c):
    a, b, scatter = solve_both(ref, c)
    mg.save("ppgauss_fit_" + name, code=np.array(c["code"]), nu_ref=c["nu_ref"], truth=c["truth"], freqs=c["freqs"],
            data=c["data"], errs=c["errs"][:, 0], fit_flags=c["flags"], init_params=c["init"], scattering_index_in=c["alpha"],
            fitted_params=a.fitted_params, fit_errs=a.fit_errs, chi2=a.chi2, dof=a.dof, scattering_index=a.scattering_index,
            scattering_index_err=a.scattering_index_err, trf_fitted_params=b.fitted_params, trf_fit_errs=b.fit_errs,
            trf_chi2=b.chi2, self_scatter=scatter)
    print("   ", name, "chi2/dof %.4f" % (a.chi2 / a.dof), "self-scatter max %.1e sigma" % scatter.max(),
          "| d chi2 %.1e" % (a.chi2 - b.chi2))
    return a


def profile_golden(ref, c):
    """GaussianSelector's auto_gauss branch (ppgauss.py:442-459) by hand, on the band-averaged profile."""
    profile = c["data"].mean(axis=0)
    errs = ref.get_noise(profile)
    auto_gauss = 0.05
    nbin = len(profile)
    init = [sorted(profile)[nbin // 10 + 1], 0.0]
    amp = profile.max()
    first_gauss = amp * ref.gaussian_profile(nbin, 0.5, auto_gauss)
    loc = 0.5 + ref.fit_phase_shift(profile, first_gauss, errs).phase
    init += [loc, auto_gauss, amp]
    errs_arr = np.zeros(nbin) + errs
    a = ref.fit_gaussian_profile(profile, init, errs_arr, None, False, quiet=True)
    true_min = ref.lm.minimize
    ref.lm.minimize = lambda fn, params, kws=None: minimize_trf(fn, params, kws)
    try:
        b = ref.fit_gaussian_profile(profile, init, errs_arr, None, False, quiet=True)
    finally:
        ref.lm.minimize = true_min
    varied = a.fit_errs > 0
    scatter = np.zeros(len(init))
    scatter[varied] = np.abs(a.fitted_params - b.fitted_params)[varied] / a.fit_errs[varied]
    # (one Gaussian on a three-component profile: chi^2/dof >> 1, a large-residual problem on which MINPACK
    # converges linearly and stops at its ftol further out than in the portrait fits -- measured 4e-4 sigma;
    # the conditions on the portrait fits' inputs do not apply, the scatter is recorded as it is)
    assert scatter.max() < 1e-3, scatter
    mg.save("ppgauss_profile", profile=profile, noise=errs, auto_gauss=auto_gauss, init_params=np.array(init),
            fitted_params=a.fitted_params, fit_errs=a.fit_errs, residuals=a.residuals, chi2=a.chi2, dof=a.dof,
            trf_fitted_params=b.fitted_params, self_scatter=scatter)
    print("    profile chi2/dof %.3f" % (a.chi2 / a.dof), "self-scatter max %.1e" % scatter.max())


PHI_INJ, DM_INJ = 0.002, 2e-4


def convergence_golden(ref, refgauss, c):
    """The rotate-and-refit loop of make_gaussian_model (ppgauss.py:168-205) on the 16 x 256 case with the
    data rotated by a known phase and DM, pass by pass: fit_gaussian_portrait, gen_gaussian_portrait,
    check_convergence (the reference's own, on an object that carries the fields it reads)."""
    nu_fit = ref.guess_fit_freq(c["freqs"], None)
    port = ref.rotate_data(c["data"], -PHI_INJ, -DM_INJ, P_EXAMPLE, c["freqs"], nu_fit)
    o = types.SimpleNamespace(njoin=0, Ps=[P_EXAMPLE], freqsxs=[c["freqs"]], nu_fit=nu_fit, niter=2, itern=2, duration=0.0,
                              portx=port.copy())
    params = c["init"].copy()
    passes = []
    for it in range(3):
        r = ref.fit_gaussian_portrait(c["code"], o.portx, params, c["alpha"], c["errs"], c["flags"], False, c["phases"],
                                      c["freqs"], c["nu_ref"], join_params=[], P=None, quiet=True)
        params = r.fitted_params.copy()
        o.modelx = ref.gen_gaussian_portrait(c["code"], r.fitted_params, r.scattering_index, c["phases"], c["freqs"],
                                             c["nu_ref"])
        cnv = refgauss.DataPortrait.check_convergence(o, efac=1.0, quiet=True)
        passes.append([o.phi, o.phierr, o.DM, o.DMerr, o.red_chi2, 1.0 if cnv else 0.0])
        if it == 0:
            first = r
        if cnv or it == 2:
            break
        o.niter -= 1
        o.portx = ref.rotate_data(o.portx, o.phi, o.DM, P_EXAMPLE, c["freqs"], nu_fit)
    passes = np.array(passes)
    assert passes[-1, 5] == 1.0, passes          # the loop ends converged within niter = 2
    assert passes[0, 5] == 0.0, passes           # ... and not at once
    mg.save("ppgauss_convergence", data=port, phi_inj=PHI_INJ, DM_inj=DM_INJ, nu_fit=nu_fit, P=P_EXAMPLE,
            first_fitted_params=first.fitted_params, first_fit_errs=first.fit_errs, first_chi2=first.chi2,
            passes=passes)
    print("    convergence passes (phi, phierr, DM, DMerr, red_chi2, converged):\n", passes)


def model_text_golden(ref, refgauss, c, a):
    """DataPortrait.write_model / write_errfile (ppgauss.py:336-372) of the 12 x 200 fit, one loc moved
    past 1 so that the tidy-up shows."""
    nbin = len(c["phases"])
    params = a.fitted_params.copy()
    params[2 + 6] += 1.0
    o = types.SimpleNamespace(model_params=params, model_param_errs=a.fit_errs.copy(), Ps=[P_EXAMPLE], nbin=nbin,
                              model_name="PSR_1234-5678", model_code=c["code"], nu_ref=c["nu_ref"], fit_flags=c["flags"],
                              scattering_index=a.scattering_index, scattering_index_err=a.scattering_index_err, fitalpha=0,
                              datafile="fake.npz")
    out = os.path.join(HERE, "ppgauss_fit.gmodel")
    refgauss.DataPortrait.write_model(o, outfile=out, quiet=True)
    refgauss.DataPortrait.write_errfile(o, errfile=out + "_errs", quiet=True)
    mg.save("ppgauss_model_text", model_params=params, model_param_errs=a.fit_errs, fit_flags=c["flags"], P=P_EXAMPLE, nbin=nbin,
            nu_ref=c["nu_ref"], scattering_index=a.scattering_index, scattering_index_err=a.scattering_index_err)


def main():
    ref, refgauss, lm, tmp = import_ppgauss()
    rows_golden(ref)
    ca = fit_case(ref, 16, 256, None, True, mg.SEED + 701)
    fit_golden(ref, "16x256", ca)
    cb = fit_case(ref, 12, 200, 30.0, False, mg.SEED + 734)      # (the first seed from 702 on that meets every condition)
    ab = fit_golden(ref, "12x200", cb)
    profile_golden(ref, ca)
    convergence_golden(ref, refgauss, ca)
    model_text_golden(ref, refgauss, cb, ab)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
