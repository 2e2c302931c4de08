"""Levenberg-Marquardt fits of Gaussian-component models (ppgauss).

The reference fits with lmfit (fit_gaussian_portrait / fit_gaussian_profile,
pplib.py:1842-2052): MINPACK's lmdif on a forward-difference Jacobian, with bounded
parameters mapped to unbounded internal ones by MINUIT's transforms.  This module is
the same fit with its own driver: Levenberg-Marquardt on the normal equations with
Marquardt's diagonal scaling, the same transforms, the same forward-difference steps
(sqrt(eps) |p|, or sqrt(eps) at 0, on the internal parameters), and lmfit's errors
(scale_covar: the covariance times chi^2 / dof, carried back to the external
parameters; 0 for fixed ones).  The minimum of the objective does not depend on the
optimiser, so the fitted parameters are the reference's.

The driver does not know how residuals are formed.  It takes an evaluator

    evaluate(sets[nsets, nparam], h[nsets - 1]) -> (chi2, g, G)

which for the external parameter vectors `sets` (the base point first, then one
vector per stepped parameter) returns chi2 = sum R_0^2, g_a = sum D_a R_0 and G_ab =
sum D_a D_b with D_a = (R_{a+1} - R_0) / h_a.  engine_evaluator runs it on the device
(Engine.gauss_residuals + Engine.gauss_normal: one launch each per iteration, the
data portrait resident); numpy_evaluator is the host restatement for tests.

A parameter vector is the reference's: [DC, tau [bin], (loc, m_loc, wid, m_wid, amp,
m_amp) x ngauss, scattering_index].  A joined fit -- one model for njoin bands, each with a
phase offset and a Delta-DM of its own (pplib.py:1992-2017) -- carries them in front of the
scattering index, as the reference does: [..., phase1, DM1, ..., phase_njoin, DM_njoin,
scattering_index].
"""
import numpy as np

from . import gmodel
from .pplib import DataBunch, wid_max

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


# ---- MINUIT's bound transforms (lmfit Parameter.setup_bounds / scale_gradient) ----
def to_internal(x, lo, hi):
    """Internal value p of external x: x itself without bounds; with a lower bound only
    x = lo - 1 + sqrt(p^2 + 1); with both x = lo + (sin p + 1)(hi - lo) / 2."""
    if np.isinf(lo) and np.isinf(hi):
        return float(x)
    if np.isinf(hi):
        return float(np.sqrt((x - lo + 1.0) ** 2 - 1.0))
    if np.isinf(lo):
        return float(np.sqrt((hi - x + 1.0) ** 2 - 1.0))
    return float(np.arcsin(2.0 * (x - lo) / (hi - lo) - 1.0))


def to_external(p, lo, hi):
    if np.isinf(lo) and np.isinf(hi):
        return float(p)
    if np.isinf(hi):
        return float(lo - 1.0 + np.sqrt(p * p + 1.0))
    if np.isinf(lo):
        return float(hi + 1.0 - np.sqrt(p * p + 1.0))
    return float(lo + (np.sin(p) + 1.0) * (hi - lo) / 2.0)


def d_external(p, lo, hi):
    """dx / dp at internal value p."""
    if np.isinf(lo) and np.isinf(hi):
        return 1.0
    if np.isinf(hi):
        return float(p / np.sqrt(p * p + 1.0))
    if np.isinf(lo):
        return float(-p / np.sqrt(p * p + 1.0))
    return float(np.cos(p) * (hi - lo) / 2.0)


def external_covariance(cov_internal, p, lo, hi):
    """The covariance of the external parameters from that of the internal ones p."""
    grad = np.array([d_external(pi, l, h) for pi, l, h in zip(p, lo, hi)])
    return cov_internal * np.outer(grad, grad)


def portrait_bounds(nparam, njoin=0):
    """(lo, hi) of a portrait parameter vector (pplib.py:1964-2020): tau >= 0,
    0 <= wid <= wid_max, amp >= 0, everything else -- the 2 njoin join parameters too -- free."""
    lo, hi = np.full(nparam, -np.inf), np.full(nparam, np.inf)
    nmodel = nparam - 1 - 2 * njoin
    lo[1] = 0.0
    lo[4:nmodel:6], hi[4:nmodel:6] = 0.0, wid_max
    lo[6:nmodel:6] = 0.0
    return lo, hi


# ---- the driver -------------------------------------------------------------
def levenberg_marquardt(evaluate, x0, vary, lo, hi, nsample, max_iter=100, xtol=1e-6, lam0=1e-3):
    """Minimise chi2(x) over the parameters x[vary] within (lo, hi).  Returns a DataBunch:
    x (external, all parameters), stderr (0 for fixed ones), chi2, dof, niter (Jacobians
    taken), nfev (residual evaluations of single points), message.

    One iteration is one evaluate() of the base point with every stepped parameter, plus
    one evaluate() of a single point per trial step.  It ends when the undamped (Gauss-Newton)
    step from the new point would move no parameter by more than xtol of its 1-sigma error, or
    when no damping up to 1e12 finds a lower chi2 (the fit sits at the rounding floor of its
    forward differences)."""
    x = np.array(x0, dtype=np.float64)
    iv = np.flatnonzero(np.asarray(vary).astype(bool))
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    for i in iv:
        if not lo[i] <= x[i] <= hi[i]:
            raise ValueError("parameter %d = %g starts outside its bounds (%g, %g)" % (i, x[i], lo[i], hi[i]))
    p = np.array([to_internal(x[i], lo[i], hi[i]) for i in iv])
    nvar = len(iv)
    dof = int(nsample) - nvar

    def external(pv):
        out = x.copy()
        for k, i in enumerate(iv):
            out[i] = to_external(pv[k], lo[i], hi[i])
        return out

    def jacobian(pv):
        h = SQRT_EPS * np.maximum(1.0, np.abs(pv))
        sets = np.empty((nvar + 1, len(x)))
        sets[0] = external(pv)
        for k in range(nvar):
            q = pv.copy()
            q[k] += h[k]
            h[k] = q[k] - pv[k]          # the step as taken
            sets[k + 1] = external(q)
        return evaluate(sets, h)

    lam, niter, nfev, message = lam0, 0, 0, "iteration limit"
    chi2, g, G = jacobian(p)
    niter += 1
    while niter < max_iter and nvar:
        d = np.diag(G).copy()
        d[d <= 0.0] = 1.0
        accepted = False
        while lam <= 1e12:
            try:
                delta = np.linalg.solve(G + lam * np.diag(d), -g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            trial = p + delta
            c2 = evaluate(external(trial)[None], np.zeros(0))[0]
            nfev += 1
            if np.isfinite(c2) and c2 < chi2:
                accepted = True
                break
            lam *= 10.0
        if not accepted:
            message = "no lower chi2 at any damping"
            break
        p, lam = trial, max(lam / 10.0, 1e-15)
        chi2, g, G = jacobian(p)
        niter += 1
        try:
            sig = np.sqrt(np.abs(np.diag(np.linalg.inv(G))))
            newton = np.linalg.solve(G, -g)
        except np.linalg.LinAlgError:
            continue
        if np.all(np.abs(newton) <= xtol * sig):
            message = "converged: undamped step below %g sigma" % xtol
            break
    stderr = np.zeros(len(x))
    if nvar:
        try:
            cov = external_covariance(np.linalg.inv(G) * (chi2 / dof), p, lo[iv], hi[iv])
            stderr[iv] = np.sqrt(np.abs(np.diag(cov)))
        except np.linalg.LinAlgError:
            stderr[iv] = np.nan
    return DataBunch(x=external(p), stderr=stderr, chi2=float(chi2), dof=dof, niter=niter, nfev=nfev,
                     message=message)


# ---- evaluators ---------------------------------------------------------------
def _model_of(vec, code, nu_ref, nbin, njoin=0):
    """The parsed-.gmodel dict of a portrait parameter vector, tau in bins (period = nbin)."""
    vec = np.asarray(vec, dtype=np.float64)
    nmodel = len(vec) - 1 - 2 * njoin
    return dict(params=vec[:nmodel], code=code, nu_ref=nu_ref, alpha=vec[-1], ngauss=(nmodel - 2) // 6)


def host_residuals(sets, data, errs, code, freqs, nu_ref, join_ichans=None, P=None):
    """(data - gen_gaussian_portrait(set)) / errs of every parameter vector, raveled
    (fit_gaussian_portrait_function, pplib.py:1230-1242) -> [nsets, nchan nbin].  join_ichans
    and the period P: the bands of a joined fit, their parameters in the vectors."""
    data = np.asarray(data, dtype=np.float64)
    nbin = data.shape[-1]
    sig = np.asarray(errs, dtype=np.float64)
    sig = sig[:, None] if sig.ndim == 1 else sig
    njoin = 0 if join_ichans is None else len(join_ichans)
    return np.array([((data - gmodel.gaussian_portrait(_model_of(v, code, nu_ref, nbin, njoin), freqs, nbin, P=float(nbin),
                                                       join_ichans=join_ichans if njoin else None,
                                                       join_params=v[len(v) - 1 - 2 * njoin:len(v) - 1], P_join=P))
                      / sig).ravel() for v in np.atleast_2d(sets)])


def normal_equations(R, h):
    """(chi2, g, G) of residual rows R[nsets, nrow] and steps h[nsets - 1]."""
    R = np.asarray(R, dtype=np.float64)
    D = (R[1:] - R[0]) / np.asarray(h, dtype=np.float64)[:, None]
    return float(R[0] @ R[0]), D @ R[0], D @ D.T


def numpy_evaluator(data, errs, code, freqs, nu_ref, join_ichans=None, P=None):
    """The evaluator on the host (gmodel.gaussian_portrait): what the device does, restated."""
    def evaluate(sets, h):
        return normal_equations(host_residuals(sets, data, errs, code, freqs, nu_ref, join_ichans, P), h)
    return evaluate


def _set_args(sets, nbin, njoin=0):
    """The arguments of Engine.gauss_residuals for parameter vectors: (dc, tau_rot, alpha, comps)
    and, for a joined fit, the keyword join [nsets,njoin,2]."""
    sets = np.atleast_2d(np.asarray(sets, dtype=np.float64))
    nmodel = sets.shape[1] - 1 - 2 * njoin
    args = (sets[:, 0], sets[:, 1] / float(nbin), sets[:, -1], sets[:, 2:nmodel].reshape(len(sets), (nmodel - 2) // 6, 6))
    return args, (dict(join=sets[:, nmodel:-1].reshape(len(sets), njoin, 2)) if njoin else {})


def engine_evaluator(eng, code, nu_ref, nbin, njoin=0):
    """The evaluator on the device, against the portrait Engine.gauss_fit_begin made resident (and
    the band map of Engine.gauss_fit_join, njoin bands): one gauss_residuals launch for all the
    sets, one gauss_normal."""
    def evaluate(sets, h):
        sets = np.atleast_2d(sets)
        if len(sets) > eng.GAUSS_FIT_MAX_SETS:
            raise ValueError("%d varied parameters: at most %d fit in one launch" %
                             (len(sets) - 1, eng.GAUSS_FIT_MAX_SETS - 1))
        args, kw = _set_args(sets, nbin, njoin)
        eng.gauss_residuals(code, nu_ref, *args, **kw)
        return eng.gauss_normal(h)
    return evaluate


def band_of_channels(join_ichans, nchan):
    """band_of_chan[nchan] of the reference's join_ichans (one index list per band): the band of
    every channel, -1 for a channel in none.  No channel may sit in two bands."""
    band = np.full(nchan, -1, dtype=np.intc)
    for ij, ichans in enumerate(join_ichans):
        ichans = np.asarray(ichans, dtype=int).reshape(-1)
        if len(ichans) and (ichans.min() < 0 or ichans.max() >= nchan):
            raise ValueError("join_ichans[%d] names a channel outside 0..%d" % (ij, nchan - 1))
        if np.any(band[ichans] >= 0) or len(np.unique(ichans)) != len(ichans):
            raise ValueError("join_ichans[%d] names a channel twice" % ij)
        band[ichans] = ij
    return band


# ---- the reference's two fits --------------------------------------------------
def _channel_errs(errs, nchan):
    """sigma_n [nchan] of the reference's errs (one value per channel, or a portrait of them
    that is constant along each row)."""
    e = np.asarray(errs, dtype=np.float64)
    if e.ndim == 0:
        return np.full(nchan, float(e))
    if e.ndim == 2:
        if np.any(e != e[:, :1]):
            raise ValueError("errs must be constant along every channel")
        e = e[:, 0]
    if e.shape != (nchan,):
        raise ValueError("errs must be [nchan] or [nchan,nbin]")
    return e


def fit_gaussian_portrait(model_code, data, init_params, scattering_index, errs, fit_flags,
                          fit_scattering_index, phases, freqs, nu_ref, join_params=[], P=None, quiet=True,
                          evaluator=None, engine=None):
    """fit_gaussian_portrait (pplib.py:1924-2052).  join_params = [join_ichans, values, flags]
    (one index list per band; phase1, DM1, phase2, ... and one flag for each) makes it a joined
    fit, which needs the period P [s]; fitted_params and fit_errs then end with the join
    parameters, as the reference's do.  evaluator: a stand-in for the device (numpy_evaluator,
    for a joined fit one built with join_ichans and P); engine: the Engine to run on (default
    the process-wide one)."""
    data = np.asarray(data)
    nchan, nbin = data.shape
    join_ichans, join_x0, join_vary = [], np.zeros(0), np.zeros(0, dtype=bool)
    if len(join_params):
        if P is None:
            raise NotImplementedError("fit_gaussian_portrait: a joined fit (join_params) cannot turn its DMs into "
                                      "rotations without the period: P is missing")
        join_ichans = [np.asarray(ic, dtype=int).reshape(-1) for ic in join_params[0]]
        join_x0 = np.asarray(join_params[1], dtype=np.float64).reshape(-1)
        join_vary = np.asarray(join_params[2]).reshape(-1) != 0
        if len(join_x0) != 2 * len(join_ichans) or len(join_vary) != len(join_x0):
            raise ValueError("join_params must hold a phase and a DM, and a flag for each, for every band")
        if not (np.isfinite(P) and P > 0.0):
            raise ValueError("P = %r is no period" % (P,))
        band = band_of_channels(join_ichans, nchan)
    njoin = len(join_ichans)
    if len(phases) != nbin:
        raise ValueError("phases must have one entry per bin")
    init_params = np.asarray(init_params, dtype=np.float64)
    if len(init_params) < 8 or (len(init_params) - 2) % 6 or len(fit_flags) != len(init_params):
        raise ValueError("init_params and fit_flags must hold 2 + 6 ngauss values")
    x0 = np.concatenate([init_params, join_x0, [float(scattering_index)]])
    vary = np.concatenate([np.asarray(fit_flags) != 0, join_vary, [bool(fit_scattering_index)]])
    lo, hi = portrait_bounds(len(x0), njoin)
    sig = _channel_errs(errs, nchan)
    freqs = np.asarray(freqs, dtype=np.float64)
    eng = None
    if evaluator is None:
        from .engine import default_engine
        eng = engine or default_engine()
        ng = (len(init_params) - 2) // 6
        if ng > eng.GAUSS_FIT_MAX_GAUSS:
            raise ValueError("%d components: at most %d are fitted" % (ng, eng.GAUSS_FIT_MAX_GAUSS))
        if njoin > eng.GAUSS_FIT_MAX_JOIN:
            raise ValueError("%d bands: at most %d are joined" % (njoin, eng.GAUSS_FIT_MAX_JOIN))
        if vary.sum() + 1 > eng.GAUSS_FIT_MAX_SETS:
            raise ValueError("%d varied parameters: at most %d fit in one launch" % (vary.sum(), eng.GAUSS_FIT_MAX_SETS - 1))
        eng.gauss_fit_begin(data, freqs, sig)
        evaluator = engine_evaluator(eng, str(model_code), float(nu_ref), nbin, njoin)
    try:
        if eng is not None and njoin:
            eng.gauss_fit_join(band, float(P), njoin)
        r = levenberg_marquardt(evaluator, x0, vary, lo, hi, nchan * nbin)
        residuals = None
        if eng is not None:
            args, kw = _set_args(r.x, nbin, njoin)
            residuals = eng.gauss_residuals(str(model_code), float(nu_ref), *args, fetch=True, **kw)[0]
    finally:
        if eng is not None:
            eng.gauss_fit_end()
    if residuals is None:
        residuals = host_residuals(r.x, data, sig, str(model_code), freqs, float(nu_ref), join_ichans if njoin else None,
                                   P)[0].reshape(nchan, nbin)
    residuals = residuals * sig[:, None]
    if not quiet:
        print("---------------------------------------------------------------")
        print("Gaussian Portrait Fit")
        print("---------------------------------------------------------------")
        print("fit status:", r.message)
        print("Gaussians:", (len(init_params) - 2) // 6)
        print("DoF:", r.dof)
        print("reduced chi-sq: %.2g" % (r.chi2 / r.dof))
        print("residuals mean: %.3g" % np.mean(residuals))
        print("residuals std.: %.3g" % np.std(residuals))
        print("---------------------------------------------------------------")
    return DataBunch(lm_results=r, fitted_params=r.x[:-1], fit_errs=r.stderr[:-1], scattering_index=r.x[-1],
                     scattering_index_err=r.stderr[-1], chi2=r.chi2, dof=r.dof, residuals=residuals)


def fit_gaussian_profile(data, init_params, errs, fit_flags=None, fit_scattering=False, quiet=True,
                         evaluator_factory=None, engine=None):
    """fit_gaussian_profile (pplib.py:1842-1922): the portrait fit of one channel at the
    reference frequency with every evolution parameter fixed at 0 (linear evolution, so that
    any loc, wid and amp pass through unchanged).  evaluator_factory(data[1,nbin], errs[1],
    code, freqs, nu_ref) -> evaluator stands in for the device."""
    data = np.asarray(data, dtype=np.float64)
    nbin = len(data)
    init_params = np.asarray(init_params, dtype=np.float64)
    nparam = len(init_params)
    if nparam < 5 or (nparam - 2) % 3:
        raise ValueError("init_params must hold 2 + 3 ngauss values")
    ng = (nparam - 2) // 3
    if fit_flags is None:
        flags = [True] * nparam
        flags[1] = bool(fit_scattering)
    else:
        flags = [bool(fit_flags[0]), bool(fit_scattering)] + [bool(fit_flags[i]) for i in range(1, nparam - 1)]
    e = np.asarray(errs, dtype=np.float64)
    if e.ndim and np.any(e != e.flat[0]):
        raise ValueError("errs must be one noise level for the whole profile")
    sig = np.array([float(e.flat[0]) if e.ndim else float(e)])
    x0, vary = np.zeros(3 + 6 * ng), np.zeros(3 + 6 * ng, dtype=bool)
    x0[:2], vary[:2] = init_params[:2], flags[:2]
    x0[2:-1:2], vary[2:-1:2] = init_params[2:], flags[2:]
    nu_ref = 1.0
    r = fit_gaussian_portrait('111', data[None], x0[:-1], 0.0, sig, vary[:-1], False, np.arange(nbin), [nu_ref], nu_ref,
                              quiet=True, engine=engine,
                              evaluator=None if evaluator_factory is None else
                              evaluator_factory(data[None], sig, '111', np.array([nu_ref]), nu_ref))
    pick = np.r_[0, 1, np.arange(2, 2 + 6 * ng, 2)]
    fitted, fit_errs = r.fitted_params[pick], r.fit_errs[pick]
    residuals = r.residuals[0]
    if not quiet:
        print("---------------------------------------------------------------")
        print("Multi-Gaussian Profile Fit Results")
        print("---------------------------------------------------------------")
        print("fit status:", r.lm_results.message)
        print("Gaussians:", ng)
        print("DoF:", r.dof)
        print("reduced chi-sq: %.2f" % (r.chi2 / r.dof))
        print("residuals mean: %.3g" % np.mean(residuals))
        print("residuals std.: %.3g" % np.std(residuals))
        print("---------------------------------------------------------------")
    return DataBunch(fitted_params=fitted, fit_errs=fit_errs, residuals=residuals, chi2=r.chi2, dof=r.dof)
