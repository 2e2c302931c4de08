"""NumPy restatement of the narrowband scattering fit (one profile, phase and
scattering time), for the tests of pp_fit_phase_tau_batch.

The objective is the wideband one (pptoaslib.py:390-643) with a single channel:

    C(phi, tau) = Re sum_k d_k conj(m_k) conj(B_k) e^{2 pi i k phi} / sigma_F^2
    S(tau)      = sum_k |B_k|^2 |m_k|^2 / sigma_F^2,     B_k = 1 / (1 + 2 pi i k tau)
    f           = -C^2 / S

over the harmonics k = 1 .. nbin/2 (no DC term, the Nyquist term kept), with
sigma_F^2 = sigma^2 nbin / 2.  Written from the formulas, with the derivatives of
B_k taken in closed form:  dB*/dtau = i w B*^2,  d2B*/dtau2 = -2 w^2 B*^3,
|B|^2 = q = 1 / (1 + w^2 tau^2),  dq/dtau = -2 w^2 tau q^2,
d2q/dtau2 = -2 w^2 q^2 (1 - 4 w^2 tau^2 q),  w = 2 pi k.
"""
import numpy as np
import scipy.optimize as opt

LN10 = np.log(10.0)
NOUT = 11
COLS = ("phi", "phi_err", "tau", "tau_err", "scale", "scale_err", "snr", "red_chi2", "cov_phi_tau", "nfeval",
        "return_code")


def measured_noise(dft, nbin):
    """Time-domain sigma from the top quarter of the power spectrum (get_noise_PS)."""
    H = nbin // 2 + 1
    kc = int(0.75 * H)
    return np.sqrt((np.abs(dft[kc:]) ** 2).sum() / nbin / (H - kc))


def spectra(prof, model, sigma=None):
    """X_k = d_k conj(m_k) / sigma_F^2, p_k = |m_k|^2 / sigma_F^2 for k = 1 .. M, and Sd."""
    prof, model = np.asarray(prof, dtype=np.float64), np.asarray(model, dtype=np.float64)
    nbin = prof.shape[-1]
    d, m = np.fft.rfft(prof), np.fft.rfft(model)
    if sigma is None or not (sigma >= 0.0):
        sigma = measured_noise(d, nbin)
    s2 = sigma * sigma * nbin / 2.0
    d, m = d[1:], m[1:]
    return d * np.conj(m) / s2, np.abs(m) ** 2 / s2, (np.abs(d) ** 2).sum() / s2


def sums(X, p, phi, tau):
    """The nine sums in (phi, tau): C, C_phi, C_phiphi, C_tau, C_tautau, C_phitau, S, S_tau, S_tautau."""
    k = np.arange(1, len(X) + 1, dtype=np.float64)
    w = 2.0 * np.pi * k
    z = X * np.exp(1j * w * phi)
    x = w * tau
    q = 1.0 / (1.0 + x * x)
    Bc = q * (1.0 + 1j * x)              # conj(B)
    zb, zb2 = z * Bc, z * Bc * Bc
    zb3 = zb2 * Bc
    return np.array([zb.real.sum(), -(w * zb.imag).sum(), -(w * w * zb.real).sum(),
                     -(w * zb2.imag).sum(), -2.0 * (w * w * zb3.real).sum(), -(w * w * zb2.real).sum(),
                     (p * q).sum(), (-2.0 * w * w * tau * p * q * q).sum(),
                     (-2.0 * w * w * p * q * q * (1.0 - 4.0 * x * x * q)).sum()])


def param_sums(X, p, x, log10_tau):
    """The nine sums with the second parameter as fitted: tau itself or t = log10 tau (chain rule)."""
    phi, t = x
    tau = 10.0 ** t if log10_tau else t
    s = sums(X, p, phi, tau)
    if log10_tau:
        t1, t2 = LN10 * tau, LN10 * LN10 * tau
        C, Cp, Cpp, Ct, Ctt, Cpt, S, St, Stt = s
        s = np.array([C, Cp, Cpp, Ct * t1, Ctt * t1 * t1 + Ct * t2, Cpt * t1, S, St * t1, Stt * t1 * t1 + St * t2])
    return s


def fgh(X, p, x, log10_tau):
    """f, its gradient [2] and Hessian [2, 2] at x = (phi, tau or log10 tau)."""
    C, Cp, Cpp, Ct, Ctt, Cpt, S, St, Stt = param_sums(X, p, x, log10_tau)
    dC, dS = np.array([Cp, Ct]), np.array([0.0, St])
    d2C, d2S = np.array([[Cpp, Cpt], [Cpt, Ctt]]), np.array([[0.0, 0.0], [0.0, Stt]])
    f = -C * C / S
    g = f * (2.0 * dC / C - dS / S)
    h = 2.0 * f * (d2C / C - 0.5 * d2S / S + np.outer(dC, dC) / C ** 2 + np.outer(dS, dS) / S ** 2
                   - (np.outer(dC, dS) + np.outer(dS, dC)) / (C * S))
    return f, g, h


def postfit(X, p, Sd, x, log10_tau, nbin):
    """Errors from the Hessian with the amplitude in it (3 x 3: phi, tau, a), one channel of
    fit_portrait_full_function_2deriv_with_scales: returns the NOUT columns but nfeval and return_code."""
    C, Cp, Cpp, Ct, Ctt, Cpt, S, St, Stt = param_sums(X, p, x, log10_tau)
    a = C / S
    A = -2.0 * a * (np.array([[Cpp, Cpt], [Cpt, Ctt]]) - 0.5 * a * np.array([[0.0, 0.0], [0.0, Stt]]))
    U = -2.0 * (np.array([Cp, Ct]) - a * np.array([0.0, St]))
    Xi = np.linalg.inv(A - np.outer(U, U) / (2.0 * S))
    cov = 2.0 * Xi
    var_a = 2.0 * (1.0 / (2.0 * S) + (U @ Xi @ U) / (2.0 * S) ** 2)
    f = -C * C / S
    phi = x[0]
    if abs(phi) >= 0.5:
        phi %= 1.0
    if phi >= 0.5:
        phi -= 1.0
    return np.array([phi, np.sqrt(cov[0, 0]), x[1], np.sqrt(cov[1, 1]), a, np.sqrt(var_a), a * np.sqrt(S),
                     (Sd + f) / (nbin - 3), cov[0, 1]])


def seed_phase(X, p, tau, lo=-0.5, hi=0.5, Ns=100):
    """The grid point of the largest correlation at a fixed tau (fit_phase_shift's brute grid)."""
    k = np.arange(1, len(X) + 1, dtype=np.float64)
    x = 2.0 * np.pi * k * tau
    Y = X * (1.0 + 1j * x) / (1.0 + x * x)
    grid = np.arange(Ns) * ((hi - lo) / (Ns - 1)) + lo if Ns > 1 else np.array([lo])
    c = (Y[None, :] * np.exp(2j * np.pi * np.outer(grid, k))).real.sum(axis=1)
    return grid[int(np.argmax(c))]


def fit(prof, model, sigma, tau_guess, phi_guess=None, log10_tau=True, lo=-0.5, hi=0.5, Ns=100):
    """The fit by SciPy, run to a tight gradient: the NOUT columns (nfeval = SciPy's, return_code 2)."""
    nbin = len(prof)
    X, p, Sd = spectra(prof, model, sigma)
    tau0 = 10.0 ** tau_guess if log10_tau else tau_guess
    phi0 = seed_phase(X, p, tau0, lo, hi, Ns) if phi_guess is None or np.isnan(phi_guess) else phi_guess
    x = np.array([phi0, tau_guess], dtype=np.float64)
    nfev = 0
    for _ in range(3):        # (restarts: each ends where f stops changing; the last starts at the optimum)
        r = opt.minimize(lambda y: fgh(X, p, y, log10_tau)[0], x, jac=lambda y: fgh(X, p, y, log10_tau)[1],
                         hess=lambda y: fgh(X, p, y, log10_tau)[2], method="trust-exact",
                         options=dict(gtol=1e-13 * abs(fgh(X, p, x, log10_tau)[0])))
        x, nfev = r.x, nfev + r.nfev
    for _ in range(3):        # Newton on the gradient: below what a comparison of f values resolves
        f, g, h = fgh(X, p, x, log10_tau)
        x = x - np.linalg.solve(h, g)
    return np.concatenate([postfit(X, p, Sd, x, log10_tau, nbin), [nfev, 2.0]])


def tau_guesses(scat_guess, gmodel_tau_s, gmodel_nu_ref, gmodel_alpha, default_alpha, freqs, P, nbin, log10_tau):
    """The per-channel guess recipe of get_narrowband_TOAs(fit_scat=True), restated for the tests."""
    freqs = np.asarray(freqs, dtype=np.float64)
    if scat_guess is not None:
        tau_s, nu_ref, alpha = scat_guess
        tau = (tau_s / P) * (freqs / nu_ref) ** alpha
    elif gmodel_tau_s is not None:
        alpha = default_alpha if gmodel_alpha is None else gmodel_alpha
        tau = (gmodel_tau_s / P) * (freqs / gmodel_nu_ref) ** alpha
    else:
        tau = np.zeros(len(freqs))
    if log10_tau:
        tau = np.log10(np.where(tau == 0.0, 1.0 / nbin, tau))
    return tau
