"""Plain references of what the rotation, per-channel chi^2 and 1-D phase-fit kernels compute (pp_extra.h k_rotate,
k_chan_chi2, k_fps; pp_anybin.h k_rotate_any, k_chan_chi2_harm), written from the formulas (rotate_data /
rotate_portrait_full, get_channels_to_zap's time-domain chi^2, fit_phase_shift): NumPy and np.longdouble only, no GPU,
nothing imported from the package.  tests/test_rot_refs_cpu.py pins each of them to the oracle and to closed forms;
tests/test_gpu_rot_kernels.py holds the kernels against them.  The second half builds the inputs both files share.

A direct long-double transform of an 8192-bin row takes about a second, so the references are used for a few rows of
a case (ld_rows) and cached; every other row is held to the f64 oracle."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

LD = np.longdouble
PI2 = 8 * np.arctan(LD(1))
DCONST = LD(0.000241 ** -1)          # the f64 constant the oracle and the device share

POW2 = [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
ANY = [8, 62, 66, 254, 258, 1022, 1026, 4094, 250]     # both ends of every chirp-z class, and M = 125 (odd)
ALL = POW2 + ANY


def is_pow2(nbin):
    return nbin & (nbin - 1) == 0


def rot_bar(nbin):
    """The rounding-level bar of one rotation, as a fraction of the row's maximum (tests/test_gpu_ppalign.py)."""
    return 2e-13 if is_pow2(nbin) else 2e-12


# ---- transforms -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _table(nbin):
    """cos and sin of 2 pi j / nbin, j = 0 .. nbin - 1."""
    ang = np.arange(nbin, dtype=LD) * PI2 / nbin
    return np.cos(ang), np.sin(ang)


_BLOCK = 1 << 21      # table entries gathered at a time


def _dft_sums(x, rows, nbin):
    """sum_j x_j cos(2 pi rows_r j / nbin) and the same with sin, for every r: the angle index (r j) mod nbin is
    formed in integers, so the angles are reduced exactly."""
    cs, sn = _table(nbin)
    x = np.asarray(x, dtype=LD)
    cols = np.arange(len(x), dtype=np.int64)
    c, s = np.empty(len(rows), dtype=LD), np.empty(len(rows), dtype=LD)
    step = max(1, _BLOCK // max(1, len(x)))
    for r0 in range(0, len(rows), step):
        idx = np.outer(rows[r0:r0 + step], cols) % nbin
        c[r0:r0 + step] = np.dot(cs[idx], x)
        s[r0:r0 + step] = np.dot(sn[idx], x)
    return c, s


def rfft_ld(row):
    """(re, im) of harmonics 0 .. nbin / 2 of a real row: X_k = sum_j x_j e^{-2 pi i j k / nbin}."""
    nbin = len(row)
    c, s = _dft_sums(row, np.arange(nbin // 2 + 1, dtype=np.int64), nbin)
    return c, -s


def irfft_ld(re, im, nbin):
    """The real row of harmonics 0 .. nbin / 2; the imaginary parts of DC and Nyquist are dropped, as irfft does."""
    M = nbin // 2
    re, im = np.asarray(re, dtype=LD), np.asarray(im, dtype=LD)
    # x_j = (X_0 + (-1)^j Re X_M + 2 sum_{k=1}^{M-1} (Re X_k cos(2 pi j k / nbin) - Im X_k sin(2 pi j k / nbin))) / nbin
    body = np.zeros(nbin, dtype=LD)
    if M > 1:
        cs, sn = _table(nbin)
        ks = np.arange(1, M, dtype=np.int64)
        step = max(1, _BLOCK // len(ks))
        for j0 in range(0, nbin, step):
            idx = np.outer(np.arange(j0, min(nbin, j0 + step), dtype=np.int64), ks) % nbin
            body[j0:j0 + step] = 2 * (np.dot(cs[idx], re[1:M]) - np.dot(sn[idx], im[1:M]))
    alt = np.where(np.arange(nbin) % 2 == 0, LD(1), LD(-1))
    return (re[0] + alt * re[M] + body) / nbin


def _ld_int(v):
    """A Python int below 2^117 as a long double, without a pass through f64."""
    hi, lo = divmod(int(v), 1 << 53)
    return LD(hi) * LD(2) ** 53 + LD(lo)


def turns_ld(k, phi):
    """frac(k phi) for the integers k, formed exactly from the f64 phi as a fraction and only then converted: the
    device's unit_phasor forms k phi mod 1 exactly, NumPy's k * phi carries a rounding of the product."""
    f = Fraction(float(phi))
    num, den = f.numerator, f.denominator          # (den is a power of two)
    out = np.empty(np.shape(k), dtype=LD)
    flat = out.reshape(-1)
    for i, kk in enumerate(np.asarray(k).reshape(-1)):
        flat[i] = _ld_int((int(kk) * num) % den) / _ld_int(den)
    return out


def phasor_ld(k, phi):
    t = turns_ld(k, phi) * PI2
    return np.cos(t), np.sin(t)


def rotate_ld(row, phi_n):
    """rotate_data of one row: harmonics times e^{2 pi i k phi_n}, the Nyquist harmonic keeps its real part only."""
    nbin = len(row)
    re, im = rfft_ld(row)
    c, s = phasor_ld(np.arange(nbin // 2 + 1), phi_n)
    return irfft_ld(re * c - im * s, re * s + im * c, nbin)


# ---- the delay law --------------------------------------------------------------------------------------
def delay_terms_ld(phi, DM, GM, nu, nu_DM, nu_GM, P):
    """The five terms of phi_n = phi + Dconst DM (nu^-2 - nu_DM^-2) / P + Dconst^2 GM (nu^-4 - nu_GM^-4) / P, signed;
    an infinite reference frequency contributes 0."""
    phi, DM, GM, nu, P = LD(phi), LD(DM), LD(GM), LD(nu), LD(P)
    iDM = LD(0) if np.isinf(nu_DM) else LD(nu_DM) ** -2
    iGM = LD(0) if np.isinf(nu_GM) else LD(nu_GM) ** -4
    return [phi, DCONST * DM * nu ** -2 / P, -DCONST * DM * iDM / P,
            DCONST ** 2 * GM * nu ** -4 / P, -DCONST ** 2 * GM * iGM / P]


def delay_ld(phi, DM, GM, nu, nu_DM, nu_GM, P):
    t = delay_terms_ld(phi, DM, GM, nu, nu_DM, nu_GM, P)
    return t[0] + (t[1] + t[2]) + (t[3] + t[4])


# ---- per-channel reduced chi^2 ---------------------------------------------------------------------------
def scatter_ld(model_row, tau_n):
    """irfft(rfft(row) / (1 + 2 pi i k tau_n)); the row itself when tau_n = 0."""
    if tau_n == 0:
        return np.asarray(model_row, dtype=LD)
    nbin = len(model_row)
    re, im = rfft_ld(model_row)
    x = PI2 * np.arange(nbin // 2 + 1, dtype=LD) * LD(tau_n)
    den = 1 / (1 + x * x)
    return irfft_ld((re + im * x) * den, (im - re * x) * den, nbin)


def chan_red_chi2_ld(data_row, model_row, phi_n, tau_n, scale, sigma):
    """Time domain, as get_channels_to_zap forms it: the rotated data minus scale x the scattered template, squared
    and summed over the bins, / sigma^2 / (nbin - 2).  (The device sums the residual's spectrum instead.)"""
    nbin = len(data_row)
    r = rotate_ld(data_row, phi_n) - LD(scale) * scatter_ld(model_row, tau_n)
    return np.sum(r * r) / LD(sigma) ** 2 / (nbin - 2)


def zero_scale_chi2(data_row, phi_n, sigma):
    """The chi^2 of a channel of scale 0 without a transform: a rotation keeps the sum of squares of everything but the
    Nyquist harmonic X_M = sum (-1)^j d_j, of which only the real part cos(2 pi M phi_n) X_M survives, so it is
    (sum d^2 - X_M^2 sin^2(2 pi M phi_n) / nbin) / sigma^2 / (nbin - 2)."""
    d = np.asarray(data_row, dtype=LD)
    nbin = len(d)
    xm = np.sum(d[0::2]) - np.sum(d[1::2])
    s = np.sin(PI2 * turns_ld(np.array([nbin // 2]), phi_n)[0])
    return float((np.sum(d * d) - (xm * s) ** 2 / nbin) / LD(sigma) ** 2 / (nbin - 2))


# ---- 1-D phase fit ---------------------------------------------------------------------------------------
_SPEC = {}


def _spec_ld(row):
    """rfft_ld of a row, kept by the row's bytes (a fit's model and data rows are asked for at several phases)."""
    row = np.ascontiguousarray(row, dtype=np.float64)
    key = row.tobytes()
    if key not in _SPEC:
        _SPEC[key] = rfft_ld(row)
    return _SPEC[key]


def _cross(data, model, ld):
    """(k, Re, Im) of d_k conj(m_k) for k = 1 .. M and (sum |d_k|^2, sum |m_k|^2) over those k (F0_fact = 0: no DC)."""
    if ld:
        (dr, di), (mr, mi) = _spec_ld(data), _spec_ld(model)
    else:
        d, m = np.fft.rfft(np.asarray(data, dtype=np.float64)), np.fft.rfft(np.asarray(model, dtype=np.float64))
        dr, di, mr, mi = d.real, d.imag, m.real, m.imag
    dr, di, mr, mi = dr[1:], di[1:], mr[1:], mi[1:]
    return (np.arange(1, len(dr) + 1), dr * mr + di * mi, di * mr - dr * mi,
            np.sum(dr * dr + di * di), np.sum(mr * mr + mi * mi))


def fps_objective_ld(data, model, phi, ld=True):
    """fit_phase_shift_function without its 1 / err^2 and its first two derivatives in phi:
    f = -sum_k Re(d_k conj(m_k) e^{2 pi i k phi}), k = 1 .. M.  ld = False takes the spectra from NumPy's f64 transform
    (the rows of a long case that get no long-double transform); the phasors and the sums are long double either way."""
    k, xr, xi, _, _ = _cross(data, model, ld)
    c, s = phasor_ld(k, phi)           # (exact turns also over f64 spectra: NumPy's k * phi would cost ~1e-13 at M = 4096)
    kk = k.astype(LD)
    re, im = xr * c - xi * s, xr * s + xi * c
    return -np.sum(re), PI2 * np.sum(kk * im), PI2 * PI2 * np.sum(kk * kk * re)


def noise_ps_row(data, ld=True):
    """get_noise_PS(row): sqrt of the mean of |rfft|^2 / nbin over the top quarter of the harmonics."""
    nbin = len(data)
    if ld:
        re, im = _spec_ld(data)
    else:
        d = np.fft.rfft(np.asarray(data, dtype=np.float64))
        re, im = d.real, d.imag
    pows = (re * re + im * im) / nbin
    return np.sqrt(np.mean(pows[int(0.75 * len(pows)):]))


def fps_columns(data, model, noise, phi, ld=True):
    """[phase_err, scale, scale_err, snr, red_chi2] of fit_phase_shift, evaluated at the phase phi.  A noise that is
    None, NaN or negative is measured from the data (get_noise_PS), as the device decides with !(noise >= 0)."""
    nbin = len(data)
    if noise is None or not (noise >= 0):
        noise = noise_ps_row(data, ld)
    err2 = (LD(noise) if ld else float(noise)) ** 2 * nbin / 2
    _, _, _, dd, pp = _cross(data, model, ld)
    f, _, f2 = fps_objective_ld(data, model, phi, ld)
    f, f2, d, p = f / err2, f2 / err2, dd / err2, pp / err2
    scale = -f / p
    return np.array([(scale * f2) ** -0.5, scale, p ** -0.5, (scale * scale * p) ** 0.5,
                     (d - f * f / p) / (nbin - 2)], dtype=LD if ld else np.float64)


def grid_values(data, model, lo, hi, Ns):
    """f at the Ns points of scipy.optimize.brute's grid (numpy's mgrid arithmetic: j * step + lo), f64."""
    k, xr, xi, _, _ = _cross(data, model, False)
    if Ns == 1:
        pts = np.array([lo])
    else:
        pts = np.arange(Ns) * ((hi - lo) / (Ns - 1)) + lo
    if Ns * len(k) <= 1 << 20:
        ang = 2 * np.pi * np.outer(pts, k)
        return pts, -(np.cos(ang) @ xr - np.sin(ang) @ xi)
    # a long grid of long rows: the powers of e^{2 pi i phi_j} by recurrence (~1e-12 of |f| after 4096 steps, three
    # orders under the lead the grid decisions are asked to have)
    z = np.exp(2j * np.pi * pts)
    w, acc = z.copy(), np.zeros(Ns, dtype=np.complex128)
    for x in xr + 1j * xi:
        acc += x * w
        w *= z
    return pts, -acc.real


# ==== inputs shared by the CPU and the GPU file ============================================================
def f32_exact(a):
    """`a` rounded to values f32 holds exactly, as f64: one reference serves the f64 and the f32 call."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def gauss_profile(nbin, loc, wid):
    """A periodic Gaussian of FWHM `wid` rotations at phase `loc`, peak 1."""
    ph = (np.arange(nbin) + 0.5) / nbin
    d = (ph - loc + 0.5) % 1.0 - 0.5
    return np.exp(-4 * np.log(2.0) * (d / wid) ** 2)


def ld_rows(nbin, nrows):
    """The rows of a 3 x 5 cube that get a long-double reference: two at nbin >= 4094 -- one of each subint whose phase is
    no whole or half bin, where NumPy's k * phi rounds --, four spread over the subints below."""
    if nbin >= 4094:
        return [0, 7]
    return sorted({int(r) for r in np.linspace(0, nrows - 1, 4).round()})


# ---- A. rotation ----------------------------------------------------------------------------------------
ROT_FREQS = np.linspace(1200.0, 1700.0, 5)


def a1_phis(nbin):
    return np.array([0.1234, -0.31, 0.5 / nbin])


@lru_cache(maxsize=None)
def a1_cube(nbin):
    """3 subints x 5 channels: two components on an offset plus white noise at a tenth of the peak, so every harmonic
    up to Nyquist carries power; f32-exact.  (At a third of the peak NumPy's own k * phi rounding puts the ORACLE 2.5e-13
    of the row's maximum from the long-double rows at 8192 bins and phi = -0.31, outside the 2e-13 it is to stand under;
    tests/test_rot_refs_cpu.py asserts and prints that distance for the rows used.)"""
    rng = np.random.default_rng(1000 + nbin)
    prof = 0.2 + gauss_profile(nbin, 0.3, 0.04) + 0.5 * gauss_profile(nbin, 0.62, 0.11)
    x = f32_exact(rng.uniform(0.5, 2.0, (3, 5, 1)) * prof + rng.normal(0, 0.1, (3, 5, nbin)))
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def a1_reference(nbin):
    """{(i, n): rotate_ld row} for the long-double rows of a1_cube."""
    x, phis = a1_cube(nbin), a1_phis(nbin)
    return {(r // 5, r % 5): rotate_ld(x[r // 5, r % 5], phis[r // 5]) for r in ld_rows(nbin, 15)}


A2_NAMES = ["dc", "nyquist_0", "nyquist_half_bin", "nyquist_one_bin", "cos_1", "cos_M-1", "zero"]


def a2_phis(nbin):
    return np.array([0.1234, 0.0, 0.5 / nbin, 1.0 / nbin, 0.1234, -0.31, 0.1234])


def _cos_ld(nbin, k, phi):
    """cos(2 pi k (j / nbin + phi)) for every bin j, the angle reduced exactly."""
    cs, sn = _table(nbin)
    idx = (np.arange(nbin, dtype=np.int64) * k) % nbin
    c, s = phasor_ld(np.array([k]), phi)
    return cs[idx] * c[0] - sn[idx] * s[0]


def a2_rows(nbin, dtype=np.float64):
    """7 subints x 2 channels (the second is -2 x the first, exactly) in `dtype`, and the exact rotated rows in long
    double.  The cosine rows are rounded to `dtype`; rotation is linear, so their expectation is the moved cosine plus
    the rotation of the rounding residual, which NumPy's f64 rotation gives to ~1e-13 of the residual."""
    M = nbin // 2
    phis = a2_phis(nbin)
    j = np.arange(nbin)
    alt = np.where(j % 2 == 0, 1.0, -1.0)
    rows = np.zeros((7, 2, nbin), dtype=dtype)
    want = np.zeros((7, nbin), dtype=LD)
    rows[0, 0] = 1.5
    want[0] = 1.5
    for i in (1, 2, 3):
        rows[i, 0] = alt
        want[i] = np.cos(PI2 * turns_ld(np.array([M]), phis[i])[0]) * alt.astype(LD)
    for i, k in ((4, 1), (5, M - 1)):
        exact = _cos_ld(nbin, k, 0.0)
        rows[i, 0] = exact.astype(dtype)
        resid = (rows[i, 0].astype(LD) - exact).astype(np.float64)
        kk = np.arange(M + 1)
        moved = np.fft.irfft(np.fft.rfft(resid) * np.exp(2j * np.pi * kk * phis[i]), nbin)
        want[i] = _cos_ld(nbin, k, phis[i]) + moved
    rows[:, 1] = -2 * rows[:, 0]
    return rows, np.stack([want, -2 * want], axis=1)


A3_NBINS = [256, 1024, 8192, 250, 4094]
A3_P = np.array([0.005, 0.0031, 0.0123])
A3_DM = np.array([0.0, 3e-3, -2e-3])
A3_GM = np.array([0.0, 0.2, 0.0])
A3_PHI = np.array([0.1234, -0.31, 0.04321])
A3_REFS = [(1400.0, 1300.0), (np.inf, np.inf)]


def a3_freqs():
    """Per-subint frequency rows [3, 5]."""
    return np.stack([ROT_FREQS, ROT_FREQS + 7.5, ROT_FREQS[::-1] - 3.25])


def a3_delays(nu_DM, nu_GM):
    """(phi_n as f64 of the long-double value, u = 8 * 2^-53 * the summed absolute terms) for every (subint, channel)."""
    fr = a3_freqs()
    phin, u = np.empty((3, 5)), np.empty((3, 5))
    for i in range(3):
        for n in range(5):
            t = delay_terms_ld(A3_PHI[i], A3_DM[i], A3_GM[i], fr[i, n], nu_DM, nu_GM, A3_P[i])
            phin[i, n] = float(delay_ld(A3_PHI[i], A3_DM[i], A3_GM[i], fr[i, n], nu_DM, nu_GM, A3_P[i]))
            u[i, n] = 8 * 2.0 ** -53 * float(sum(abs(v) for v in t))
    return phin, u


@lru_cache(maxsize=None)
def a3_reference(nbin, iref):
    """{(i, n): rotate_ld row} of a1_cube(nbin) under the delay law with reference frequencies A3_REFS[iref]; the
    rows with DM and GM are preferred (subint 1 first)."""
    phin, _ = a3_delays(*A3_REFS[iref])
    x = a1_cube(nbin)
    picks = [(1, 0), (2, 4)] if nbin >= 4094 else [(1, 0), (1, 3), (2, 4), (0, 2)]
    return {p: rotate_ld(x[p], phin[p]) for p in picks}


# ---- B. per-channel chi^2 --------------------------------------------------------------------------------
B_NSUB, B_NCHAN = 4, 6
B_SLOTS = [0, 1, 1, 0]
B_P = np.array([0.004, 0.0052, 0.0033, 0.0047])
B_OFFSET = 0.02       # a baseline well under sigma_n: part of the residual (the DC term), chi^2 stays near 1


def b_templates(nbin):
    """Two templates [2, 6, nbin]: smooth two-component profiles of different width on a DC offset, plus a +-0.01
    alternating term, so the model's DC and Nyquist terms matter."""
    alt = np.where(np.arange(nbin) % 2 == 0, 0.01, -0.01)
    out = np.empty((2, B_NCHAN, nbin))
    for s, (w1, w2) in enumerate(((0.05, 0.12), (0.09, 0.2))):
        for n in range(B_NCHAN):
            out[s, n] = 0.3 + (1.0 + 0.1 * n) * gauss_profile(nbin, 0.35, w1) + \
                0.4 * gauss_profile(nbin, 0.6 + 0.01 * n, w2) + alt
    return f32_exact(out)          # (a data row can then equal its template in f32 and in f64)


def b_freqs():
    base = np.linspace(1250.0, 1650.0, B_NCHAN)
    return np.stack([base, base + 4.0, base - 6.5, base[::-1] + 1.25])


@lru_cache(maxsize=None)
def b1_case(nbin):
    """Data = scale x the rotated (scattered) template + white noise sigma_n + an offset, f32-exact, with the
    parameters that made it.  Subints: (0) phi only, every reference frequency infinite; (1) phi and DM at a finite
    nu_DM; (2) phi, DM and GM; (3) phi, DM and a linear tau = 0.01 rot with alpha = -4 at nu_tau.  scales[1, 2] < 0,
    scales[2, 3] = 0."""
    rng = np.random.default_rng(2000 + nbin)
    tm = b_templates(nbin)
    fr = b_freqs()
    params = np.array([[0.1234, 0.0, 0.0, 0.0, 0.0],
                       [-0.31, 2.5e-3, 0.0, 0.0, 0.0],
                       [0.04321, -1.5e-3, 0.15, 0.0, 0.0],
                       [0.27, 1e-3, 0.0, 0.01, -4.0]])
    nu_refs = np.array([[np.inf, np.inf, np.inf], [1400.0, np.inf, np.inf], [1450.0, 1350.0, np.inf],
                        [1500.0, np.inf, 1480.0]])
    scales = rng.uniform(0.8, 3.0, (B_NSUB, B_NCHAN))
    scales[1, 2] = -1.25
    scales[2, 3] = 0.0
    sigma = rng.uniform(0.05, 0.2, (B_NSUB, B_NCHAN))
    k = np.arange(nbin // 2 + 1)
    data = np.empty((B_NSUB, B_NCHAN, nbin))
    phin, taun = np.empty((B_NSUB, B_NCHAN)), np.zeros((B_NSUB, B_NCHAN))
    for i in range(B_NSUB):
        for n in range(B_NCHAN):
            phin[i, n] = float(delay_ld(params[i, 0], params[i, 1], params[i, 2], fr[i, n], nu_refs[i, 0],
                                        nu_refs[i, 1], B_P[i]))
            if params[i, 3] != 0:
                taun[i, n] = params[i, 3] * (fr[i, n] / nu_refs[i, 2]) ** params[i, 4]
            m = np.fft.rfft(tm[B_SLOTS[i], n])
            if taun[i, n] != 0:
                m = m / (1 + 2j * np.pi * k * taun[i, n])
            # the data are the template rotated the other way, so that rotating by phi_n brings them back onto it
            data[i, n] = scales[i, n] * np.fft.irfft(m * np.exp(-2j * np.pi * k * phin[i, n]), nbin) + \
                rng.normal(0, sigma[i, n], nbin) + B_OFFSET
    data = f32_exact(data)
    data.setflags(write=False)
    return dict(data=data, templates=tm, freqs=fr, P=B_P, params=params, nu_refs=nu_refs, scales=scales, sigma=sigma,
                phin=phin, taun=taun)


@lru_cache(maxsize=None)
def b1_reference(nbin):
    """{(i, n): chan_red_chi2_ld} for the long-double rows: the scattered subint and the negative scale first."""
    c = b1_case(nbin)
    picks = [(3, 1), (1, 2)] if nbin >= 4094 else [(3, 1), (1, 2), (0, 0), (2, 3), (2, 5)]
    return {p: chan_red_chi2_ld(c["data"][p], c["templates"][B_SLOTS[p[0]], p[1]], c["phin"][p], c["taun"][p],
                                c["scales"][p], c["sigma"][p]) for p in picks}


# ---- C. 1-D phase fit ------------------------------------------------------------------------------------
C_NBINS = [32, 64, 256, 2048, 4096, 8192, 8, 62, 1000, 4094]
# (every shift lies inside both bounds of C_BOUNDS, more than a grid step of Ns = 100 from their ends: the polish
# looks no further than one grid step from the best grid point)
C_SHIFTS = np.array([0.1234, -0.21, 0.017, 0.34, -0.08])
C_SNR = np.array([30.0, 30.0, 30.0, 3.0, 30.0])


@lru_cache(maxsize=None)
def c_case(nbin):
    """(data[5, nbin], model[5, nbin], sigma[5]): two Gaussians turned to later phase by C_SHIFTS plus white noise at
    peak / C_SNR."""
    rng = np.random.default_rng(3000 + nbin)
    wid = max(0.05, 1.5 / nbin)
    model = gauss_profile(nbin, 0.4, wid) + 0.45 * gauss_profile(nbin, 0.55, 2.2 * wid)
    k = np.arange(nbin // 2 + 1)
    sigma = model.max() / C_SNR
    data = np.stack([np.fft.irfft(np.fft.rfft(model) * np.exp(-2j * np.pi * k * s), nbin) * 1.7 +
                     rng.normal(0, sg, nbin) for s, sg in zip(C_SHIFTS, sigma)])
    data.setflags(write=False)
    return data, np.tile(model, (5, 1)), sigma


def c_ld_pairs(nbin):
    """The pairs of a batch whose optimum is judged by the long-double objective (the others by the f64 one)."""
    return [0, 3] if nbin >= 4094 else [0, 1, 2, 3, 4]


C_NS = lambda nbin: [1, 2, 100, 257, nbin]                       # noqa: E731
C_BOUNDS = {"tie": (-0.5, 0.5), "plain": (-0.3, 0.4)}


def c_grid_margin(nbin, i, lo, hi, Ns):
    """(index of the best grid point, its lead over the runner-up as a fraction of |f|).  When hi - lo = 1 the two
    ends are one phase and tie exactly (c_ends_tie); the device's argmin takes the lower index, so the last point is
    left out here and index 0 stands for both."""
    data, model, _ = c_case(nbin)
    _, f = grid_values(data[i], model[i], lo, hi, Ns)
    if Ns == 1:
        return 0, np.inf
    if hi - lo == 1.0:
        f = f[:-1]
        if len(f) == 1:
            return 0, np.inf
    best = int(np.argmin(f))
    return best, float((np.delete(f, best).min() - f[best]) / abs(f[best]))


def c_ends_tie(nbin, i, lo, hi):
    """The exact objective at lo and hi is one number when they are one phase: k lo and k hi are the same turns."""
    data, model, _ = c_case(nbin)
    ld = nbin < 4094 or i in c_ld_pairs(nbin)
    a, b = fps_objective_ld(data[i], model[i], lo, ld=ld), fps_objective_ld(data[i], model[i], hi, ld=ld)
    k = np.arange(1, nbin // 2 + 1)
    return bool(np.array_equal(turns_ld(k, lo), turns_ld(k, hi))) and (not ld or a[0] == b[0])
