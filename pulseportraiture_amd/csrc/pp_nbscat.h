// Narrowband scattering fits on the device (included at the end of pp_toas.hip, after pp_gaussfit.h): phase and
// scattering time of one profile against its template profile, a batch of independent two-parameter problems.
//
// For the harmonics k = 1 .. M = nbin / 2 of a profile pair (no DC term, the Nyquist term kept, as fps_body), with
// B_k(tau) = 1 / (1 + 2 pi i k tau), tau in rotations, and sigma_F^2 = sigma^2 nbin / 2:
//     C(phi, tau) = Re sum_k d_k conj(m_k) conj(B_k) e^{2 pi i k phi} / sigma_F^2
//     S(tau)      = sum_k |B_k|^2 |m_k|^2 / sigma_F^2
//     f = -C^2 / S,    a = C / S
// which is the wideband objective (pptoaslib.py:390-643) with one channel.  With w = 2 pi k and q = |B|^2 =
// 1 / (1 + w^2 tau^2):  conj(B) = q (1 + i w tau),  d conj(B) / dtau = i w conj(B)^2,  d2 conj(B) / dtau2 =
// -2 w^2 conj(B)^3,  dq / dtau = -2 w^2 tau q^2,  d2q / dtau2 = -2 w^2 q^2 (1 - 4 w^2 tau^2 q): no division by tau,
// so tau = 0 is an ordinary point.  One pass over the harmonics gives the nine sums C, C_phi, C_phiphi, C_tau,
// C_tautau, C_phitau, S, S_tau, S_tautau; under log10_tau the chain rule of scattering_times_deriv / _2deriv
// (pptoaslib.py:246-274) turns them into derivatives by t = log10 tau.
//
// One 256-thread workgroup per pair (k_fps's form): the cross-spectrum d_k conj(m_k) and |m_k|^2 sit in LDS (48 KB at
// M = 2048), thread t walks harmonics t + 1, t + 257, ... with the phasor recurrence of fps_sums, and block_sum adds
// the threads' parts in a fixed order: a pair's answer is a function of that pair alone, bit for bit.  Every scalar of
// the solver is computed by every thread from those sums, so the control flow is uniform and every barrier is reached
// by the whole workgroup.

namespace pp {

// (PP_NBS_NOUT = 11 outputs per pair: include/pp_toas.h)
#define PP_NBS_MAXEV 64       // evaluations of the nine sums per pair, at most
#define PP_NBS_MINSNR 6.0     // a pair fitted below this S/N is no detection: see nbs_body

struct NbsArgs {
    const cplx* spec;         // rows alternate data_i, model_i, M + 1 harmonics each
    const double* noise;      // [nprof] time-domain sigma, NaN / < 0 = measure (null: measure all)
    const double* guess;      // [nprof][2]: phi (NaN = grid search), tau or log10 tau
    double* out;              // [nprof][PP_NBS_NOUT]
    double lo, hi;
    int Ns, M, nprof, log10_tau;
};

// this thread's part of the nine sums in (phi, tau) over its strided harmonics
__device__ __forceinline__ void nbs_part(const cplx* X, const double* p, int M, double phi, double tau, int vt,
                                         double (&u)[9]) {
#pragma unroll
    for (int q = 0; q < 9; ++q) u[q] = 0.0;
    if (vt >= M) return;
    cplx e = unit_phasor((double)(vt + 1), phi);
    const cplx wst = unit_phasor(256.0, phi);
    for (int j = vt; j < M; j += 256) {
        const double w = PP_TWO_PI * (double)(j + 1), w2 = w * w;
        const double x = w * tau, q = 1.0 / fma(x, x, 1.0);
        const cplx bc = make_double2(q, q * x);                 // conj(B_k)
        const cplx zb = cmul(cmul(X[j], e), bc), zb2 = cmul(zb, bc), zb3 = cmul(zb2, bc);
        u[0] += zb.x;
        u[1] = fma(-w, zb.y, u[1]);
        u[2] = fma(-w2, zb.x, u[2]);
        u[3] = fma(-w, zb2.y, u[3]);
        u[4] = fma(-2.0 * w2, zb3.x, u[4]);
        u[5] = fma(-w2, zb2.x, u[5]);
        const double pq = p[j] * q, pq2 = pq * q * w2;
        u[6] += pq;
        u[7] = fma(-2.0 * tau, pq2, u[7]);
        u[8] = fma(-2.0 * (1.0 - 4.0 * x * x * q), pq2, u[8]);
        e = cmul(e, wst);
    }
}

// value, gradient and Hessian of f = -C^2 / S from the nine sums (in the fitted parameters)
struct NbsEval {
    double f, g0, g1, h00, h01, h11;
};
__device__ __forceinline__ NbsEval nbs_fgh(const double (&s)[9]) {
    const double C = s[0], S = s[6], iC = 1.0 / C, iS = 1.0 / S;
    const double f = -C * C * iS;
    const double c0 = s[1] * iC, c1 = s[3] * iC, s1 = s[7] * iS;       // C_i / C, S_i / S (S_phi = 0)
    NbsEval r;
    r.f = f;
    r.g0 = f * 2.0 * c0;
    r.g1 = f * (2.0 * c1 - s1);
    r.h00 = 2.0 * f * (s[2] * iC + c0 * c0);
    r.h01 = 2.0 * f * (s[5] * iC + c0 * c1 - c0 * s1);
    r.h11 = 2.0 * f * (s[4] * iC - 0.5 * s[8] * iS + c1 * c1 + s1 * s1 - 2.0 * c1 * s1);
    return r;
}

// The minimiser of the quadratic model g.p + p.H.p / 2 inside |p| <= delta, 2 x 2: the eigenvalues and eigenvectors in
// closed form, the shift lam >= max(0, -l1) with |p(lam)| = delta by a safeguarded Newton iteration on 1 / |p| (at most
// 40 steps, bisection whenever Newton leaves the bracket).  interior: the Newton step itself.
__device__ inline void nbs_tr_step(const NbsEval& e, double delta, double& px, double& py, double& pred, bool& interior) {
    const double a = e.h00, b = e.h01, c = e.h11;
    const double mean = 0.5 * (a + c), diff = 0.5 * (a - c), r = hypot(diff, b);
    const double l1 = mean - r, l2 = mean + r;
    double vx, vy;                       // eigenvector of l2; (-vy, vx) is l1's
    if (diff >= 0.0) { vx = diff + r; vy = b; } else { vx = b; vy = r - diff; }
    const double n = hypot(vx, vy);
    if (n > 0.0) { vx /= n; vy /= n; } else { vx = 1.0; vy = 0.0; }
    const double g1 = -vy * e.g0 + vx * e.g1, g2 = vx * e.g0 + vy * e.g1;
    double p1 = 0.0, p2 = 0.0;
    interior = false;
    if (l1 > 0.0) {
        p1 = -g1 / l1; p2 = -g2 / l2;
        interior = hypot(p1, p2) <= delta;
    }
    if (!interior) {
        double lo = fmax(0.0, -l1), hi = lo + hypot(g1, g2) / delta, lam = hi;
        for (int it = 0; it < 40; ++it) {
            const double d1 = l1 + lam, d2 = l2 + lam;
            const double pn = (d1 > 0.0) ? hypot(g1 / d1, g2 / d2) : INFINITY;
            if (pn > delta) lo = lam; else hi = lam;
            double nl;
            if (d1 > 0.0 && pn > 0.0) {
                const double dpn = -(g1 * g1 / (d1 * d1 * d1) + g2 * g2 / (d2 * d2 * d2)) / pn;
                nl = lam + (1.0 / pn - 1.0 / delta) * (pn * pn) / dpn;
            } else nl = 0.5 * (lo + hi);
            if (!(nl > lo && nl < hi)) nl = 0.5 * (lo + hi);
            const bool done = fabs(nl - lam) <= 1e-14 * fabs(nl);
            lam = nl;
            if (done) break;
        }
        if (!(l1 + lam > 0.0)) lam = hi;
        p1 = -g1 / (l1 + lam); p2 = -g2 / (l2 + lam);
    }
    px = -vy * p1 + vx * p2;
    py = vx * p1 + vy * p2;
    pred = -(e.g0 * px + e.g1 * py) - 0.5 * (a * px * px + 2.0 * b * px * py + c * py * py);
}

__device__ __forceinline__ bool nbs_finite(double v) { return fabs(v) < INFINITY; }     // (false for NaN)

// The fit of pair i by 256 threads.  X[M] and p[M] are LDS work arrays.  Return codes (include/pp_toas.h):
//   PP_RC_STALL 2   converged: the Newton steps stopped shrinking (the rounding of the gradient)
//   PP_RC_MAXITER 1 PP_NBS_MAXEV evaluations spent; the outputs are those of the last accepted point
//   PP_RC_NAN 3     NaN / Inf in the data, the model, the noise or the guess; an all-zero data or model row (C = 0 or
//                   S = 0); a Hessian that is not positive definite at the end (no covariance); a linear tau more than
//                   3 tau_err below zero; a fitted S/N below PP_NBS_MINSNR (the tail of a profile that is not
//                   detected is fitted to the noise).  phi, tau, their errors and the covariance are NaN then; scale,
//                   snr and red_chi2 are NaN as well unless the fit itself ran to its end.
//                   Also a numerically singular Hessian (unscattered data: see the post-fit stage): the covariance is
//                   NaN, tau_err infinite, and phi, tau, phi_err and scale_err are those at fixed tau.
__device__ __forceinline__ void nbs_body(const NbsArgs& a, const int i, const int tid, cplx* X, double* p, double* scratch,
                                         double* shv, int* shj) {
    const int M = a.M, H = M + 1, kc = (int)(0.75 * H);
    const cplx* d = a.spec + (size_t)(2 * i) * H;
    const cplx* m = a.spec + (size_t)(2 * i + 1) * H;
    double* o = a.out + (size_t)i * PP_NBS_NOUT;
    auto give_up = [&](int nfev) {
        if (tid == 0) {
            for (int q = 0; q < 9; ++q) o[q] = NAN;
            o[9] = (double)nfev;
            o[10] = 3.0;
        }
    };
    double v[3];   // sum |d|^2, sum |m|^2, tail of |d|^2
    fps_bsum<3, 1>(v, scratch, tid, [&](const int vt, double (&u)[3]) __attribute__((always_inline)) {
        u[0] = u[1] = u[2] = 0.0;
        for (int k = 1 + vt; k <= M; k += 256) {
            const cplx dk = d[k], mk = m[k];
            X[k - 1] = cmulc(dk, mk);
            const double pm = cnorm(mk), pd = cnorm(dk);
            p[k - 1] = pm;
            u[0] += pd; u[1] += pm;
            if (k >= kc) u[2] += pd;
        }
    });
    const double B = 2.0 * M;
    double sig = a.noise ? a.noise[i] : NAN;
    if (!(sig >= 0.0)) sig = sqrt(v[2] / B / (double)(H - kc));      // get_noise_PS, as fps_body
    const double err2 = sig * sig * (0.5 * B), ierr2 = 1.0 / err2;
    const double Sd = v[0] * ierr2;
    const double phi_g = a.guess[2 * i], t_g = a.guess[2 * i + 1];
    const bool lg = a.log10_tau != 0;
    // the parameter box: a trial point outside it counts as a failed step, a guess outside it ends the pair
    auto in_box = [&](double t) { return lg ? (t >= -12.0 && t <= 3.0) : (fabs(t) <= 1e3); };
    if (!(nbs_finite(v[0]) && nbs_finite(v[1]) && v[0] > 0.0 && v[1] > 0.0 && err2 > 0.0 && nbs_finite(ierr2) &&
          nbs_finite(Sd) && in_box(t_g) && !(fabs(phi_g) == INFINITY))) {
        give_up(0);
        return;
    }
    auto tau_of = [&](double t) { return lg ? pow(10.0, t) : t; };
    double phi = phi_g;
    if (!(phi == phi)) {
        // ---- seed: the grid of fps_body over phi at the guessed tau, against the scattered model.  The cross-
        // spectrum takes conj(B_k(tau_0)) for the walk (every thread its own harmonics) and is restored after it
        const double tau0 = tau_of(t_g);
        if (tau0 != 0.0) {
            for (int j = tid; j < M; j += 256) {
                const double x = PP_TWO_PI * (double)(j + 1) * tau0, q = 1.0 / fma(x, x, 1.0);
                X[j] = cmul(X[j], make_double2(q, q * x));
            }
            __syncthreads();
        }
        const int Ns = a.Ns;
        double bestv = INFINITY;
        int bestj = 0x7fffffff;
        const double h = (Ns > 1) ? (a.hi - a.lo) / (double)(Ns - 1) : 0.5;
        for (int j = tid; j < Ns; j += 256) {
            const double ph = (Ns > 1) ? add_rn(mul_rn((double)j, h), a.lo) : a.lo;
            double s0, s1, s2;
            fps_sums(X, M, ph, 0, 1, s0, s1, s2);
            const double vv = -s0;
            if (vv < bestv) { bestv = vv; bestj = j; }
        }
        const int best = max(0, min(block_argmin256(bestv, bestj, shv, shj), Ns - 1));
        phi = (Ns > 1) ? add_rn(mul_rn((double)best, h), a.lo) : a.lo;
        if (tau0 != 0.0) {
            for (int j = tid; j < M; j += 256) X[j] = cmulc(d[j + 1], m[j + 1]);
            __syncthreads();
        }
    }
    // the nine sums in the fitted parameters at (ph, t), the same in every thread; false: not a point of the objective
    auto sums_at = [&](double ph, double t, double (&s)[9]) -> bool {
        const double tau = tau_of(t);
        fps_bsum<9, 1>(s, scratch, tid, [&](const int vt, double (&u)[9]) __attribute__((always_inline)) {
            nbs_part(X, p, M, ph, tau, vt, u);
        });
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 9; ++q) { s[q] *= ierr2; ok = ok && nbs_finite(s[q]); }
        if (lg) {
            const double t1 = PP_LN10 * tau, t2 = PP_LN10 * t1;
            s[4] = s[4] * t1 * t1 + s[3] * t2;
            s[8] = s[8] * t1 * t1 + s[7] * t2;
            s[3] *= t1; s[5] *= t1; s[7] *= t1;
        }
        return ok && s[6] > 0.0 && s[0] != 0.0;
    };
    // ---- solve: trust region with the exact 2 x 2 step; near the optimum (the predicted reduction below 1e-6 |f|,
    // the step an interior Newton step) the steps are taken as they come -- a comparison of f values resolves
    // nothing there -- until one is no shorter than the one before it: the rounding of the gradient.  (Not "much
    // shorter": on unscattered data without noise the minimum is degenerate along phi + tau = const, Newton's steps
    // shrink by 2/3 each, and the fit has to walk that down.)
    double s[9], st[9];
    int nfev = 1, rc = 1, polish = 0;
    double t = t_g;
    if (!sums_at(phi, t, s)) { give_up(nfev); return; }
    NbsEval e = nbs_fgh(s);
    // (the radius is a length in (phi, tau) whichever parameter is fitted -- a step in t = log10 tau counts as
    // ln10 tau dt, at most 100 dt -- and starts at half a step of the default grid: what the seed leaves open.  From a
    // larger one the first Newton step overshoots along the valley phi + tau = const into the one at negative tau.)
    double delta = 0.005, lastn = INFINITY;
    for (int it = 0; it < 2 * PP_NBS_MAXEV && nfev < PP_NBS_MAXEV; ++it) {
        double px, py, pred;
        bool interior;
        const double dsc = lg ? fmax(PP_LN10 * tau_of(t), 0.01) : 1.0;
        NbsEval es = e;
        es.g1 /= dsc; es.h01 /= dsc; es.h11 /= dsc * dsc;
        nbs_tr_step(es, delta, px, py, pred, interior);
        const double pn = hypot(px, py);
        py /= dsc;
        if (!(pred > 0.0) || !nbs_finite(pn)) { rc = (interior && pred == 0.0) ? 2 : 3; break; }
        const bool near = interior && pred <= 1e-6 * fabs(e.f);
        if (near && ((polish >= 1 && pn >= lastn) || pn <= 1e-16)) { rc = 2; break; }
        const double pht = phi + px, tt = t + py;
        const bool okt = in_box(tt) && sums_at(pht, tt, st);
        if (in_box(tt)) ++nfev;
        if (near && okt) {
            phi = pht; t = tt; e = nbs_fgh(st);
#pragma unroll
            for (int q = 0; q < 9; ++q) s[q] = st[q];
            lastn = pn;
            ++polish;
            continue;
        }
        double rho = -1.0;
        NbsEval et = e;
        if (okt) { et = nbs_fgh(st); rho = (e.f - et.f) / pred; }
        if (!(rho >= 0.25)) delta = 0.25 * pn;
        else if (rho > 0.75 && !interior) delta = fmin(2.0 * delta, 0.02);
        if (rho > 0.1) {
            phi = pht; t = tt; e = et;
#pragma unroll
            for (int q = 0; q < 9; ++q) s[q] = st[q];
        }
        if (delta < 1e-14) { rc = 2; break; }
    }
    if (rc == 3) { give_up(nfev); return; }
    // ---- post-fit: the Hessian with the amplitude in it, 3 x 3 (fit_portrait_full_function_2deriv_with_scales with
    // one channel): A_ij = -2 a (C_ij - a S_ij / 2), U_i = -2 (C_i - a S_i), the amplitude's own entry 2 S;
    // covariance of (phi, tau) = 2 (A - U U^T / 2S)^-1
    if (tid == 0) {
        const double C = s[0], S = s[6], sc = C / S;
        const double A00 = -2.0 * sc * s[2], A01 = -2.0 * sc * s[5], A11 = -2.0 * sc * (s[4] - 0.5 * sc * s[8]);
        const double U0 = -2.0 * s[1], U1 = -2.0 * (s[3] - sc * s[7]);
        const double i2S = 0.5 / S;
        const double X00 = A00 - U0 * U0 * i2S, X01 = A01 - U0 * U1 * i2S, X11 = A11 - U1 * U1 * i2S;
        const double det = X00 * X11 - X01 * X01;
        const double v00 = 2.0 * X11 / det, v01 = -2.0 * X01 / det, v11 = 2.0 * X00 / det;
        // U^T X^-1 U
        const double uxu = (U0 * U0 * X11 - 2.0 * U0 * U1 * X01 + U1 * U1 * X00) / det;
        const double var_a = 2.0 * (i2S + uxu * i2S * i2S);
        const double snr = sc * sqrt(S);
        double ph = phi;
        if (fabs(ph) >= 0.5) ph -= floor(ph);            // phi %= 1
        if (ph >= 0.5) ph -= 1.0;
        // A singular (phi, tau) block: X00 X11 and X01^2 agree to all the digits the nine sums carry (~1e-13 from sums of
        // up to 2048 terms), so a determinant below 1e-10 of the products is rounding, whatever its sign.  It happens
        // where it must: at tau = 0, d conj(B_k) / dtau = i w is the derivative of the phasor by phi / 2 pi, hence
        // C_phitau = C_phiphi, C_tautau = 2 C_phiphi, S_tautau = 2 C_phiphi / a and the block is K [[1, 1], [1, 1]]
        // exactly -- on unscattered data the fit cannot tell a scattering time from a delay.  The marginal errors
        // are infinite then; what is known is the phase at that tau: tau_err = inf, no covariance, and phi_err,
        // scale_err the errors at fixed tau (fit_phase_shift's).
        const bool pd = X00 > 0.0 && X11 > 0.0 && nbs_finite(X00) && nbs_finite(X11) && nbs_finite(X01);
        const bool singular = pd && !(det > 1e-10 * X00 * X11);
        const double phi_err = singular ? sqrt(2.0 / X00) : sqrt(v00), tau_err = singular ? INFINITY : sqrt(v11);
        const double scale_err = sqrt(singular ? 2.0 * i2S : var_a);
        const bool seen = snr >= PP_NBS_MINSNR && nbs_finite(scale_err);
        const bool good = pd && !singular && seen && nbs_finite(phi_err) && nbs_finite(tau_err) && (lg || t >= -3.0 * tau_err);
        const bool keep = good || (singular && seen);         // phi and tau are a point of the valley's floor
        o[0] = keep ? ph : NAN;
        o[1] = keep ? phi_err : NAN;
        o[2] = keep ? t : NAN;
        o[3] = keep ? tau_err : NAN;
        o[4] = sc;
        o[5] = scale_err;
        o[6] = snr;
        o[7] = (Sd + e.f) / (B - 3.0);
        o[8] = good ? v01 : NAN;
        o[9] = (double)nfev;
        o[10] = good ? (double)rc : 3.0;
    }
}

__global__ __launch_bounds__(256) void k_fps_scat(NbsArgs a) {
    __shared__ cplx Xs[PP_FPS_LDS];
    __shared__ double ps[PP_FPS_LDS];
    __shared__ double scratch[4 * 9];
    __shared__ double shv[4];
    __shared__ int shj[4];
    nbs_body(a, blockIdx.x, threadIdx.x, Xs, ps, scratch, shv, shj);
}

}  // namespace pp

// ---- host ------------------------------------------------------------------
static int fit_phase_tau_run(pp_ctx* c, const double* data, const double* model, const double* noise, const double* guess,
                             int nprof, int nbin, double lo, double hi, int Ns, int log10_tau, double* out) {
    const int M = nbin / 2;
    int rc;
    // interleave rows: data_i, model_i
    const size_t rowb = (size_t)nbin * 8;
    if ((rc = c->data.reserve(2 * (size_t)nprof * rowb))) return rc;
    HIP_TRY(hipMemcpy2DAsync(c->data.p, 2 * rowb, data, rowb, rowb, nprof, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync((char*)c->data.p + rowb, 2 * rowb, model, rowb, rowb, nprof, hipMemcpyHostToDevice, c->stream));
    if ((rc = c->X.reserve(2 * (size_t)nprof * (size_t)(M + 1) * sizeof(cplx)))) return rc;
    if ((rc = c->o_params.reserve((size_t)nprof * PP_NBS_NOUT * 8))) return rc;
    if ((rc = upload(c, c->x0, guess, (size_t)nprof * 16))) return rc;
    const double* dnoise = nullptr;
    if (noise) {
        if ((rc = upload(c, c->errs, noise, (size_t)nprof * 8))) return rc;
        dnoise = c->errs.as<double>();
    }
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;      // (a first use copies the table: not inside a timed span)
    cplx* spec = c->X.as<cplx>();
    {
        Prof pr(c, KF_NBSFFT);
        if ((rc = rows_harmonics(c, c->data.p, PP_F64, 2 * nprof, nbin, spec))) return rc;
    }
    {
        Prof pr(c, KF_NBSFIT);
        NbsArgs fa{spec, dnoise, c->x0.as<double>(), c->o_params.as<double>(), lo, hi, Ns, M, nprof, log10_tau ? 1 : 0};
        hipLaunchKernelGGL(k_fps_scat, dim3(nprof), dim3(256), 0, c->stream, fa);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->o_params.p, (size_t)nprof * PP_NBS_NOUT * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

extern "C" int pp_fit_phase_tau_batch(pp_ctx* c, const double* data, const double* model, const double* noise,
                                      const double* guess, int nprof, int nbin, double lo, double hi, int Ns,
                                      int log10_tau, double* out) {
    if (int busy_ = ctx_busy(c, "pp_fit_phase_tau_batch")) return busy_;
    if (!c || !data || !model || !guess || !out) return fail(PP_EINVAL, "pp_fit_phase_tau_batch: null argument");
    if (!nbin_any_ok(nbin) || nbin / 2 > PP_FPS_LDS) return nbin_refuse("pp_fit_phase_tau_batch", nbin);
    if (nprof < 1) return fail(PP_EINVAL, "pp_fit_phase_tau_batch: bad shape %d x %d", nprof, nbin);
    if (Ns < 1) return fail(PP_EINVAL, "pp_fit_phase_tau_batch: Ns %d", Ns);
    if (!(lo <= hi)) return fail(PP_EINVAL, "pp_fit_phase_tau_batch: bounds %g > %g", lo, hi);
    HIP_TRY(hipSetDevice(c->device));
    const int M = nbin / 2;
    return for_runs(nprof, aux_chunk_cap(c, 2.0 * nbin * 8 + 2.0 * (M + 1) * 16 + 128, nprof), [&](Run r) {
        return fit_phase_tau_run(c, r.at(data, nbin), r.at(model, nbin), r.at(noise, 1), r.at(guess, 2), r.n, nbin, lo, hi, Ns,
                                 log10_tau, r.at(out, PP_NBS_NOUT));
    });
}
