// Wavelet smoothing on the device (included at the end of pp_toas.hip, after pp_nbscat.h): the reference's
// wavelet_smooth (pplib.py:1621-1666), fit_wavelet_smooth_function (:1737-1761) and smart_smooth (:1668-1735) for
// the db8 wavelet, all in f64.
//
// The stationary wavelet transform with periodic boundary is, per level j, a pair of circular correlations of the
// running approximation with the low-pass filter h and its quadrature mirror g, dilated by s = 2^(j-1):
//     a_j[n] = sum_k h[k] a_{j-1}[n + s k],    d_j[n] = sum_k g[k] a_{j-1}[n + s k],    g[k] = (-1)^k h[15 - k].
// The inverse (the average of the even and odd decimated inverses) is the frame adjoint, level by level:
//     r_{j-1} = (H_j^T r_j + G_j^T T(d_j)) / 2,   r_L = T(a_L),   T the elementwise threshold.
// A circular shift of a level's coefficient arrays cancels between the two, so no alignment convention enters.
//
// The forward transform does not depend on the threshold factor: it runs ONCE per row to the deepest level tried
// (k_wl_forward), and leaves a_j, d_j of every level and the median of |a_j u d_j| (the threshold's scale at level j)
// in a scratch buffer.  Every evaluation of the objective -- the 30 grid points of every (row, level) in one launch
// (k_wl_grid), the simplex finishes (k_wl_simplex), the final smooth (k_wl_apply) -- is then one workgroup that
// thresholds the coarsest approximation into LDS, walks the levels down reading the thresholded details from the
// scratch buffer, transforms the smoothed row with the row transform of the fit (pp_fft.h; pp_anybin.h for lengths
// that are no power of two) and forms signal, tail noise and chi^2 by workgroup sums of a fixed order.  Nothing is
// accumulated atomically in floating point and no value of a row depends on another row: the same row gives the
// same bits in any batch.

namespace pp {

constexpr int WL_TAPS = 16;       // db8
constexpr int WL_NGRID = 30;      // scipy.optimize.brute's Ns in smart_smooth
constexpr int WL_MAXLEV = 12;     // log2(4096)
constexpr int WL_FT = 256;        // threads of the forward transform's workgroup

struct WlFilt { double h[WL_TAPS]; };     // low-pass taps, PyWavelets' rec_lo order (energy first)

// k-th smallest (0-based) of |v[0 .. n)|, exact: non-negative doubles order like their bit patterns, the pattern is
// fixed eight bits at a time from the top by a 256-bin count of the values that share the prefix found so far
__device__ inline double wl_select(const double* v, int n, unsigned k, unsigned* hist, unsigned long long* sh) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += WL_FT) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(v[i]));
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (cum + hist[b] > k) break;
                cum += hist[b];
            }
            sh[0] = prefix | ((unsigned long long)b << shift);
            sh[1] = (unsigned long long)(k - cum);
        }
        __syncthreads();
        prefix = sh[0];
        k = (unsigned)sh[1];
        __syncthreads();
    }
    return __longlong_as_double((long long)prefix);
}

// One workgroup per row: the row as f64, whether it holds anything but zeros, and for every level j = 1 .. nlev the
// coefficients coef[row][j - 1] = (a_j[nbin], d_j[nbin]) with med[row][j - 1] = numpy.median(|a_j u d_j|)
template <typename Tin>
__global__ __launch_bounds__(WL_FT) void k_wl_forward(const void* src, int nbin, int nlev, WlFilt f, double* x64,
                                                      double* coef, double* med, int* live) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh[2];
    const int row = blockIdx.x, tid = threadIdx.x;
    const Tin* x = reinterpret_cast<const Tin*>(src) + (size_t)row * nbin;
    double* xr = x64 + (size_t)row * nbin;
    int nz = 0;
    for (int n = tid; n < nbin; n += WL_FT) {
        const double v = (double)x[n];
        xr[n] = v;
        nz |= (v != 0.0) ? 1 : 0;
    }
    __threadfence_block();
    nz = __syncthreads_or(nz);
    if (tid == 0) live[row] = nz;
    double* cr = coef + (size_t)row * nlev * 2 * nbin;
    for (int j = 1; j <= nlev; ++j) {
        const double* prev = (j == 1) ? xr : cr + (size_t)(j - 2) * 2 * nbin;
        double* aj = cr + (size_t)(j - 1) * 2 * nbin;
        double* dj = aj + nbin;
        const int s = 1 << (j - 1);       // (2^nlev divides nbin: s <= nbin / 2)
        for (int n = tid; n < nbin; n += WL_FT) {
            double a = 0.0, d = 0.0;
            int idx = n;
#pragma unroll
            for (int k = 0; k < WL_TAPS; ++k) {
                const double v = prev[idx];
                a = fma(f.h[k], v, a);
                d = fma((k & 1) ? -f.h[WL_TAPS - 1 - k] : f.h[WL_TAPS - 1 - k], v, d);
                idx += s;
                if (idx >= nbin) idx -= nbin;
            }
            aj[n] = a;
            dj[n] = d;
        }
        __threadfence_block();
        __syncthreads();
        const double lo = wl_select(aj, 2 * nbin, (unsigned)(nbin - 1), hist, sh);
        const double hi = wl_select(aj, 2 * nbin, (unsigned)nbin, hist, sh);
        if (tid == 0) med[(size_t)row * nlev + j - 1] = 0.5 * (lo + hi);
    }
}

// get_noise_PS (pplib.py:2249-2253) of every row from its harmonics H[row][M + 1]
__global__ __launch_bounds__(256) void k_wl_rawnoise(const cplx* H, int nbin, double* noise) {
    __shared__ double red[4];
    const int row = blockIdx.x, tid = threadIdx.x, M = nbin / 2, kc = (int)(0.75 * (M + 1));
    const cplx* h = H + (size_t)row * (M + 1);
    double top[1] = {0.0};
    for (int k = kc + tid; k <= M; k += 256) top[0] += cnorm(h[k]);
    block_sum<1>(top, red);
    if (tid == 0) noise[row] = sqrt(top[0] / (double)nbin / (double)(M + 1 - kc));
}

struct WlArgs {
    const double* x64;        // [nrows][nbin]
    const double* coef;       // [nrows][nlev][2][nbin]
    const double* med;        // [nrows][nlev]
    const double* rawnoise;   // [nrows]
    const int* live;          // [nrows]
    double* srow;             // [workgroups][nbin]: the smoothed row of the evaluation in hand
    int nrows, nbin, nlev, soft;
    double c2ln;              // sqrt(2 ln nbin)
    double rchi2_tol;
    WlFilt f;
    AnyArgs g;                // twB (every length); chirp, bft, twL (lengths that are no power of two)
    int ntry;                 // levels smart_smooth tries: 1 .. ntry (<= nlev)
    double* fgrid;            // [nrows][ntry][WL_NGRID]
    double* lev_fact;         // [nrows][ntry]  the simplex's best factor,
    double* lev_fun;          // ... its value
    int* lev_nfev;            // ... and the evaluations spent (grid included)
    const int* nlevel_row;    // plain smoothing: [nrows] level and
    const double* fact_row;   // ... factor
    double* out;              // [nrows][nbin]
    double* info;             // smart: [nrows][5] level, fact, -fun, reduced chi^2 of the final smooth, nfev
};

// the transform of the row length: a tuned plan of M = nbin / 2 points, or the chirp-z route through L points
template <int M_>
struct WlPow2 {
    static constexpr bool ANY = false;
    static constexpr int L = M_, T = FftPlan<M_>::T, NMAX = 2 * M_, LDS0 = FftPlan<M_>::LDS_ELEMS, LDS1 = 1;
};
template <int L_>
struct WlAny {
    static constexpr bool ANY = true;
    static constexpr int L = L_, T = FftPlan<L_>::T, NMAX = L_, LDS0 = FftPlan<L_>::LDS_ELEMS, LDS1 = L_;
};

struct WlWork {
    cplx* lds;       // the transform's work array
    cplx* buf;       // chirp-z: the packed row (unused by the tuned plans)
    double* r;       // the running approximation, nbin values: the same LDS as buf (chirp-z) or lds (tuned plans)
    double* red;     // workgroup sums
    double* srow;
    int tid;
};

// wavelet_smooth of one row at (lev, fact) from the stored coefficients: the result in w.r and in w.srow
template <class F>
__device__ __forceinline__ void wl_smooth_row(const WlArgs& a, const WlWork& w, int row, int lev, double fact) {
    constexpr int T = F::T, PER = (F::NMAX + T - 1) / T;
    const int nbin = a.nbin, tid = w.tid, soft = a.soft;
    const double* cr = a.coef + (size_t)row * a.nlev * 2 * nbin;
    const double lopt = (fact * (a.med[(size_t)row * a.nlev + lev - 1] / 0.6745)) * a.c2ln;
    // pywt.threshold: hard -- 0 where |c| < lopt; soft -- c max(1 - lopt / |c|, 0), a NaN (0 / 0) kept as numpy's clip keeps it
    auto thr = [&](double c) __attribute__((always_inline)) {
        if (soft) {
            double t = 1.0 - lopt / fabs(c);
            t = (t < 0.0) ? 0.0 : t;
            return c * t;
        }
        return (fabs(c) < lopt) ? 0.0 : c;
    };
    const double* aL = cr + (size_t)(lev - 1) * 2 * nbin;
    for (int n = tid; n < nbin; n += T) w.r[n] = thr(aL[n]);
    __syncthreads();
    for (int j = lev; j >= 1; --j) {
        const double* dj = cr + (size_t)(j - 1) * 2 * nbin + nbin;
        const int s = 1 << (j - 1);
        double reg[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int m = tid + i * T;
            double acc = 0.0;
            if (m < nbin) {
                int idx = m;
#pragma unroll
                for (int k = 0; k < WL_TAPS; ++k) {
                    acc = fma(a.f.h[k], w.r[idx], acc);
                    acc = fma((k & 1) ? -a.f.h[WL_TAPS - 1 - k] : a.f.h[WL_TAPS - 1 - k], thr(dj[idx]), acc);
                    idx -= s;
                    if (idx < 0) idx += nbin;
                }
            }
            reg[i] = 0.5 * acc;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int m = tid + i * T;
            if (m < nbin) w.r[m] = reg[i];
        }
        __syncthreads();
    }
    for (int n = tid; n < nbin; n += T) w.srow[n] = w.r[n];
    __threadfence_block();
    __syncthreads();
}

// this thread's share of sum_{k >= 1} |rfft(srow)_k|^2 and of its top quarter (get_noise_PS's harmonics)
template <class F>
__device__ __forceinline__ void wl_power(const WlArgs& a, const WlWork& w, double& pw, double& top) {
    constexpr int T = F::T, L = F::L;
    const int M = a.nbin / 2, kc = (int)(0.75 * (M + 1)), tid = w.tid;
    pw = top = 0.0;
    if constexpr (F::ANY) {
        // (w.r IS w.buf: the row's M packed pairs are in place)
        czt_any<L>(w.buf, w.lds, a.g, tid);
        const cplx z0 = w.buf[0];
        for (int k = 1 + tid; k <= M; k += T) {
            cplx d;
            if (k == M) d = make_double2(z0.x - z0.y, 0.0);
            else {
                const cplx zk = w.buf[k];
                cplx zc = w.buf[M - k];
                zc.y = -zc.y;
                const cplx E = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
                const cplx O = make_double2(0.5 * (zk.x - zc.x), 0.5 * (zk.y - zc.y));
                const cplx wo = cmul(a.g.twB[k], O);
                d = make_double2(E.x + wo.y, E.y - wo.x);
            }
            const double p = cnorm(d);
            pw += p;
            if (k >= kc) top += p;
        }
    } else {
        fft_row<L, double>(w.lds, w.srow, a.g.twB, tid);
        __syncthreads();
        for (int k = 1 + tid; k <= M; k += T) {
            const double p = cnorm(rfft_harmonic<L>(w.lds, a.g.twB, k));
            pw += p;
            if (k >= kc) top += p;
        }
    }
    __syncthreads();
}

// fit_wavelet_smooth_function (pplib.py:1737-1761) of row `row` at (lev, fact), the same value in every thread;
// leaves the smoothed row in w.srow.  st[0] = reduced chi^2 against the row, st[1] = sum_{k >= 1} |rfft|^2.
template <class F>
__device__ __noinline__ double wl_objective(const WlArgs& a, const WlWork& w, int row, int lev, double fact, double* st) {
    constexpr int T = F::T;
    const int nbin = a.nbin, M = nbin / 2, kc = (int)(0.75 * (M + 1)), tid = w.tid;
    wl_smooth_row<F>(a, w, row, lev, fact);
    double v[3];
    wl_power<F>(a, w, v[0], v[1]);
    const double* x = a.x64 + (size_t)row * nbin;
    const double sg = a.rawnoise[row];
    v[2] = 0.0;
    for (int n = tid; n < nbin; n += T) {
        const double t = (x[n] - w.srow[n]) / sg;
        v[2] += t * t;
    }
    block_sum<3>(v, w.red);
    __syncthreads();
    double snr = 0.0;
    if (v[0] != 0.0) {
        const double noise = sqrt(v[1] / (double)nbin / (double)(M + 1 - kc)) * sqrt((double)nbin / 2.0);
        snr = (noise != 0.0) ? v[0] / noise : INFINITY;
    }
    const double rc = v[2] / (double)nbin;
    if (fabs(rc - 1.0) > a.rchi2_tol) snr = 0.0;
    st[0] = rc;
    st[1] = v[0];
    return -snr;
}

#define PP_WL_SHARED(F)                                                                         \
    __shared__ cplx lds_[F::LDS0];                                                              \
    __shared__ cplx buf_[F::LDS1];                                                              \
    __shared__ double red_[3 * (F::T / 64)];                                                    \
    const int tid = threadIdx.x;                                                                \
    const WlWork w{lds_, buf_, reinterpret_cast<double*>(F::ANY ? buf_ : lds_), red_,           \
                   a.srow + (size_t)blockIdx.x * a.nbin, tid}

// grid point j of brute's range (0, 3): numpy.mgrid's arithmetic, arange(Ns) * step + start
__device__ __forceinline__ double wl_grid_point(int j) { return add_rn(mul_rn((double)j, 3.0 / (double)(WL_NGRID - 1)), 0.0); }

// stage 1: every grid point of every level of every row, one workgroup each
template <class F>
__global__ __launch_bounds__(F::T) void k_wl_grid(WlArgs a) {
    PP_WL_SHARED(F);
    const long long total = (long long)a.nrows * a.ntry * WL_NGRID;
    for (long long it = blockIdx.x; it < total; it += gridDim.x) {
        const int j = (int)(it % WL_NGRID), lev = (int)((it / WL_NGRID) % a.ntry) + 1, row = (int)(it / ((long long)WL_NGRID * a.ntry));
        if (!a.live[row]) continue;
        double st[2];
        const double v = wl_objective<F>(a, w, row, lev, wl_grid_point(j), st);
        if (tid == 0) a.fgrid[it] = v;
    }
}

// stage 2: brute's finish of every (row, level): scipy's fmin from the best grid point (the first of equal values)
template <class F>
__global__ __launch_bounds__(F::T) void k_wl_simplex(WlArgs a) {
    PP_WL_SHARED(F);
    const long long total = (long long)a.nrows * a.ntry;
    for (long long it = blockIdx.x; it < total; it += gridDim.x) {
        const int lev = (int)(it % a.ntry) + 1, row = (int)(it / a.ntry);
        if (!a.live[row]) continue;
        const double* fg = a.fgrid + (size_t)it * WL_NGRID;
        int best = 0;
        for (int j = 1; j < WL_NGRID; ++j)
            if (fg[j] < fg[best]) best = j;
        double f0, st[2];
        int fcalls;
        const double xm = nelder_mead_1d(wl_grid_point(best), [&](double x) { return wl_objective<F>(a, w, row, lev, x, st); }, f0, fcalls);
        if (tid == 0) {
            a.lev_fact[it] = xm;
            a.lev_fun[it] = f0;
            a.lev_nfev[it] = WL_NGRID + fcalls;
        }
    }
}

// stage 3 (smart = 1): the level of the smallest value (the first of equal ones), the final smooth, zeroed when its own
// reduced chi^2 is further than rchi2_tol from 1; an all-zero row stays zero.  smart = 0: wavelet_smooth at the
// caller's level and factor.
template <class F>
__global__ __launch_bounds__(F::T) void k_wl_apply(WlArgs a, int smart) {
    PP_WL_SHARED(F);
    constexpr int T = F::T;
    for (int row = blockIdx.x; row < a.nrows; row += gridDim.x) {
        double* out = a.out + (size_t)row * a.nbin;
        int lev, nfev = 0;
        double fact, fun = 0.0;
        if (smart) {
            if (!a.live[row]) {
                for (int n = tid; n < a.nbin; n += T) out[n] = 0.0;
                if (tid < 5) a.info[(size_t)row * 5 + tid] = 0.0;
                continue;
            }
            const size_t b = (size_t)row * a.ntry;
            int il = 0;
            for (int l = 0; l < a.ntry; ++l) {
                if (a.lev_fun[b + l] < a.lev_fun[b + il]) il = l;
                nfev += a.lev_nfev[b + l];
            }
            lev = il + 1;
            fact = a.lev_fact[b + il];
            fun = a.lev_fun[b + il];
        } else {
            lev = a.nlevel_row[row];
            fact = a.fact_row[row];
        }
        double st[2];
        (void)wl_objective<F>(a, w, row, lev, fact, st);
        const bool zero = smart && fabs(st[0] - 1.0) > a.rchi2_tol;
        for (int n = tid; n < a.nbin; n += T) out[n] = zero ? 0.0 : w.srow[n];
        if (smart && tid == 0) {
            double* o = a.info + (size_t)row * 5;
            o[0] = (double)lev; o[1] = fact; o[2] = -fun; o[3] = st[0]; o[4] = (double)nfev;
        }
        __syncthreads();
    }
}

}  // namespace pp

// ---- host side ---------------------------------------------------------------------------------------------
// the taps must be an orthonormal low-pass filter: sum h = sqrt 2, sum_k h[k] h[k + 2 m] = delta_m
static int wl_check_filter(const char* who, const double* h) {
    double s = 0.0;
    for (int k = 0; k < WL_TAPS; ++k) s += h[k];
    if (!(std::fabs(s - std::sqrt(2.0)) < 1e-12)) return fail(PP_EINVAL, "%s: the filter's taps sum to %.17g, not sqrt 2", who, s);
    for (int m = 0; m < WL_TAPS / 2; ++m) {
        double d = 0.0;
        for (int k = 0; k + 2 * m < WL_TAPS; ++k) d += h[k] * h[k + 2 * m];
        if (!(std::fabs(d - (m == 0 ? 1.0 : 0.0)) < 1e-12)) return fail(PP_EINVAL, "%s: the filter is not orthonormal (shift %d: %.3g)", who, 2 * m, d);
    }
    return PP_OK;
}

// f(policy): the transform of the row length as the compile-time type the kernels want
template <typename Fn>
static int wl_with_plan(pp_ctx* c, int nbin, AnyArgs* g, Fn f) {
    if (nbin_ok(nbin)) {
        const cplx* tw = nullptr;
        if (int rc = get_twiddles(c, nbin, &tw)) return rc;
        memset(g, 0, sizeof *g);
        g->nbin = nbin; g->M = nbin / 2; g->twB = tw;
        switch (nbin / 2) {
            case 16: f(WlPow2<16>{}); break;
            case 32: f(WlPow2<32>{}); break;
            case 64: f(WlPow2<64>{}); break;
            case 128: f(WlPow2<128>{}); break;
            case 256: f(WlPow2<256>{}); break;
            case 512: f(WlPow2<512>{}); break;
            case 1024: f(WlPow2<1024>{}); break;
            case 2048: f(WlPow2<2048>{}); break;
            default: return fail(PP_EINVAL, "wavelet smoothing: nbin %d", nbin);
        }
        return PP_OK;
    }
    int L = 0;
    if (int rc = any_args(c, nbin, g, &L)) return rc;
    return with_any_len(L, [&](auto LL) { f(WlAny<decltype(LL)::value>{}); });
}

// One run of rows: forward transforms, then either the plain smooth (smart = 0) or the three stages of smart_smooth.
// nlevel / fact: per row (smart = 0).  stats: k_pca_stats of the smoothed rows (smart = 1).
static int wl_run(pp_ctx* c, const void* rows, int dtype, int on_device, int nrows, int nbin, const double* filt, int soft,
                  int smart, int ntry, double rchi2_tol, const int32_t* nlevel, const double* fact, int nlev, double* out,
                  double* info, double* stats, double* raw_noise) {
    pp_ctx::Wl& W = c->wl;
    const int M = nbin / 2;
    const size_t rowb = (size_t)nbin * 8, esz = dtype == PP_F64 ? 8 : 4;
    int rc;
    const void* dsrc = rows;
    if (!on_device) {
        if ((rc = upload(c, c->data, rows, (size_t)nrows * nbin * esz))) return rc;
        dsrc = c->data.p;
    }
    // at most 2048 workgroups walk the evaluations: one scratch row each
    const long long nwork = smart ? (long long)nrows * ntry * WL_NGRID : nrows;
    const int grid = (int)std::max(1LL, std::min(nwork, 2048LL));
    if ((rc = W.x64.reserve((size_t)nrows * rowb))) return rc;
    if ((rc = W.coef.reserve((size_t)nrows * nlev * 2 * rowb))) return rc;
    if ((rc = W.med.reserve((size_t)nrows * nlev * 8))) return rc;
    if ((rc = W.noise.reserve((size_t)nrows * 8))) return rc;
    if ((rc = W.live.reserve((size_t)nrows * 4))) return rc;
    if ((rc = W.srow.reserve((size_t)grid * rowb))) return rc;
    if ((rc = W.out.reserve((size_t)nrows * rowb))) return rc;
    if ((rc = W.small.reserve((size_t)nrows * (5 + 4) * 8))) return rc;
    if ((rc = c->X.reserve((size_t)nrows * (M + 1) * sizeof(cplx)))) return rc;
    WlFilt f;
    std::copy(filt, filt + WL_TAPS, f.h);
    with_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL((k_wl_forward<decltype(t)>), dim3(nrows), dim3(WL_FT), 0, c->stream, dsrc, nbin, nlev, f,
                           W.x64.as<double>(), W.coef.as<double>(), W.med.as<double>(), W.live.as<int>());
    });
    HIP_TRY(hipGetLastError());
    if ((rc = rows_harmonics(c, W.x64.p, PP_F64, nrows, nbin, c->X.as<cplx>()))) return rc;
    hipLaunchKernelGGL(k_wl_rawnoise, dim3(nrows), dim3(256), 0, c->stream, (const cplx*)c->X.as<cplx>(), nbin, W.noise.as<double>());
    HIP_TRY(hipGetLastError());
    WlArgs a;
    memset(&a, 0, sizeof a);
    a.x64 = W.x64.as<double>(); a.coef = W.coef.as<double>(); a.med = W.med.as<double>(); a.rawnoise = W.noise.as<double>();
    a.live = W.live.as<int>(); a.srow = W.srow.as<double>();
    a.nrows = nrows; a.nbin = nbin; a.nlev = nlev; a.soft = soft;
    a.c2ln = std::sqrt(2.0 * std::log((double)nbin));
    a.rchi2_tol = rchi2_tol;
    a.f = f;
    a.ntry = ntry;
    a.out = W.out.as<double>();
    a.info = W.small.as<double>();
    double* dstats = a.info + (size_t)nrows * 5;
    if (smart) {
        const size_t nl = (size_t)nrows * ntry;
        if ((rc = W.fgrid.reserve(nl * WL_NGRID * 8))) return rc;
        if ((rc = W.lev.reserve(nl * (8 + 8 + 4)))) return rc;
        a.fgrid = W.fgrid.as<double>();
        a.lev_fact = W.lev.as<double>();
        a.lev_fun = a.lev_fact + nl;
        a.lev_nfev = reinterpret_cast<int*>(a.lev_fun + nl);
    } else {
        if ((rc = upload(c, W.par, fact, (size_t)nrows * 8))) return rc;
        if ((rc = upload(c, W.idx, nlevel, (size_t)nrows * 4))) return rc;
        a.fact_row = W.par.as<double>();
        a.nlevel_row = W.idx.as<int>();
    }
    const int grid_lev = (int)std::max(1LL, std::min((long long)nrows * ntry, (long long)grid));
    const int grid_row = std::min(nrows, grid);
    if ((rc = wl_with_plan(c, nbin, &a.g, [&](auto F) {
            using P = decltype(F);
            if (smart) {
                hipLaunchKernelGGL((k_wl_grid<P>), dim3(grid), dim3(P::T), 0, c->stream, a);
                hipLaunchKernelGGL((k_wl_simplex<P>), dim3(grid_lev), dim3(P::T), 0, c->stream, a);
            }
            hipLaunchKernelGGL((k_wl_apply<P>), dim3(grid_row), dim3(P::T), 0, c->stream, a, smart);
        })))
        return rc;
    HIP_TRY(hipGetLastError());
    if (smart) {
        // the statistics find_significant_eigvec takes of the smoothed rows, by ppspline's own kernel
        if ((rc = rows_harmonics(c, W.out.p, PP_F64, nrows, nbin, c->X.as<cplx>()))) return rc;
        hipLaunchKernelGGL(k_pca_stats, dim3(nrows), dim3(PCA_ST), 0, c->stream, (const double*)W.out.as<double>(),
                           (const cplx*)c->X.as<cplx>(), nbin, dstats);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(info, a.info, (size_t)nrows * 5 * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(stats, dstats, (size_t)nrows * 4 * 8, hipMemcpyDeviceToHost, c->stream));
        if (raw_noise) HIP_TRY(hipMemcpyAsync(raw_noise, W.noise.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(out, W.out.p, (size_t)nrows * rowb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

// what both entry points check of their rows
static int wl_validate(const char* who, pp_ctx* c, const void* rows, int dtype, int nrows, int nbin, const double* filt,
                       int threshtype, const void* out) {
    if (!c || !rows || !filt || !out) return fail(PP_EINVAL, "%s: null argument", who);
    if (nbin < 16 || nbin > 4096 || nbin % 2) return fail(PP_EINVAL, "%s: nbin %d must be even and in [16, 4096]", who, nbin);
    if (nrows < 1) return fail(PP_EINVAL, "%s: %d rows", who, nrows);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "%s: dtype %d", who, dtype);
    if (threshtype != 0 && threshtype != 1) return fail(PP_EINVAL, "%s: threshtype %d (0 hard, 1 soft)", who, threshtype);
    return wl_check_filter(who, filt);
}

// device bytes per row of a run: the f64 copy, the coefficients, the output, harmonics, and the small arrays
static double wl_row_bytes(int nbin, int nlev, int ntry, size_t esz) {
    return (double)nbin * (esz + 8.0 * (2 + 2 * nlev) + 8.0) + 64.0 + (double)ntry * (WL_NGRID + 3) * 8.0;
}

extern "C" int pp_wavelet_smooth(pp_ctx* c, const void* rows, int dtype, int on_device, int nrows, int nbin,
                                 const double* filt, int threshtype, const int32_t* nlevel, int64_t nlevel_stride,
                                 const double* fact, int64_t fact_stride, void* out) {
    if (int busy_ = ctx_busy(c, "pp_wavelet_smooth")) return busy_;
    if (int rc = wl_validate("pp_wavelet_smooth", c, rows, dtype, nrows, nbin, filt, threshtype, out)) return rc;
    if (!nlevel || !fact) return fail(PP_EINVAL, "pp_wavelet_smooth: null argument");
    if ((nlevel_stride != 0 && nlevel_stride != 1) || (fact_stride != 0 && fact_stride != 1))
        return fail(PP_EINVAL, "pp_wavelet_smooth: strides must be 0 (one value) or 1 (one per row)");
    std::vector<int32_t> lv((size_t)nrows);
    std::vector<double> fc((size_t)nrows);
    int nlev = 0;
    for (int i = 0; i < nrows; ++i) {
        lv[i] = nlevel[(size_t)i * nlevel_stride];
        fc[i] = fact[(size_t)i * fact_stride];
        if (lv[i] < 1 || lv[i] > WL_MAXLEV || nbin % (1 << lv[i]))
            return fail(PP_EINVAL, "pp_wavelet_smooth: %d levels of %d bins (2^levels must divide nbin)", (int)lv[i], nbin);
        nlev = std::max(nlev, (int)lv[i]);
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t esz = dtype == PP_F64 ? 8 : 4;
    const int cap = aux_chunk_cap(c, wl_row_bytes(nbin, nlev, 0, esz), nrows);
    return for_runs(nrows, cap, [&](Run r) {
        return wl_run(c, r.at((const char*)rows, (size_t)nbin * esz), dtype, on_device, r.n, nbin, filt, threshtype, 0, 0, 0.0,
                      r.at(lv.data(), 1), r.at(fc.data(), 1), nlev, (double*)r.at((char*)out, (size_t)nbin * 8), nullptr, nullptr, nullptr);
    });
}

extern "C" int pp_smart_smooth(pp_ctx* c, const void* rows, int dtype, int on_device, int nrows, int nbin,
                               const double* filt, int threshtype, int try_nlevels, double rchi2_tol, void* out,
                               double* info5, double* stats4, double* raw_noise) {
    if (int busy_ = ctx_busy(c, "pp_smart_smooth")) return busy_;
    if (int rc = wl_validate("pp_smart_smooth", c, rows, dtype, nrows, nbin, filt, threshtype, out)) return rc;
    if (!info5 || !stats4) return fail(PP_EINVAL, "pp_smart_smooth: null argument");
    if (try_nlevels < 1 || try_nlevels > WL_MAXLEV || nbin % (1 << try_nlevels))
        return fail(PP_EINVAL, "pp_smart_smooth: %d levels of %d bins (2^levels must divide nbin)", try_nlevels, nbin);
    if (!(rchi2_tol >= 0.0)) return fail(PP_EINVAL, "pp_smart_smooth: rchi2_tol %g", rchi2_tol);
    HIP_TRY(hipSetDevice(c->device));
    const size_t esz = dtype == PP_F64 ? 8 : 4;
    const int cap = aux_chunk_cap(c, wl_row_bytes(nbin, try_nlevels, try_nlevels, esz), nrows);
    return for_runs(nrows, cap, [&](Run r) {
        return wl_run(c, r.at((const char*)rows, (size_t)nbin * esz), dtype, on_device, r.n, nbin, filt, threshtype, 1, try_nlevels,
                      rchi2_tol, nullptr, nullptr, try_nlevels, (double*)r.at((char*)out, (size_t)nbin * 8), r.at(info5, 5),
                      r.at(stats4, 4), r.at(raw_noise, 1));
    });
}
