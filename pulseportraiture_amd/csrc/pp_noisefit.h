// The 'fit' noise method on the device (included at the end of pp_toas.hip, after pp_zap.h): pplib.find_kc
// (pplib.py:1465-1495) and get_noise_fit (pplib.py:2255-2287) of every row.  find_kc fits b f_a(k) + dc to the
// log10 power spectrum with opt.brute over a 20 x 20 x 20 grid (a, b, dc); f_a(k) = exp(-a k) ('exp_dc') or the
// half triangle 1 - k / floor(a) below floor(a) ('half_tri').  The search is separable: with d'_k = data_k -
// min(data), b = ib R / 19 and dc' = idc R / 19 (R = max - min),
//     chi^2(a, b, dc) = [S_dd - 2 dc' S_d + H dc'^2] + b [b S_ff(a) + 2 dc' S_f(a) - 2 S_df(a)],
// so one pass over the row forms S_d, S_dd and the 20 S_df(a), and the 8000 cells cost a handful of operations
// each.  S_f, S_ff, the 20 cut-offs kc(a) and the table f_a(k) depend on (H, fn) only: the host builds them once
// per row length (noise_fit_table) and the kernels read the table through L2, each a's sum cut at the harmonic
// klim(a) where f_a(k) drops below 2^-70 (exp_dc) or is zero (half_tri).
//
// The two rules the reference's argmin implies are kept bit for bit:
//   - a cell with b = 0 gets the bracket [..] alone (0 times a finite number), the same bits for every a: all 20
//     a tie and the lowest flat index (a slowest, dc fastest) wins, as NumPy's argmin over the raveled grid;
//   - a harmonic of zero power makes log10 -inf and the reference's whole grid NaN: argmin gives cell 0, whose
//     a = 1 / H never passes the 0.005 test, so kc = H - 1 (any non-finite log power takes this way).
// Every sum is taken in an order fixed by the row length alone: a row's bits depend on nothing else in the call.

namespace pp {

constexpr int PP_NF_NS = 20;                 // opt.brute's Ns
constexpr int PP_NF_CELLS = PP_NF_NS * PP_NF_NS * PP_NF_NS;
constexpr int PP_NF_MAXH = 2049;             // nbin <= 4096
constexpr int PP_NF_T = 256;                 // lanes of the harmonics twin and of the power-spectrum entry
constexpr int PP_NF_HEAD = 4 * PP_NF_NS;     // S_f, S_ff, klim, kc of the 20 a in front of the table f_a(k)
constexpr int PP_NF_NSUM = PP_NF_NS + 2;     // the 20 S_df(a), S_d, S_dd

struct NoiseFitArgs {
    ChanNoiseArgs cn;         // rows, norms and outputs as pp_channel_noise has them (cn.M = H - 1 for power spectra)
    const double* pows;       // [nrows][H] rows that already are power spectra, or nullptr
    const double* tab;        // noise_fit_table of (H, fn)
    double fact;              // get_noise_fit's factor on kc
    int* kc;                  // [nrows]
    int* cell;                // [nrows][3] (ia, ib, idc)
};

template <int T>
struct NoiseFitShared {
    double red[(T / 64) * PP_NF_NSUM];
    double sdf[PP_NF_NS];
    int wf[T / 64];           // the waves' winning flat cells
};

// workgroup totals (sums, or maxima) of the lanes' w[0 .. N), on every lane, in an order the lane count fixes
template <int T, int N, bool MAX>
__device__ __forceinline__ void nf_block(double* red, double (&w)[N]) {
    constexpr int NW = T / 64;
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < N; ++q) w[q] = MAX ? group_max<64>(w[q]) : group_sum<64>(w[q]);
    if (NW > 1) {
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < N; ++q) red[(tid >> 6) * N + q] = w[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < N; ++q) {
            double t = red[q];
            for (int u = 1; u < NW; ++u) t = MAX ? fmax(t, red[u * N + q]) : t + red[u * N + q];
            w[q] = t;
        }
        __syncthreads();
    }
}

// find_kc and get_noise_fit of the row whose log10 powers are d[0 .. H): lane tid has written the entries
// k = tid, tid + T, ... and reads no others before the first workgroup sum.  v: the row's moments (chan_noise_reduce);
// pow_at(k) * pscale is the power of harmonic k again, for the tail's mean.
template <int T, typename PowAt>
__device__ __forceinline__ void noisefit_row(const NoiseFitArgs& a, long long r, int H, double* d, NoiseFitShared<T>& sh,
                                             const double v[5], double pscale, PowAt pow_at) {
    constexpr int NS = PP_NF_NS;
    const int tid = threadIdx.x;
    const double* hd = a.tab;
    // min and max of the data; anything not finite sends the row to cell 0
    double w[3] = {-INFINITY, -INFINITY, 0.0};
    for (int k = tid; k < H; k += T) {
        const double x = d[k];
        w[0] = fmax(w[0], -x);
        w[1] = fmax(w[1], x);
        if (!(fabs(x) < INFINITY)) w[2] = 1.0;
    }
    nf_block<T, 3, true>(sh.red, w);
    int flat = 0;
    if (w[2] == 0.0) {          // (uniform over the workgroup)
        const double mn = -w[0], step = (w[1] - mn) / (double)(NS - 1);
        double s[PP_NF_NSUM];
        double sd = 0.0, sdd = 0.0;
        for (int k = tid; k < H; k += T) {
            const double x = d[k] - mn;
            d[k] = x;
            sd += x;
            sdd = fma(x, x, sdd);
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int kl = (int)hd[2 * NS + q];
            const double* f = hd + PP_NF_HEAD + (size_t)q * H;
            double acc = 0.0;
            for (int k = tid; k < kl; k += T) acc = fma(d[k], f[k], acc);
            s[q] = acc;
        }
        s[NS] = sd; s[NS + 1] = sdd;
        nf_block<T, PP_NF_NSUM, false>(sh.red, s);
        sd = s[NS]; sdd = s[NS + 1];
        // the 8000 cells, flat index = (ia 20 + ib) 20 + idc.  A lane owns the (ib, idc) pairs c = tid, tid + T, ... of
        // every a: b, dc' and the bracket are formed once, and each a adds its three sums (uniform: scalar loads
        // and one LDS word).  a ascends outside, c inside: the lane meets its cells in flat order and
        // keeps its first minimum; then the workgroup's
        constexpr int NJ = (NS * NS + T - 1) / T;
        double cb[NJ], cdc[NJ], cbase[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = tid + T * j;
            cb[j] = (double)(c / NS) * step;
            cdc[j] = (double)(c % NS) * step;
            cbase[j] = sdd - 2.0 * cdc[j] * sd + (double)H * cdc[j] * cdc[j];
        }
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < NS; ++q) sh.sdf[q] = s[q];
        }
        __syncthreads();
        double best = INFINITY;
        int bf = PP_NF_CELLS;
#pragma unroll 1
        for (int q = 0; q < NS; ++q) {          // (not unrolled: 20 copies of the cells cost 140 registers more)
            const double sf = hd[q], sff = hd[NS + q], sdf = sh.sdf[q];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const double chi = cbase[j] + cb[j] * (cb[j] * sff + 2.0 * cdc[j] * sf - 2.0 * sdf);
                if ((NS * NS) % T == 0 || tid + T * j < NS * NS) {
                    if (chi < best) { best = chi; bf = q * NS * NS + tid + T * j; }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int of = __shfl_xor(bf, o, 64);
            if (ob < best || (ob == best && of < bf)) { best = ob; bf = of; }
        }
        if (T > 64) {
            if ((tid & 63) == 0) { sh.red[tid >> 6] = best; sh.wf[tid >> 6] = bf; }
            __syncthreads();
            best = sh.red[0]; bf = sh.wf[0];
            for (int u = 1; u < T / 64; ++u) {
                const double ob = sh.red[u];
                const int of = sh.wf[u];
                if (ob < best || (ob == best && of < bf)) { best = ob; bf = of; }
            }
            __syncthreads();
        }
        flat = bf < PP_NF_CELLS ? bf : 0;       // (no cell below +inf: argmin's cell 0)
    }
    // kc of the winning a; get_noise_fit (pplib.py:2273-2277): k = fact kc, clipped to int(0.99 H) from H on
    const int ia = flat / (NS * NS);
    const int kcv = (int)hd[3 * NS + ia];
    double kk = a.fact * (double)kcv;
    if (kk >= (double)H) kk = fmin((double)(int)(0.99 * (double)H), kk);
    const int start = (int)kk;
    double tl[1] = {0.0};
    for (int k = start + tid; k < H; k += T) tl[0] += pow_at(k);
    nf_block<T, 1, false>(sh.red, tl);
    if (tid == 0) {
        chan_noise_finish(a.cn, r, v, sqrt(tl[0] / pscale / (double)(H - start)));
        if (a.kc) a.kc[r] = kcv;
        if (a.cell) {
            a.cell[3 * r] = ia;
            a.cell[3 * r + 1] = (flat / NS) % NS;
            a.cell[3 * r + 2] = flat % NS;
        }
    }
}

// one workgroup per row, as k_chan_noise: the row is read once into the transform's first stage, its moments are
// taken there, and the log10 powers of its H harmonics go to LDS beside the transform's image, which stays for the
// tail's mean; nothing but the row's scalars is written
template <int M, typename Tin>
__global__ __launch_bounds__(FftPlan<M>::T) void k_noisefit(NoiseFitArgs a) {
    constexpr int T = FftPlan<M>::T, R1 = FftPlan<M>::R1, PER1 = FftPlan<M>::PER1;
    constexpr int NBF = StageGeom<M, T, R1>::NBF;
    typedef typename RawOf<Tin>::type Raw;
    __shared__ cplx lds[FftPlan<M>::LDS_ELEMS];
    __shared__ double d[M + 1];
    __shared__ NoiseFitShared<T> sh;
    const int tid = threadIdx.x;
    for (long long r = blockIdx.x; r < a.cn.nrows; r += gridDim.x) {
        const Tin* grow = reinterpret_cast<const Tin*>(a.cn.src) + (size_t)r * (2 * M);
        Raw raw[PER1][R1];
        stage_load_global<M, T, R1>(raw, grow, tid);
        RowTwiddles<M> tw;
        load_row_twiddles<M>(tw, a.cn.twB, tid);
        double v[5];
        chan_noise_start(v);
        cplx z[PER1][R1];
#pragma unroll
        for (int i = 0; i < PER1; ++i)
#pragma unroll
            for (int k = 0; k < R1; ++k) {
                z[i][k] = to_cplx(raw[i][k]);
                if (NBF % T == 0 || tid + T * i < NBF) {          // (the lanes stage_load_global loaded)
                    chan_noise_sample(v, z[i][k].x);
                    chan_noise_sample(v, z[i][k].y);
                }
            }
        fft_first_stage<M>(lds, z, tw, tid);
        fft_later_stages<M>(lds, tw, tid);
        for (int k = tid; k <= M; k += T) d[k] = log10(cnorm(rfft_harmonic<M>(lds, a.cn.twB, k)) / (double)(2 * M));
        chan_noise_reduce<T>(sh.red, v);
        noisefit_row<T>(a, r, M + 1, d, sh, v, (double)(2 * M),
                        [&](int k) { return cnorm(rfft_harmonic<M>(lds, a.cn.twB, k)); });
        lds_sync<T>();          // the image is rewritten by the next row
    }
}

// the same from the harmonics k_any left in a.cn.harm (row lengths without a tuned plan).  Harmonic 0 is taken from
// the row's own sum: a row of integers that sum to zero has exactly no power there, as in the reference's transform,
// where the chirp transform leaves rounding
template <typename Tin>
__global__ __launch_bounds__(PP_NF_T) void k_noisefit_harm(NoiseFitArgs a) {
    constexpr int T = PP_NF_T;
    __shared__ double d[PP_NF_MAXH];
    __shared__ NoiseFitShared<T> sh;
    const int tid = threadIdx.x;
    const int M = a.cn.M, H = M + 1;
    for (long long r = blockIdx.x; r < a.cn.nrows; r += gridDim.x) {
        const Tin* grow = reinterpret_cast<const Tin*>(a.cn.src) + (size_t)r * (2 * M);
        double v[5];
        chan_noise_start(v);
        for (int j = tid; j < 2 * M; j += T) chan_noise_sample(v, (double)grow[j]);
        chan_noise_reduce<T>(sh.red, v);
        const cplx* h = a.cn.harm + (size_t)r * H;
        const double p0 = v[0] * v[0];
        auto pow_at = [&](int k) { return k == 0 ? p0 : cnorm(h[k]); };
        for (int k = tid; k < H; k += T) d[k] = log10(pow_at(k) / (double)(2 * M));
        noisefit_row<T>(a, r, H, d, sh, v, (double)(2 * M), pow_at);
        __syncthreads();
    }
}

// find_kc itself: rows that already are power spectra
__global__ __launch_bounds__(PP_NF_T) void k_noisefit_pows(NoiseFitArgs a) {
    constexpr int T = PP_NF_T;
    __shared__ double d[PP_NF_MAXH];
    __shared__ NoiseFitShared<T> sh;
    const int tid = threadIdx.x;
    const int H = a.cn.M + 1;
    for (long long r = blockIdx.x; r < a.cn.nrows; r += gridDim.x) {
        const double* p = a.pows + (size_t)r * H;
        double v[5];
        chan_noise_start(v);          // (no samples: norm 1)
        for (int k = tid; k < H; k += T) d[k] = log10(p[k]);
        noisefit_row<T>(a, r, H, d, sh, v, 1.0, [&](int k) { return p[k]; });
        __syncthreads();
    }
}

}  // namespace pp

// ---- the width grid ----------------------------------------------------------
// What opt.brute(..., Ns=20) builds for find_kc's first axis (pplib.py:1476-1485), np.mgrid[lo:hi:20j] = i step + lo
// with step = (hi - lo) / 19 in NumPy's order of operations, and find_kc's kc of each value (pplib.py:1487-1493)
static void noise_fit_grid(int H, int fn, double* a20, int32_t* kc20) {
    // (len(data)**-1 is Python's float power, the C library's pow at run time, not a division: the two differ in the
    // last bit at H = 1923; the exponent is kept from the compiler, which would fold the call into 1 / H)
    volatile double minus_one = -1.0;
    const double lo = fn == PP_KC_EXP_DC ? std::pow((double)H, minus_one) : 1.0, hi = fn == PP_KC_EXP_DC ? 1.0 : (double)H;
    const double step = (hi - lo) / 19.0;
    for (int i = 0; i < pp::PP_NF_NS; ++i) {
        volatile double prod = (double)i * step;       // (two roundings, as NumPy's: never one fused operation)
        const double a = prod + lo;
        a20[i] = a;
        int kc = H - 1;
        if (fn == PP_KC_EXP_DC) {
            for (int k = 0; k < H; ++k)
                if (std::exp(-a * (double)k) < 0.005) { kc = k; break; }
        } else kc = (int)std::floor(a);
        kc20[i] = kc;
    }
}

extern "C" int pp_noise_fit_grid(int H, int fn, double* a20, int32_t* kc20) {
    if (!a20 || !kc20) return fail(PP_EINVAL, "pp_noise_fit_grid: null argument");
    if (H < 2 || (fn != PP_KC_EXP_DC && fn != PP_KC_HALF_TRI)) return fail(PP_EINVAL, "pp_noise_fit_grid: H %d, fn %d", H, fn);
    noise_fit_grid(H, fn, a20, kc20);
    return PP_OK;
}

static constexpr size_t PP_NF_MAX_TABLES = 32;
// the device table of (H, fn): S_f(a), S_ff(a), klim(a), kc(a) of the 20 a, then f_a(k), [20][H]
static int noise_fit_table(pp_ctx* c, int H, int fn, const double** out) {
    const int key = 2 * H + (fn == PP_KC_HALF_TRI ? 1 : 0);
    auto it = c->nftabs.find(key);
    if (it != c->nftabs.end()) { *out = it->second.as<double>(); return PP_OK; }
    constexpr int NS = pp::PP_NF_NS, HEAD = pp::PP_NF_HEAD;
    double a20[NS];
    int32_t kc20[NS];
    noise_fit_grid(H, fn, a20, kc20);
    std::vector<double> t((size_t)HEAD + (size_t)NS * H, 0.0);
    const double tiny = std::ldexp(1.0, -70);
    for (int q = 0; q < NS; ++q) {
        double* f = t.data() + HEAD + (size_t)q * H;
        long double sf = 0.0L, sff = 0.0L;
        int klim = H;
        if (fn == PP_KC_EXP_DC) {
            for (int k = 0; k < H; ++k) {
                const double e = std::exp(-a20[q] * (double)k);
                if (e < tiny) { klim = k; break; }
                f[k] = e;
            }
        } else {
            const int ai = (int)std::floor(a20[q]);
            klim = std::min(ai, H);
            for (int k = 0; k < klim; ++k) f[k] = 1.0 - (double)k / (double)ai;
        }
        for (int k = 0; k < klim; ++k) { sf += f[k]; sff += (long double)f[k] * f[k]; }
        t[q] = (double)sf; t[NS + q] = (double)sff; t[2 * NS + q] = (double)klim; t[3 * NS + q] = (double)kc20[q];
    }
    // at most PP_NF_MAX_TABLES stay resident (up to 328 KB each): a caller that sweeps row lengths starts over.  Every
    // entry point that uses a table ends with a synchronise of the stream, so none is in use here
    if (c->nftabs.size() >= PP_NF_MAX_TABLES) {
        for (auto& kv : c->nftabs) kv.second.release();
        c->nftabs.clear();
    }
    DevBuf b;
    int rc = b.reserve(t.size() * sizeof(double));
    if (rc) return rc;
    HIP_TRY(hipMemcpy(b.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    c->nftabs[key] = b;
    *out = b.as<double>();
    return PP_OK;
}

// ---- the 'fit' noise of every row ----------------------------------------------
static int noise_fit_run(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, int input_kind, int fn,
                         double fact, int norm_method, const double* divisor, double* norms, double* noise, int32_t* kc,
                         int32_t* cell, double* snrs, double fudge) {
    const int M = nbin / 2, H = M + 1;
    const bool pows = input_kind == PP_NOISEFIT_POWS;
    const bool anyb = !pows && !nbin_ok(nbin);
    int rc;
    const void* dsrc = src;
    if (!on_device) {
        const size_t bytes = pows ? (size_t)nrows * H * 8 : (size_t)nrows * nbin * (dtype == PP_F64 ? 8 : 4);
        if ((rc = upload(c, c->data, src, bytes))) return rc;
        dsrc = c->data.p;
    }
    const double* ddiv = nullptr;
    if (norm_method == PP_NORM_PROF) {
        if ((rc = upload(c, c->wts, divisor, (size_t)nrows * 8))) return rc;
        ddiv = c->wts.as<double>();
    }
    if ((rc = c->sdraw.reserve((size_t)nrows * 8))) return rc;
    if ((rc = c->noise.reserve((size_t)nrows * 8))) return rc;
    if ((rc = c->misc.reserve((size_t)nrows * 16))) return rc;
    if (snrs && (rc = c->csum.reserve((size_t)nrows * 8))) return rc;
    const cplx* tw = nullptr;
    if (!pows && (rc = get_twiddles(c, nbin, &tw))) return rc;
    const double* tab = nullptr;
    if ((rc = noise_fit_table(c, H, fn, &tab))) return rc;
    int* dkc = c->misc.as<int>();
    NoiseFitArgs a{{pows ? nullptr : dsrc, nullptr, tw, ddiv, c->sdraw.as<double>(), c->noise.as<double>(), nrows, M, norm_method,
                    snrs ? c->csum.as<double>() : nullptr, fudge},
                   pows ? (const double*)dsrc : nullptr, tab, fact, dkc, dkc + nrows};
    if (anyb) {
        if ((rc = c->X.reserve((size_t)nrows * H * sizeof(cplx)))) return rc;
        if ((rc = harmonics_any(c, dsrc, dtype, 1, nrows, nbin, c->X.as<cplx>()))) return rc;
        a.cn.harm = c->X.as<cplx>();
    }
    {
        Prof pr(c, KF_NOISEFIT);
        if (pows) {
            hipLaunchKernelGGL(k_noisefit_pows, dim3(any_grid(nrows)), dim3(PP_NF_T), 0, c->stream, a);
        } else if (anyb) {
            with_dtype(dtype, [&](auto t) {
                hipLaunchKernelGGL(k_noisefit_harm<decltype(t)>, dim3(any_grid(nrows)), dim3(PP_NF_T), 0, c->stream, a);
            });
        } else {
            PP_DISPATCH_M(M, {
                if constexpr (MM + 1 <= PP_NF_MAXH) {
                    const int T = FftPlan<MM>::T;
                    with_dtype(dtype, [&](auto t) {
                        hipLaunchKernelGGL((k_noisefit<MM, decltype(t)>),
                                           dim3(resident_grid(c, k_noisefit<MM, decltype(t)>, T, nrows, fft_grid(T, nrows))), dim3(T), 0,
                                           c->stream, a);
                    });
                } else return fail(PP_EINVAL, "pp_channel_noise_fit: nbin %d", nbin);
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(norms, c->sdraw.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(noise, c->noise.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    if (kc) HIP_TRY(hipMemcpyAsync(kc, dkc, (size_t)nrows * 4, hipMemcpyDeviceToHost, c->stream));
    if (cell) HIP_TRY(hipMemcpyAsync(cell, dkc + nrows, (size_t)nrows * 12, hipMemcpyDeviceToHost, c->stream));
    if (snrs) HIP_TRY(hipMemcpyAsync(snrs, c->csum.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

static int noise_fit_rows(pp_ctx* c, const char* who, const void* src, int dtype, int on_device, int nrows, int nbin,
                          int input_kind, int fn, double fact, int norm_method, const double* divisor, double* norms,
                          double* noise, int32_t* kc, int32_t* cell, double* snrs, double fudge) {
    if (int busy_ = ctx_busy(c, who)) return busy_;
    if (!c || !src || !norms || !noise) return fail(PP_EINVAL, "%s: null argument", who);
    if (!nbin_any_ok(nbin) || nbin > 4096) return fail(PP_EINVAL, "%s: nbin %d must be even and in [8, 4096]", who, nbin);
    if (nrows < 1) return fail(PP_EINVAL, "%s: bad shape %d x %d", who, nrows, nbin);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "%s: dtype %d", who, dtype);
    if (input_kind != PP_NOISEFIT_ROWS && input_kind != PP_NOISEFIT_POWS) return fail(PP_EINVAL, "%s: input kind %d", who, input_kind);
    if (fn != PP_KC_EXP_DC && fn != PP_KC_HALF_TRI) return fail(PP_EINVAL, "%s: fn %d", who, fn);
    if (!(fact >= 0.0) || !(fact < 1e6)) return fail(PP_EINVAL, "%s: fact %g", who, fact);
    if (norm_method < PP_NORM_NONE || norm_method > PP_NORM_ABS) return fail(PP_EINVAL, "%s: norm method %d", who, norm_method);
    if (norm_method == PP_NORM_PROF && !divisor) return fail(PP_EINVAL, "%s: norm 'prof' needs the divisors", who);
    const bool pows = input_kind == PP_NOISEFIT_POWS;
    if (pows && (dtype != PP_F64 || norm_method != PP_NORM_NONE))
        return fail(PP_EINVAL, "%s: power spectra are f64 and take no norm", who);
    HIP_TRY(hipSetDevice(c->device));
    const size_t rowb = pows ? (size_t)(nbin / 2 + 1) * 8 : (size_t)nbin * (dtype == PP_F64 ? 8 : 4);
    const size_t harmb = pows || nbin_ok(nbin) ? 0 : (size_t)(nbin / 2 + 1) * sizeof(cplx);
    int cap = on_device ? nrows : aux_chunk_cap(c, (double)(rowb + harmb) + 40.0, nrows);
    if (harmb) cap = std::min<long long>(cap, std::max<long long>(1, ((long long)256 << 20) / (long long)harmb));
    return for_runs(nrows, cap, [&](Run r) {
        return noise_fit_run(c, r.at((const char*)src, rowb), dtype, on_device, r.n, nbin, input_kind, fn, fact, norm_method,
                             r.at(divisor, 1), r.at(norms, 1), r.at(noise, 1), r.at(kc, 1), r.at(cell, 3), r.at(snrs, 1), fudge);
    });
}

// pplib.get_noise_fit(row, fact) (pplib.py:2255-2287) of every row with find_kc (pplib.py:1465-1495) inside it, and
// normalize_portrait's norm (pplib.py:2462-2507) as pp_channel_noise forms it; rows that already are power spectra
// are find_kc's own input
extern "C" int pp_channel_noise_fit(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, int input_kind,
                                    int fn, double fact, int norm_method, const double* divisor, double* norms, double* noise,
                                    int32_t* kc, int32_t* cell) {
    return noise_fit_rows(c, "pp_channel_noise_fit", src, dtype, on_device, nrows, nbin, input_kind, fn, fact, norm_method,
                          divisor, norms, noise, kc, cell, nullptr, 1.0);
}

// pplib.get_SNR(row, fudge) (pplib.py:2289-2308) with get_noise(method='fit') (pplib.py:2221-2222) as its noise:
// sum, maximum and noise from one pass over the row
extern "C" int pp_channel_snrs_fit(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, int fn,
                                   double fact, double fudge, double* snrs) {
    if (!snrs || nrows < 1) return fail(PP_EINVAL, "pp_channel_snrs_fit: null argument or no rows");
    std::vector<double> norms((size_t)nrows), noise((size_t)nrows);
    return noise_fit_rows(c, "pp_channel_snrs_fit", src, dtype, on_device, nrows, nbin, PP_NOISEFIT_ROWS, fn, fact,
                          PP_NORM_NONE, nullptr, norms.data(), noise.data(), nullptr, nullptr, snrs, fudge);
}
