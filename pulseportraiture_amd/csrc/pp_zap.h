// ppzap on the device (included at the end of pp_toas.hip): the channel noise of every row
// (pplib.get_noise_PS, frac = 4) with normalize_portrait's norm, and get_zap_channels' iterative
// median / sigma clip of that noise, one workgroup per subint.

namespace pp {

struct ChanNoiseArgs {
    const void* src;          // [nrows][2 M]
    const cplx* harm;         // [nrows][M + 1] k_any's harmonics (rows of no tuned plan), or nullptr
    const cplx* twB;          // W_B^k, k = 0..M
    const double* divisor;    // [nrows] the norms of PP_NORM_PROF, or nullptr
    double* norms;            // [nrows]
    double* noise;            // [nrows] noise of the normalised row: noise / |norm|
    long long nrows;
    int M, method;
    double* snr;              // [nrows] get_SNR of the row (pp_channel_snrs), or nullptr
    double fudge;
};

// workgroup totals of the lanes' v = {sum, maximum, sum of squares, max |x| (!= 0 iff row.any()), power of
// the top quarter of the harmonics}; every lane returns them
template <int T>
__device__ __forceinline__ void chan_noise_reduce(double* red, double v[5]) {
    constexpr int NW = T / 64;
    const int tid = threadIdx.x;
    v[0] = group_sum<64>(v[0]);
    v[1] = group_max<64>(v[1]);
    v[2] = group_sum<64>(v[2]);
    v[3] = group_max<64>(v[3]);
    v[4] = group_sum<64>(v[4]);
    if (NW > 1) {
        if ((tid & 63) == 0)
            for (int q = 0; q < 5; ++q) red[(tid >> 6) * 5 + q] = v[q];
        __syncthreads();
        for (int q = 0; q < 5; ++q) v[q] = red[q];
        for (int w = 1; w < NW; ++w) {
            v[0] += red[w * 5]; v[1] = fmax(v[1], red[w * 5 + 1]); v[2] += red[w * 5 + 2];
            v[3] = fmax(v[3], red[w * 5 + 3]); v[4] += red[w * 5 + 4];
        }
        __syncthreads();
    }
}

// normalize_portrait (pplib.py:2462-2507): rows with no non-zero sample keep norm 1 (and noise 0)
// (noise: the row's own, by whichever estimator)
__device__ __forceinline__ void chan_noise_finish(const ChanNoiseArgs& a, long long r, const double v[5], double noise) {
    double norm = 1.0;
    if (v[3] != 0.0) {
        switch (a.method) {
            case PP_NORM_MEAN: norm = v[0] / (2.0 * a.M); break;
            case PP_NORM_MAX: norm = v[1]; break;
            case PP_NORM_PROF: norm = a.divisor[r]; break;
            case PP_NORM_RMS: norm = noise; break;
            case PP_NORM_ABS: norm = sqrt(v[2]); break;
            default: break;
        }
    }
    a.norms[r] = norm;
    a.noise[r] = noise / fabs(norm);
    if (a.snr) {
        // get_SNR (pplib.py:2289-2308; its dc is 0): the equivalent width sum / max, 1 and a zero result where
        // that is not positive
        double Weq = v[0] / v[1];
        const double keep = Weq <= 0.0 ? 0.0 : 1.0;
        if (Weq <= 0.0) Weq = 1.0;
        a.snr[r] = v[0] / (noise * sqrt(Weq)) * keep / a.fudge;
    }
}

__device__ __forceinline__ void chan_noise_store(const ChanNoiseArgs& a, long long r, const double v[5]) {
    const int M = a.M, H = M + 1, kc = (int)(0.75 * H);    // get_noise_PS: int((1 - 1/4) * len(pows))
    chan_noise_finish(a, r, v, sqrt(v[4] / (2.0 * M) / (double)(H - kc)));
}

__device__ __forceinline__ void chan_noise_start(double v[5]) {
    v[0] = 0.0; v[1] = -INFINITY; v[2] = 0.0; v[3] = 0.0; v[4] = 0.0;
}
__device__ __forceinline__ void chan_noise_sample(double v[5], double x) {
    v[0] += x;
    v[1] = fmax(v[1], x);
    v[2] = fma(x, x, v[2]);
    v[3] = fmax(v[3], fabs(x));
}

// one workgroup per row (as k_rfft_rows): the row is read once, into the registers of the transform's first
// stage, and its moments are taken there; then the transform and the power of the top quarter of its
// harmonics; nothing but the two scalars of the row is written
template <int M, typename Tin>
__global__ __launch_bounds__(FftPlan<M>::T) void k_chan_noise(ChanNoiseArgs a) {
    constexpr int T = FftPlan<M>::T, R1 = FftPlan<M>::R1, PER1 = FftPlan<M>::PER1;
    constexpr int NBF = StageGeom<M, T, R1>::NBF;
    typedef typename RawOf<Tin>::type Raw;
    __shared__ cplx lds[FftPlan<M>::LDS_ELEMS];
    __shared__ double red[5 * (T / 64)];
    const int tid = threadIdx.x;
    const int kc = (int)(0.75 * (M + 1));
    for (long long r = blockIdx.x; r < a.nrows; r += gridDim.x) {
        const Tin* grow = reinterpret_cast<const Tin*>(a.src) + (size_t)r * (2 * M);
        Raw raw[PER1][R1];
        stage_load_global<M, T, R1>(raw, grow, tid);
        RowTwiddles<M> tw;
        load_row_twiddles<M>(tw, a.twB, tid);
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
        for (int k = kc + tid; k <= M; k += T) v[4] += cnorm(rfft_harmonic<M>(lds, a.twB, k));
        chan_noise_reduce<T>(red, v);
        if (tid == 0) chan_noise_store(a, r, v);
        lds_sync<T>();          // the image is rewritten by the next row
    }
}

// the same from the harmonics k_any left in a.harm (row lengths without a tuned plan)
template <typename Tin>
__global__ __launch_bounds__(64) void k_chan_noise_harm(ChanNoiseArgs a) {
    const int M = a.M, kc = (int)(0.75 * (M + 1));
    const long long r = blockIdx.x;
    // (k_any has read the row for its transform: this second read is the compatibility path's)
    const Tin* grow = reinterpret_cast<const Tin*>(a.src) + (size_t)r * (2 * M);
    double v[5];
    chan_noise_start(v);
    for (int j = threadIdx.x; j < 2 * M; j += 64) chan_noise_sample(v, (double)grow[j]);
    const cplx* h = a.harm + (size_t)r * (M + 1);
    for (int k = kc + (int)threadIdx.x; k <= M; k += 64) v[4] += cnorm(h[k]);
    chan_noise_reduce<64>(nullptr, v);
    if (threadIdx.x == 0) chan_noise_store(a, r, v);
}

// get_zap_channels (ppzap.py:18-47) for one subint per workgroup: its good channels' values are
// sorted in LDS (absent and removed channels sort last as +inf) for the median; mean and
// population std of the same values; every channel above median + nstd std leaves at once, and
// the rounds end on one that flags nothing or when no channel is left
constexpr int PP_ZAP_MAXCHAN = 4096;
constexpr int PP_ZAP_T = 256;

__global__ __launch_bounds__(PP_ZAP_T) void k_zap_median(const double* noise, const unsigned char* good, int nchan,
                                                         double nstd, unsigned char* zap) {
    __shared__ double s[PP_ZAP_MAXCHAN];
    __shared__ unsigned char alive[PP_ZAP_MAXCHAN];
    __shared__ double red[PP_ZAP_T / 64];
    __shared__ int nflag;
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nchan;
    const double* x = noise + base;
    int P = 1;
    while (P < nchan) P <<= 1;
    for (int n = tid; n < nchan; n += PP_ZAP_T) {
        alive[n] = good[base + n] ? 1 : 0;
        zap[base + n] = 0;
    }
    __syncthreads();
    auto block_sum = [&](double v) {
        v = group_sum<64>(v);
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        double t = 0.0;
        for (int w = 0; w < PP_ZAP_T / 64; ++w) t += red[w];
        __syncthreads();
        return t;
    };
    for (;;) {
        double cnt = 0.0, sum = 0.0;
        for (int n = tid; n < P; n += PP_ZAP_T) {
            const bool on = n < nchan && alive[n];
            s[n] = on ? x[n] : INFINITY;
            if (on) { cnt += 1.0; sum += x[n]; }
        }
        const int nalive = (int)block_sum(cnt);
        if (nalive == 0) break;
        const double mean = block_sum(sum) / nalive;
        double dev = 0.0;
        for (int n = tid; n < nchan; n += PP_ZAP_T)
            if (alive[n]) dev += (x[n] - mean) * (x[n] - mean);
        const double sd = sqrt(block_sum(dev) / nalive);
        // bitonic sort of s[0 .. P)
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P; i += PP_ZAP_T) {
                    const int l = i ^ j;
                    if (l > i) {
                        const double u = s[i], w = s[l];
                        if (((i & k) == 0) == (u > w)) { s[i] = w; s[l] = u; }
                    }
                }
                __syncthreads();
            }
        const double med = (nalive & 1) ? s[nalive / 2] : (s[nalive / 2 - 1] + s[nalive / 2]) / 2.0;
        const double thr = med + nstd * sd;
        if (tid == 0) nflag = 0;
        __syncthreads();
        for (int n = tid; n < nchan; n += PP_ZAP_T)
            if (alive[n] && x[n] > thr) {
                alive[n] = 0;
                zap[base + n] = 1;
                atomicAdd(&nflag, 1);
            }
        __syncthreads();
        if (nflag == 0) break;
    }
}

}  // namespace pp

// ---- ppzap: channel noise and norms ------------------------------------------
// pplib.get_noise_PS(row, frac=4) (pplib.py:2227-2253) of every row, with the norm of
// normalize_portrait (pplib.py:2462-2507) that ppzap applies before it (ppzap.py:222-230)
// (snrs: pp_channel_snrs' output of the same pass, or nullptr)
static int channel_noise_run(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, int norm_method,
                             const double* divisor, double* norms, double* noise, double* snrs, double fudge) {
    const int M = nbin / 2;
    const bool anyb = !nbin_ok(nbin);
    int rc;
    const void* dsrc = src;
    if (!on_device) {
        if ((rc = upload(c, c->data, src, (size_t)nrows * nbin * (dtype == PP_F64 ? 8 : 4)))) return rc;
        dsrc = c->data.p;
    }
    const double* ddiv = nullptr;
    if (norm_method == PP_NORM_PROF) {
        if ((rc = upload(c, c->wts, divisor, (size_t)nrows * 8))) return rc;
        ddiv = c->wts.as<double>();
    }
    if ((rc = c->sdraw.reserve((size_t)nrows * 8))) return rc;
    if ((rc = c->noise.reserve((size_t)nrows * 8))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    if (snrs && (rc = c->csum.reserve((size_t)nrows * 8))) return rc;
    ChanNoiseArgs a{dsrc, nullptr, tw, ddiv, c->sdraw.as<double>(), c->noise.as<double>(), nrows, M, norm_method,
                    snrs ? c->csum.as<double>() : nullptr, fudge};
    if (anyb) {
        if ((rc = c->X.reserve((size_t)nrows * (M + 1) * sizeof(cplx)))) return rc;
        if ((rc = harmonics_any(c, dsrc, dtype, 1, nrows, nbin, c->X.as<cplx>()))) return rc;
        a.harm = c->X.as<cplx>();
        with_dtype(dtype, [&](auto t) { hipLaunchKernelGGL(k_chan_noise_harm<decltype(t)>, dim3(nrows), dim3(64), 0, c->stream, a); });
    } else {
        PP_DISPATCH_M(M, {
            const int T = FftPlan<MM>::T;
            // (a persistent grid of the kernel's residency: registers, not LDS, bound it at M = 1024)
            with_dtype(dtype, [&](auto t) {
                hipLaunchKernelGGL((k_chan_noise<MM, decltype(t)>), dim3(resident_grid(c, k_chan_noise<MM, decltype(t)>, T, nrows, fft_grid(T, nrows))),
                                   dim3(T), 0, c->stream, a);
            });
        });
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(norms, c->sdraw.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(noise, c->noise.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    if (snrs) HIP_TRY(hipMemcpyAsync(snrs, c->csum.p, (size_t)nrows * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

static int channel_noise_rows(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, int norm_method,
                              const double* divisor, double* norms, double* noise, double* snrs, double fudge) {
    if (int busy_ = ctx_busy(c, "pp_channel_noise")) return busy_;
    if (!c || !src || !norms || !noise) return fail(PP_EINVAL, "pp_channel_noise: null argument");
    if (!nbin_any_ok(nbin) || nbin > 4096) return fail(PP_EINVAL, "pp_channel_noise: nbin %d must be even and in [8, 4096]", nbin);
    if (nrows < 1) return fail(PP_EINVAL, "pp_channel_noise: bad shape %d x %d", nrows, nbin);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_channel_noise: dtype %d", dtype);
    if (norm_method < PP_NORM_NONE || norm_method > PP_NORM_ABS) return fail(PP_EINVAL, "pp_channel_noise: norm method %d", norm_method);
    if (norm_method == PP_NORM_PROF && !divisor) return fail(PP_EINVAL, "pp_channel_noise: norm 'prof' needs the divisors");
    HIP_TRY(hipSetDevice(c->device));
    // runs of rows: host rows through the work memory, and k_any's harmonics of at most 256 MiB at a time (device rows too)
    const size_t rowb = (size_t)nbin * (dtype == PP_F64 ? 8 : 4), harmb = nbin_ok(nbin) ? 0 : (size_t)(nbin / 2 + 1) * sizeof(cplx);
    int cap = on_device ? nrows : aux_chunk_cap(c, (double)(rowb + harmb) + 24.0, nrows);
    if (harmb) cap = std::min<long long>(cap, std::max<long long>(1, ((long long)256 << 20) / (long long)harmb));
    return for_runs(nrows, cap, [&](Run r) {
        return channel_noise_run(c, r.at((const char*)src, rowb), dtype, on_device, r.n, nbin, norm_method, r.at(divisor, 1),
                                 r.at(norms, 1), r.at(noise, 1), r.at(snrs, 1), fudge);
    });
}

extern "C" int pp_channel_noise(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin,
                                int norm_method, const double* divisor, double* norms, double* noise) {
    return channel_noise_rows(c, src, dtype, on_device, nrows, nbin, norm_method, divisor, norms, noise, nullptr, 1.0);
}

// ---- ppspline: channel S/N ----------------------------------------------------
// pplib.get_SNR(row, fudge) (pplib.py:2289-2308) of every row: its sum, maximum and get_noise_PS noise from one
// pass over it
extern "C" int pp_channel_snrs(pp_ctx* c, const void* src, int dtype, int on_device, int nrows, int nbin, double fudge,
                               double* snrs) {
    if (!snrs || nrows < 1) return fail(PP_EINVAL, "pp_channel_snrs: null argument or no rows");
    std::vector<double> norms((size_t)nrows), noise((size_t)nrows);
    return channel_noise_rows(c, src, dtype, on_device, nrows, nbin, PP_NORM_NONE, nullptr, norms.data(), noise.data(), snrs,
                              fudge);
}

// ---- ppzap: the median / sigma clip ----------------------------------------
// get_zap_channels (ppzap.py:18-47) over the good channels of every subint at once
extern "C" int pp_zap_median(pp_ctx* c, const double* noise, const unsigned char* good, int nsub, int nchan, double nstd,
                             unsigned char* zap) {
    if (int busy_ = ctx_busy(c, "pp_zap_median")) return busy_;
    if (!c || !noise || !good || !zap) return fail(PP_EINVAL, "pp_zap_median: null argument");
    if (nsub < 1 || nchan < 1 || nchan > PP_ZAP_MAXCHAN)
        return fail(PP_EINVAL, "pp_zap_median: bad shape %d x %d (at most %d channels)", nsub, nchan, PP_ZAP_MAXCHAN);
    HIP_TRY(hipSetDevice(c->device));
    const size_t nc = (size_t)nsub * nchan;
    int rc;
    if ((rc = upload(c, c->errs, noise, nc * 8))) return rc;
    if ((rc = upload(c, c->mask, good, nc))) return rc;
    if ((rc = c->misc.reserve(nc))) return rc;
    hipLaunchKernelGGL(k_zap_median, dim3(nsub), dim3(PP_ZAP_T), 0, c->stream, c->errs.as<double>(),
                       c->mask.as<unsigned char>(), nchan, nstd, c->misc.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(zap, c->misc.p, nc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}
