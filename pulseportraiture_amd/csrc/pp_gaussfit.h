// ppgauss on the device (included at the end of pp_toas.hip, after pp_pca.h): what a Levenberg-Marquardt fit of a
// Gaussian-component portrait (fit_gaussian_portrait, pplib.py:1924-2052) needs per iteration.  The data portrait and
// 1 / sigma_n stay resident between pp_gauss_fit_begin and pp_gauss_fit_end.  pp_gauss_residuals forms the weighted
// residual rows (data_n - model_n(params_s)) / sigma_n of up to 100 parameter sets -- the base point and one stepped
// parameter each for a forward-difference Jacobian -- in one launch, the model rows by the very code of
// k_gauss_rows / k_gauss_portrait (pp_extra.h).  pp_gauss_normal reduces them to chi^2, J^T r and J^T J by a
// two-stage slab sum in a fixed order, without floating-point atomics: the same call gives the same bits.
//
// A joined fit (gen_gaussian_portrait's join_ichans, pplib.py:923-929) fits one model to several bands at once, every
// band with a phase offset and a Delta-DM of its own: pp_gauss_fit_join makes the channels' band indices resident, and
// pp_gauss_residuals then rotates the model row of channel n of set s by phi_n = phase_sj + Dconst DM_sj (nu_n^-2 -
// nu_ref^-2) / P, j the channel's band, inside the row's own pass through its harmonics (gauss_portrait_row).

namespace pp {

constexpr int GFIT_MAX_GAUSS = 16;       // components of a fitted model
constexpr int GFIT_MAX_SETS = 100;       // parameter sets per pp_gauss_residuals / pp_gauss_normal
constexpr int GFIT_MAX_JOIN = 16;        // bands of a joined fit
constexpr int GN_TJ = 32;                // samples of every set staged in LDS per step of the reduction
constexpr int GN_T = 256;                // threads of a reduction workgroup
constexpr int GN_ACC = (GFIT_MAX_SETS * GFIT_MAX_SETS + GN_T - 1) / GN_T;     // pair sums held per thread

struct GaussFitArgs {
    const double* freqs;      // [nchan]
    const double* data;       // [nchan][B], f64
    const double* isig;       // [nchan] 1 / sigma_n
    const double* comps;      // [nsets][ngauss][6]
    const double* scal;       // [3][nsets]: dc, tau (rot at nu_ref), alpha of every set
    const cplx* twB;
    double* R;                // [nsets][nchan][B]
    double nu_ref;
    int nchan, ngauss, nsets;
    int code_loc, code_wid, code_amp;
    const int* band;          // [nchan] band of every channel, -1: in none (null: no joined fit)
    const double* join;       // [nsets][njoin][2]: phase, Delta-DM of every set and band (null: all zero)
    double P;                 // the period the Delta-DMs turn into rotations with
    int njoin;
};

// the rotation of channel n (frequency nu) in set s of a joined fit, k_rotate's expression with nu_DM = nu_ref;
// 0 outside joined fits and for a channel in no band
__device__ __forceinline__ double gauss_fit_rotation(const GaussFitArgs& f, int s, int n, double nu) {
    if (!f.band || !f.join) return 0.0;
    const int j = f.band[n];
    if (j < 0) return 0.0;
    const double* pj = f.join + ((size_t)s * f.njoin + j) * 2;
    return pj[0] + PP_DCONST * pj[1] * (1.0 / (nu * nu) - 1.0 / (f.nu_ref * f.nu_ref)) / f.P;
}

// the template arguments of parameter set s
__device__ __forceinline__ GaussArgs gauss_fit_set(const GaussFitArgs& f, int s) {
    return GaussArgs{f.freqs, f.comps + (size_t)s * f.ngauss * 6, f.twB, nullptr, f.nu_ref, f.scal[s], f.scal[f.nsets + s],
                     f.scal[2 * f.nsets + s], f.nchan, f.ngauss, f.code_loc, f.code_wid, f.code_amp};
}

// a generated row leaves as the weighted residual against its data row (GaussRowOut's counterpart)
struct GaussResidOut {
    const double* data;
    double* out;
    double isig;
    __device__ __forceinline__ void one(int j, double v) const { out[j] = (data[j] - v) * isig; }
    __device__ __forceinline__ void two(int j, double v0, double v1) const {
        const double2 d = reinterpret_cast<const double2*>(data)[j];
        reinterpret_cast<double2*>(out)[j] = make_double2((d.x - v0) * isig, (d.y - v1) * isig);
    }
};

// R[s][n][:] of rows of 2 M bins: one workgroup per (channel n = blockIdx.x, set s = blockIdx.y)
template <int M>
__global__ __launch_bounds__(FftPlan<M>::T) void k_gauss_resid(GaussFitArgs f) {
    constexpr int B = 2 * M;
    __shared__ cplx lds[FftPlan<M>::LDS_ELEMS];
    __shared__ cplx zin[M];
    __shared__ GaussComp gc[PP_MAX_GAUSS];
    const int n = blockIdx.x, s = blockIdx.y;
    const GaussArgs a = gauss_fit_set(f, s);
    const double nu = f.freqs[n];
    gauss_portrait_row<M>(a, nu, lds, zin, gc, threadIdx.x,
                          GaussResidOut{f.data + (size_t)n * B, f.R + ((size_t)s * f.nchan + n) * B, f.isig[n]},
                          gauss_fit_rotation(f, s, n, nu));
}

// general row lengths: the unscattered model rows of every set into R (k_gauss_rows' row); a scattered set's rows
// then go through the harmonics as gauss_generate's do, and k_gauss_resid_finish turns models into residuals
__global__ __launch_bounds__(256) void k_gauss_fit_rows(GaussFitArgs f, int B) {
    __shared__ GaussComp gc[PP_MAX_GAUSS];
    const int n = blockIdx.x, s = blockIdx.y;
    const GaussArgs a = gauss_fit_set(f, s);
    gauss_plain_row(a, f.freqs[n], B, gc, threadIdx.x, 256, GaussRowOut{f.R + ((size_t)s * f.nchan + n) * B});
}
// general row lengths, an unscattered set of a joined fit with a rotation somewhere: all its rows went through their
// harmonics, and a row whose own rotation is zero came back moved by a rounding; it is written again, so that such a
// row has the bits it has without a band map -- as at the power-of-two lengths, where it never sees a transform
__global__ __launch_bounds__(256) void k_gauss_fit_unrotated(GaussFitArgs f, int B, int s) {
    __shared__ GaussComp gc[PP_MAX_GAUSS];
    const int n = blockIdx.x;
    const double nu = f.freqs[n];
    if (gauss_fit_rotation(f, s, n, nu) != 0.0) return;       // (the same for every thread of the workgroup)
    const GaussArgs a = gauss_fit_set(f, s);
    gauss_plain_row(a, nu, B, gc, threadIdx.x, 256, GaussRowOut{f.R + ((size_t)s * f.nchan + n) * B});
}
__global__ __launch_bounds__(256) void k_gauss_resid_finish(GaussFitArgs f, int B) {
    const int n = blockIdx.x, s = blockIdx.y;
    double* row = f.R + ((size_t)s * f.nchan + n) * B;
    const GaussResidOut o{f.data + (size_t)n * B, row, f.isig[n]};
    for (int j = threadIdx.x; j < B; j += 256) o.one(j, row[j]);
}

// general row lengths, a set of a joined fit with a rotation somewhere: k_scatter_harm's filter with the scattering
// time of the row, then the row's rotation -- h_nk <- h_nk / (1 + 2 pi i k tau_n) e^{2 pi i k phi_n}; DC unchanged,
// Nyquist Re(d_M B_M) cos(2 pi M phi_n) (gauss_portrait_row).  harm: the harmonics of set s's rows
__global__ __launch_bounds__(256) void k_gauss_join_harm(cplx* harm, GaussFitArgs f, int s, int M) {
    const int n = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > M || k == 0) return;
    const double nu = f.freqs[n];
    const double tau_ref = f.scal[f.nsets + s];
    const double taun = (tau_ref != 0.0) ? tau_ref * pow(nu / f.nu_ref, f.scal[2 * f.nsets + s]) : 0.0;
    const double phin = gauss_fit_rotation(f, s, n, nu);
    cplx* h = harm + (size_t)n * (M + 1);
    const double xk = PP_TWO_PI * (double)k * taun, dk = 1.0 / (1.0 + xk * xk);
    if (k == M) {
        double yM = h[M].x * dk;
        if (phin != 0.0) yM *= unit_phasor((double)M, phin).x;
        h[M] = make_double2(yM, 0.0);
    } else {
        cplx y = cmul(h[k], make_double2(dk, -xk * dk));
        if (phin != 0.0) y = cmul(y, unit_phasor((double)k, phin));
        h[k] = y;
    }
}

template <typename Tin>
__global__ __launch_bounds__(256) void k_gauss_widen(const void* src, double* dst, size_t n) {
    const Tin* x = reinterpret_cast<const Tin*>(src);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) dst[j] = (double)x[j];
}

// Stage one of the normal equations.  With V_0 = R_0 and V_a = (R_a - R_0) / h_{a-1} (a = 1 .. nsets - 1) the Gram
// matrix V V^T holds chi^2 = V_0 . V_0, g_a = V_a . V_0 and G_ab = V_a . V_b.  Workgroup c owns samples
// [c chunk, (c + 1) chunk) and writes its sums of the pairs a <= b to part[c][a nsets + b]; thread t owns the pairs
// t, t + 256, ... and adds its products sample by sample, in order (every product and every sum rounded on its own:
// the terms are the ones a host sum of V_a[j] V_b[j] sees).
__global__ __launch_bounds__(GN_T) void k_gauss_normal_part(const double* R, const double* h, int nsets, long long nrow,
                                                            int chunk, double* part) {
    __shared__ double V[GFIT_MAX_SETS][GN_TJ + 1];
    const int tid = threadIdx.x;
    const int NP = nsets * nsets;
    const long long j0 = (long long)blockIdx.x * chunk, j1 = min(nrow, j0 + (long long)chunk);
    double acc[GN_ACC];
    int ab[GN_ACC];
#pragma unroll
    for (int i = 0; i < GN_ACC; ++i) {
        const int p = tid + GN_T * i;
        const int a = p / nsets, b = p - a * nsets;
        acc[i] = 0.0;
        ab[i] = (p < NP && a <= b) ? (a << 8 | b) : -1;
    }
    for (long long t0 = j0; t0 < j1; t0 += GN_TJ) {
        for (int idx = tid; idx < nsets * GN_TJ; idx += GN_T) {
            const int a = idx / GN_TJ, jj = idx - a * GN_TJ;
            const long long j = t0 + jj;
            double v = 0.0;
            if (j < j1) {
                const double r0 = R[j];
                v = (a == 0) ? r0 : (R[(size_t)a * nrow + j] - r0) / h[a - 1];
            }
            V[a][jj] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GN_ACC; ++i) {
            if (ab[i] >= 0) {
                const double* va = V[ab[i] >> 8];
                const double* vb = V[ab[i] & 255];
                double s = acc[i];
#pragma unroll 4
                for (int jj = 0; jj < GN_TJ; ++jj) s = add_rn(s, mul_rn(va[jj], vb[jj]));
                acc[i] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < GN_ACC; ++i)
        if (ab[i] >= 0) part[(size_t)blockIdx.x * NP + tid + GN_T * i] = acc[i];
}

// Stage two: the chunks' partials added in chunk order, one thread per pair; the full symmetric matrix out[nsets][nsets]
__global__ __launch_bounds__(256) void k_gauss_normal_sum(const double* part, int nchunk, int nsets, double* out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int NP = nsets * nsets;
    if (p >= NP) return;
    const int a = p / nsets, b = p - a * nsets;
    if (a > b) return;
    double s = 0.0;
    for (int q = 0; q < nchunk; ++q) s = add_rn(s, part[(size_t)q * NP + p]);
    out[(size_t)a * nsets + b] = s;
    out[(size_t)b * nsets + a] = s;
}

}  // namespace pp

// the residual rows of one call may take this much device memory (nsets nchan nbin 8 bytes)
static const double kGaussFitMaxBytes = 2147483648.0;

// samples per workgroup of the reduction's first stage: a function of the row count alone (at most 1024 chunks of whole
// LDS steps, at least 256 samples each), never of the device
static int gauss_normal_chunk(long long nrow) {
    const long long per = (nrow + 1023) / 1024;
    return (int)std::max<long long>(256, (per + pp::GN_TJ - 1) / pp::GN_TJ * pp::GN_TJ);
}

extern "C" int pp_gauss_fit_begin(pp_ctx* c, const void* data, int dtype, int on_device, int nchan, int nbin,
                                  const double* freqs, const double* errs) {
    if (int busy_ = ctx_busy(c, "pp_gauss_fit_begin")) return busy_;
    if (!c || !data || !freqs || !errs) return fail(PP_EINVAL, "pp_gauss_fit_begin: null argument");
    pp_ctx::GaussFit& F = c->gfit;
    F.open = false;             // (a refused begin leaves no fit open either)
    F.nsets = 0;
    F.njoin = 0;                // (... and no band map)
    if (!nbin_any_ok(nbin)) return nbin_refuse("pp_gauss_fit_begin", nbin);
    if (nchan < 1) return fail(PP_EINVAL, "pp_gauss_fit_begin: bad shape %d x %d", nchan, nbin);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_gauss_fit_begin: dtype %d", dtype);
    std::vector<double> isig((size_t)nchan);
    for (int n = 0; n < nchan; ++n) {
        if (!(errs[n] > 0.0) || std::isinf(errs[n])) return fail(PP_EINVAL, "pp_gauss_fit_begin: errs[%d] = %g is no noise level", n, errs[n]);
        if (!(freqs[n] > 0.0)) return fail(PP_EINVAL, "pp_gauss_fit_begin: freqs[%d] = %g", n, freqs[n]);
        isig[n] = 1.0 / errs[n];
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t nel = (size_t)nchan * nbin;
    int rc;
    if ((rc = F.data.reserve(nel * 8))) return rc;
    if (dtype == PP_F64) {
        HIP_TRY(hipMemcpyAsync(F.data.p, data, nel * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    } else {
        const void* src = data;
        if (!on_device) {
            if ((rc = upload(c, c->data, data, nel * 4))) return rc;
            src = c->data.p;
        }
        const int grid = (int)std::min<size_t>((nel + 255) / 256, 4096);
        hipLaunchKernelGGL((k_gauss_widen<float>), dim3(grid), dim3(256), 0, c->stream, src, F.data.as<double>(), nel);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = upload(c, F.isig, isig.data(), (size_t)nchan * 8))) return rc;
    if ((rc = upload(c, F.freqs, freqs, (size_t)nchan * 8))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (isig and the caller's arrays are free again)
    F.nchan = nchan; F.nbin = nbin; F.open = true;
    return PP_OK;
}

extern "C" int pp_gauss_fit_end(pp_ctx* c) {
    if (int busy_ = ctx_busy(c, "pp_gauss_fit_end")) return busy_;
    if (!c) return fail(PP_EINVAL, "pp_gauss_fit_end: null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->gfit.release();
    return PP_OK;
}

extern "C" int pp_gauss_fit_join(pp_ctx* c, int njoin, const int* band_of_chan, double P) {
    if (int busy_ = ctx_busy(c, "pp_gauss_fit_join")) return busy_;
    if (!c || !band_of_chan) return fail(PP_EINVAL, "pp_gauss_fit_join: null argument");
    pp_ctx::GaussFit& F = c->gfit;
    if (!F.open) return fail(PP_ESTATE, "pp_gauss_fit_join: no fit is open (pp_gauss_fit_begin first)");
    if (njoin < 1 || njoin > GFIT_MAX_JOIN) return fail(PP_EINVAL, "pp_gauss_fit_join: %d bands, 1..%d are joined", njoin, GFIT_MAX_JOIN);
    for (int n = 0; n < F.nchan; ++n)
        if (band_of_chan[n] < -1 || band_of_chan[n] >= njoin)
            return fail(PP_EINVAL, "pp_gauss_fit_join: band_of_chan[%d] = %d is outside [-1, %d)", n, band_of_chan[n], njoin);
    if (!(P > 0.0) || std::isinf(P)) return fail(PP_EINVAL, "pp_gauss_fit_join: P = %g is no period", P);
    HIP_TRY(hipSetDevice(c->device));
    F.njoin = 0;
    int rc;
    if ((rc = upload(c, F.band, band_of_chan, (size_t)F.nchan * sizeof(int)))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the caller's array is free again)
    F.njoin = njoin; F.P = P;
    return PP_OK;
}

extern "C" int pp_gauss_residuals(pp_ctx* c, const char* code, double nu_ref, int nsets, const double* dc,
                                  const double* tau_rot, const double* alpha, int ngauss, const double* comps,
                                  double* out_or_null, const double* join_or_null) {
    if (int busy_ = ctx_busy(c, "pp_gauss_residuals")) return busy_;
    if (!c || !code || !dc || !tau_rot || !alpha || !comps) return fail(PP_EINVAL, "pp_gauss_residuals: null argument");
    pp_ctx::GaussFit& F = c->gfit;
    if (!F.open) return fail(PP_ESTATE, "pp_gauss_residuals: no data portrait is resident (pp_gauss_fit_begin first)");
    if (ngauss < 1 || ngauss > GFIT_MAX_GAUSS) return fail(PP_EINVAL, "pp_gauss_residuals: %d components, 1..%d are fitted", ngauss, GFIT_MAX_GAUSS);
    if (nsets < 1 || nsets > GFIT_MAX_SETS) return fail(PP_EINVAL, "pp_gauss_residuals: %d parameter sets, 1..%d per call", nsets, GFIT_MAX_SETS);
    for (int j = 0; j < 3; ++j)
        if (code[j] != '0' && code[j] != '1') return fail(PP_EINVAL, "pp_gauss_residuals: model code '%.3s'", code);
    if (join_or_null && !F.njoin)
        return fail(PP_ESTATE, "pp_gauss_residuals: join parameters without a resident band map (pp_gauss_fit_join first)");
    const int njoin = join_or_null ? F.njoin : 0;
    const int nchan = F.nchan, nbin = F.nbin, M = nbin / 2;
    const size_t nrow = (size_t)nchan * nbin;
    if ((double)nsets * (double)nrow * 8.0 > kGaussFitMaxBytes)
        return fail(PP_EINVAL, "pp_gauss_residuals: %d sets of %d x %d residuals exceed %.0f bytes", nsets, nchan, nbin, kGaussFitMaxBytes);
    HIP_TRY(hipSetDevice(c->device));
    F.nsets = 0;
    int rc;
    // (the join table rides behind the three scalars of every set)
    const size_t njp = (size_t)nsets * njoin * 2;
    std::vector<double> scal(3 * (size_t)nsets + njp);
    std::copy(dc, dc + nsets, scal.begin());
    std::copy(tau_rot, tau_rot + nsets, scal.begin() + nsets);
    std::copy(alpha, alpha + nsets, scal.begin() + 2 * (size_t)nsets);
    if (njp) std::copy(join_or_null, join_or_null + njp, scal.begin() + 3 * (size_t)nsets);
    if ((rc = upload(c, c->x0, scal.data(), scal.size() * 8))) return rc;
    if ((rc = upload(c, c->misc, comps, (size_t)nsets * ngauss * 48))) return rc;
    if ((rc = F.R.reserve((size_t)nsets * nrow * 8))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    GaussFitArgs f{F.freqs.as<double>(), F.data.as<double>(), F.isig.as<double>(), c->misc.as<double>(), c->x0.as<double>(), tw,
                   F.R.as<double>(), nu_ref, nchan, ngauss, nsets, code[0] - '0', code[1] - '0', code[2] - '0',
                   njoin ? F.band.as<int>() : nullptr, njoin ? c->x0.as<double>() + 3 * (size_t)nsets : nullptr, F.P, njoin};
    const dim3 grid((unsigned)nchan, (unsigned)nsets);
    {
        Prof pr(c, KF_GAUSSRES);
        if (!nbin_ok(nbin)) {
            hipLaunchKernelGGL(k_gauss_fit_rows, grid, dim3(256), 0, c->stream, f, nbin);
            HIP_TRY(hipGetLastError());
            const size_t H = (size_t)M + 1;
            for (int s = 0; s < nsets; ++s) {
                // (a set whose join parameters are all zero is an unjoined one, and goes the way it always did)
                bool rot = false;
                for (int q = 0; q < 2 * njoin; ++q) rot = rot || join_or_null[(size_t)s * njoin * 2 + q] != 0.0;
                if (tau_rot[s] == 0.0 && !rot) continue;
                // (gauss_generate's route: chirp-z there, 1 / (1 + 2 pi i k tau_n), and back)
                double* rows = F.R.as<double>() + (size_t)s * nrow;
                if ((rc = c->seedbuf.reserve((size_t)nchan * H * sizeof(cplx)))) return rc;
                cplx* harm = c->seedbuf.as<cplx>();
                if ((rc = harmonics_any(c, rows, PP_F64, 1, nchan, nbin, harm))) return rc;
                if (rot)
                    hipLaunchKernelGGL(k_gauss_join_harm, dim3((unsigned)((H + 255) / 256), nchan), dim3(256), 0, c->stream, harm, f, s, M);
                else
                    hipLaunchKernelGGL(k_scatter_harm, dim3((unsigned)((H + 255) / 256), nchan), dim3(256), 0, c->stream, harm,
                                       (const double*)F.freqs.as<double>(), nu_ref, tau_rot[s], alpha[s], M);
                HIP_TRY(hipGetLastError());
                if ((rc = irfft_any(c, nbin, harm, nchan, rows))) return rc;
                if (rot && tau_rot[s] == 0.0) {
                    hipLaunchKernelGGL(k_gauss_fit_unrotated, dim3((unsigned)nchan), dim3(256), 0, c->stream, f, nbin, s);
                    HIP_TRY(hipGetLastError());
                }
            }
            hipLaunchKernelGGL(k_gauss_resid_finish, grid, dim3(256), 0, c->stream, f, nbin);
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                hipLaunchKernelGGL((k_gauss_resid<MM>), grid, dim3(T), 0, c->stream, f);
            });
        }
    }
    HIP_TRY(hipGetLastError());
    if (out_or_null) HIP_TRY(hipMemcpyAsync(out_or_null, F.R.p, (size_t)nsets * nrow * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the parameter arrays are free again)
    F.nsets = nsets; F.nrow = (long long)nrow;
    return PP_OK;
}

extern "C" int pp_gauss_normal(pp_ctx* c, const double* R_or_null, int on_device, int nsets, int nrow, const double* h,
                               double* chi2, double* g, double* G) {
    if (int busy_ = ctx_busy(c, "pp_gauss_normal")) return busy_;
    if (!c || !chi2) return fail(PP_EINVAL, "pp_gauss_normal: null argument");
    if (nsets < 1 || nsets > GFIT_MAX_SETS) return fail(PP_EINVAL, "pp_gauss_normal: %d parameter sets, 1..%d per call", nsets, GFIT_MAX_SETS);
    if (nrow < 1) return fail(PP_EINVAL, "pp_gauss_normal: %d samples per set", nrow);
    if (nsets > 1 && (!h || !g || !G)) return fail(PP_EINVAL, "pp_gauss_normal: null argument");
    if ((double)nsets * (double)nrow * 8.0 > kGaussFitMaxBytes)
        return fail(PP_EINVAL, "pp_gauss_normal: %d sets of %d residuals exceed %.0f bytes", nsets, nrow, kGaussFitMaxBytes);
    for (int a = 0; a + 1 < nsets; ++a)
        if (!(h[a] != 0.0) || std::isinf(h[a])) return fail(PP_EINVAL, "pp_gauss_normal: h[%d] = %g is no step", a, h[a]);
    pp_ctx::GaussFit& F = c->gfit;
    if (!R_or_null && (F.nsets != nsets || F.nrow != (long long)nrow))
        return fail(PP_ESTATE, "pp_gauss_normal: no resident residual rows of %d sets x %d samples (pp_gauss_residuals left %d x %lld)",
                    nsets, nrow, F.nsets, F.nrow);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const double* R = F.R.as<double>();
    if (R_or_null && on_device) R = R_or_null;
    else if (R_or_null) {
        // (the caller's rows take the resident rows' place)
        F.nsets = 0;
        if ((rc = upload(c, F.R, R_or_null, (size_t)nsets * nrow * 8))) return rc;
        R = F.R.as<double>();
        F.nsets = nsets; F.nrow = nrow;
    }
    const int NP = nsets * nsets;
    const int chunk = gauss_normal_chunk(nrow);
    const int nchunk = (int)(((long long)nrow + chunk - 1) / chunk);
    if ((rc = F.part.reserve((size_t)nchunk * NP * 8))) return rc;
    if ((rc = F.gram.reserve((size_t)NP * 8))) return rc;
    const double* dh = nullptr;
    if (nsets > 1) {
        if ((rc = upload(c, F.h, h, (size_t)(nsets - 1) * 8))) return rc;
        dh = F.h.as<double>();
    }
    {
        Prof pr(c, KF_GAUSSNORM);
        hipLaunchKernelGGL(k_gauss_normal_part, dim3(nchunk), dim3(GN_T), 0, c->stream, R, dh, nsets, (long long)nrow, chunk,
                           F.part.as<double>());
        hipLaunchKernelGGL(k_gauss_normal_sum, dim3((NP + 255) / 256), dim3(256), 0, c->stream,
                           (const double*)F.part.as<double>(), nchunk, nsets, F.gram.as<double>());
    }
    HIP_TRY(hipGetLastError());
    std::vector<double> full((size_t)NP);
    HIP_TRY(hipMemcpyAsync(full.data(), F.gram.p, (size_t)NP * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *chi2 = full[0];
    const int K = nsets - 1;
    for (int a = 0; a < K; ++a) {
        g[a] = full[(size_t)(a + 1)];
        for (int b = 0; b < K; ++b) G[(size_t)a * K + b] = full[(size_t)(a + 1) * nsets + b + 1];
    }
    return PP_OK;
}
