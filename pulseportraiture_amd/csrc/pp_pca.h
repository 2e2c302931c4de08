// ppspline on the device (included at the end of pp_toas.hip, after pp_zap.h): the weighted PCA of an
// aligned average portrait -- mean profile, centred rows, the Gram matrix of the smaller side on the f64
// MFMA, the leading eigenvectors mapped back to profiles with their significance statistics, the projection
// and the reconstruction (pplib.pca :1497-1534, find_significant_eigvec :1555-1619, reconstruct_portrait
// :1536-1553).  The symmetric eigenproblem of the small matrix is the host's (LAPACK, as in the reference).

namespace pp {

constexpr int PCA_CH = 32;        // channels per partial column sum
constexpr int PCA_TB = 64;        // Gram tile edge of a workgroup (4 waves, 32 x 32 each)
constexpr int PCA_KC = 16;        // reduction elements staged per step
constexpr int PCA_MAXVEC = 16;    // eigenvectors examined at most (the reference examines 10)

typedef double v4d __attribute__((ext_vector_type(4)));

// partial[chunk][j] = sum over the chunk's channels n (in order) of w[n] * (x[n][j] - centre[j])
template <typename Tin>
__global__ __launch_bounds__(64) void k_pca_colsum(const void* src, const double* w, const double* centre, int nchan,
                                                   int nbin, double* partial) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nbin) return;
    const Tin* x = reinterpret_cast<const Tin*>(src);
    const int n0 = blockIdx.y * PCA_CH, n1 = min(nchan, n0 + PCA_CH);
    const double c = centre ? centre[j] : 0.0;
    double s = 0.0;
    for (int n = n0; n < n1; ++n) s += w[n] * ((double)x[(size_t)n * nbin + j] - c);
    partial[(size_t)blockIdx.y * nbin + j] = s;
}

// out[j] = (sum of the chunks' partials, in order) / sumw
__global__ __launch_bounds__(64) void k_pca_colfinish(const double* partial, int nchunk, int nbin, double sumw, double* out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nbin) return;
    double s = 0.0;
    for (int q = 0; q < nchunk; ++q) s += partial[(size_t)q * nbin + j];
    out[j] = s / sumw;
}

// D[n][j] = x[n][j] - mean[j] (the reference's delta_port) and S = sqrt(w[n]) (D[n][j] - avg[j]) (np.cov's
// re-centred rows, scaled): S[n][j] with pitch `pitch` for the dual side (reduction over bins), S[j][n] for
// the primal side (reduction over channels)
template <typename Tin>
__global__ __launch_bounds__(64) void k_pca_centre(const void* src, const double* w, const double* mean, const double* avg,
                                                   int nchan, int nbin, int dual, int pitch, double* D, double* S) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nbin) return;
    const Tin* x = reinterpret_cast<const Tin*>(src);
    const int n0 = blockIdx.y * PCA_CH, n1 = min(nchan, n0 + PCA_CH);
    const double m = mean[j], a = avg[j];
    for (int n = n0; n < n1; ++n) {
        const double d = (double)x[(size_t)n * nbin + j] - m;
        D[(size_t)n * nbin + j] = d;
        const double s = sqrt(w[n]) * (d - a);
        if (dual) S[(size_t)n * pitch + j] = s;
        else S[(size_t)j * pitch + n] = s;
    }
}

// G = scale * A A^T for A[npad][mpad] (zero padded: npad a multiple of 64, mpad of 16), f64 throughout, on
// v_mfma_f64_16x16x4_f64.  One workgroup per 64 x 64 tile of the upper triangle (tile row <= tile column), four
// waves of 2 x 2 MFMA tiles each; both operand panels go through LDS PCA_KC reduction elements at a time.  The
// reduction runs in one fixed order and nothing is accumulated atomically: the same input gives the same bits.
// Tiles off the diagonal are stored twice, as computed and mirrored.
// (operands, lane l: A[row l & 15][k l >> 4], B[k l >> 4][col l & 15]; result register r: row (l >> 4) + 4 r,
// column l & 15)
__global__ __launch_bounds__(256) void k_pca_gram(const double* A, int npad, int mpad, int n, double scale, double* G) {
    __shared__ double sa[PCA_TB][PCA_KC + 1], sb[PCA_TB][PCA_KC + 1];
    const int nb = npad / PCA_TB;
    int t = blockIdx.x, bi = 0;
    while (t >= nb - bi) { t -= nb - bi; ++bi; }
    const int bj = bi + t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int lr = tid >> 2, lc = (tid & 3) * 4;
    const double* pa = A + (size_t)(bi * PCA_TB + lr) * mpad + lc;
    const double* pb = A + (size_t)(bj * PCA_TB + lr) * mpad + lc;
    v4d acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int r16 = lane & 15, k4 = lane >> 4;
    for (int k0 = 0; k0 < mpad; k0 += PCA_KC) {
        const double2 a0 = *reinterpret_cast<const double2*>(pa + k0), a1 = *reinterpret_cast<const double2*>(pa + k0 + 2);
        const double2 b0 = *reinterpret_cast<const double2*>(pb + k0), b1 = *reinterpret_cast<const double2*>(pb + k0 + 2);
        sa[lr][lc] = a0.x; sa[lr][lc + 1] = a0.y; sa[lr][lc + 2] = a1.x; sa[lr][lc + 3] = a1.y;
        sb[lr][lc] = b0.x; sb[lr][lc + 1] = b0.y; sb[lr][lc + 2] = b1.x; sb[lr][lc + 3] = b1.y;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PCA_KC; kk += 4) {
            const double fa0 = sa[wr + r16][kk + k4], fa1 = sa[wr + 16 + r16][kk + k4];
            const double fb0 = sb[wc + r16][kk + k4], fb1 = sb[wc + 16 + r16][kk + k4];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bi * PCA_TB + wr + 16 * i + k4 + 4 * r, col = bj * PCA_TB + wc + 16 * j + r16;
                if (row < n && col < n) {
                    const double v = acc[i][j][r] * scale;
                    G[(size_t)row * n + col] = v;
                    if (bi != bj) G[(size_t)col * n + row] = v;
                }
            }
}

// the dual side's eigenvectors as profiles: B[v][j] = sum_n S[n][j] u_v[n] / sqrt(lam_v fact)  (S = sqrt(w) times
// the centred rows, G = S S^T / fact, G u = lam u: unit length in exact arithmetic; k_pca_unit makes it so); an
// eigenvalue that is not positive gives a zero row
__global__ __launch_bounds__(64) void k_pca_backproject(const double* S, int pitch, int nchan, int nbin, const double* U,
                                                        const double* lam, int nvec, double fact, double* B) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nbin) return;
    double s[PCA_MAXVEC];
#pragma unroll
    for (int v = 0; v < PCA_MAXVEC; ++v) s[v] = 0.0;
    for (int n = 0; n < nchan; ++n) {
        const double x = S[(size_t)n * pitch + j];
#pragma unroll
        for (int v = 0; v < PCA_MAXVEC; ++v)
            if (v < nvec) s[v] = fma(x, U[(size_t)v * nchan + n], s[v]);
    }
#pragma unroll
    for (int v = 0; v < PCA_MAXVEC; ++v)
        if (v < nvec) B[(size_t)v * nbin + j] = lam[v] > 0.0 ? s[v] / sqrt(lam[v] * fact) : 0.0;
}

constexpr int PCA_ST = 256;

// workgroup total of one value per thread, on every thread (fixed order)
__device__ __forceinline__ double pca_block_sum(double* red, double v) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int q = 0; q < PCA_ST / 64; ++q) t += red[q];
    __syncthreads();
    return t;
}

// A back-projected vector scaled to unit length, one workgroup per vector.  Its length is sqrt(lam_exact / lam): the
// computed eigenvalue carries an absolute error of rounding x the LARGEST eigenvalue, which is a relative 1e-11 of
// a noise eigenvalue 1e5 times smaller, and the vector's power (find_significant_eigvec's signal) would carry
// it; LAPACK's eigenvectors of the covariance, the reference's, have unit length to rounding.
__global__ __launch_bounds__(PCA_ST) void k_pca_unit(double* B, int nbin) {
    __shared__ double red[PCA_ST / 64];
    double* b = B + (size_t)blockIdx.x * nbin;
    double s = 0.0;
    for (int j = threadIdx.x; j < nbin; j += PCA_ST) s = fma(b[j], b[j], s);
    s = pca_block_sum(red, s);
    if (!(s > 0.0)) return;
    const double len = sqrt(s);
    for (int j = threadIdx.x; j < nbin; j += PCA_ST) b[j] /= len;
}

// find_significant_eigvec's numbers of one basis vector per workgroup (pplib.py:1586-1595, no smoothing), from the
// vector and its harmonics H[0..M]: stats[v] = {sum_{k>=1} |H_k|^2, get_noise_PS(ev) (:2249-2253),
// max |ev|, count_crossings(|ev|, 0.1 max |ev|) (:686-694)}
__global__ __launch_bounds__(PCA_ST) void k_pca_stats(const double* B, const cplx* H, int nbin, double* stats) {
    __shared__ double red[PCA_ST / 64];
    const int v = blockIdx.x, tid = threadIdx.x, M = nbin / 2, kc = (int)(0.75 * (M + 1));
    const double* ev = B + (size_t)v * nbin;
    const cplx* h = H + (size_t)v * (M + 1);
    double pw = 0.0, top = 0.0, mx = 0.0;
    for (int k = 1 + tid; k <= M; k += PCA_ST) {
        const double p = cnorm(h[k]);
        pw += p;
        if (k >= kc) top += p;
    }
    for (int j = tid; j < nbin; j += PCA_ST) mx = fmax(mx, fabs(ev[j]));
    pw = pca_block_sum(red, pw);
    top = pca_block_sum(red, top);
    mx = group_max<64>(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    const double x0 = 0.1 * mx;
    auto sgn = [](double d) { return d > 0.0 ? 1 : (d < 0.0 ? -1 : 0); };
    double changes = 0.0, zeros = 0.0;
    for (int j = tid; j < nbin; j += PCA_ST) {
        const int s = sgn(fabs(ev[j]) - x0);
        if (s == 0) zeros += 1.0;
        if (j + 1 < nbin && sgn(fabs(ev[j + 1]) - x0) != s) changes += 1.0;
    }
    changes = pca_block_sum(red, changes);
    zeros = pca_block_sum(red, zeros);
    if (tid == 0) {
        stats[4 * v] = pw;
        stats[4 * v + 1] = sqrt(top / (double)nbin / (double)(M + 1 - kc));
        stats[4 * v + 2] = mx;
        stats[4 * v + 3] = changes - zeros;
    }
}

// one workgroup per channel: proj[n][c] = sum_j D[n][j] B[ieig[c]][j], then reconst[n][j] = sum_c proj[n][c]
// B[ieig[c]][j] + mean[j]  (ppspline.py:126-129)
__global__ __launch_bounds__(PCA_ST) void k_pca_project(const double* D, const double* B, const double* mean, const int* ieig,
                                                        int ncomp, int nbin, double* proj, double* reconst) {
    __shared__ double red[PCA_ST / 64];
    __shared__ double pr[PCA_MAXVEC];
    const int n = blockIdx.x, tid = threadIdx.x;
    const double* d = D + (size_t)n * nbin;
    for (int c = 0; c < ncomp; ++c) {
        const double* b = B + (size_t)ieig[c] * nbin;
        double s = 0.0;
        for (int j = tid; j < nbin; j += PCA_ST) s = fma(d[j], b[j], s);
        s = pca_block_sum(red, s);
        if (tid == 0) { pr[c] = s; proj[(size_t)n * ncomp + c] = s; }
    }
    __syncthreads();
    for (int j = tid; j < nbin; j += PCA_ST) {
        double s = 0.0;
        for (int c = 0; c < ncomp; ++c) s = fma(pr[c], B[(size_t)ieig[c] * nbin + j], s);
        reconst[(size_t)n * nbin + j] = s + mean[j];
    }
}

}  // namespace pp

// ---- ppspline: mean profile, centred rows and the Gram matrix of the smaller side ------------
// pplib.pca (pplib.py:1497-1528) up to the covariance: mean_prof = sum_n w_n port_n / sumw (ppspline.py:70),
// delta = port - mean_prof, np.cov(delta.T, aweights=w, ddof=1): rows re-centred by their weighted average,
// normalised by fact = sumw - sum w^2 / sumw.
extern "C" int pp_pca_gram(pp_ctx* c, const void* src, int dtype, int on_device, int nchan, int nbin, const double* w,
                           double sumw, double fact, double* mean_prof, double* gram) {
    if (int busy_ = ctx_busy(c, "pp_pca_gram")) return busy_;
    if (!c || !src || !w || !mean_prof || !gram) return fail(PP_EINVAL, "pp_pca_gram: null argument");
    if (!nbin_any_ok(nbin) || nbin > 4096) return fail(PP_EINVAL, "pp_pca_gram: nbin %d must be even and in [8, 4096]", nbin);
    if (nchan < 2 || nchan > 65536) return fail(PP_EINVAL, "pp_pca_gram: %d channels (2 ... 65536)", nchan);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_pca_gram: dtype %d", dtype);
    if (!(sumw > 0.0) || !(fact > 0.0)) return fail(PP_EINVAL, "pp_pca_gram: weights sum %g, normalisation %g", sumw, fact);
    HIP_TRY(hipSetDevice(c->device));
    pp_ctx::Pca& p = c->pca;
    p.nchan = p.nbin = 0;
    const size_t esz = dtype == PP_F64 ? 8 : 4, np_ = (size_t)nchan * nbin;
    const int dual = nchan < nbin ? 1 : 0;
    const int n = dual ? nchan : nbin, m = dual ? nbin : nchan;
    const int npad = (n + PCA_TB - 1) / PCA_TB * PCA_TB, mpad = (m + PCA_KC - 1) / PCA_KC * PCA_KC;
    const int nchunk = (nchan + PCA_CH - 1) / PCA_CH;
    int rc;
    const void* dsrc = src;
    if (!on_device) {
        if ((rc = upload(c, c->data, src, np_ * esz))) return rc;
        dsrc = c->data.p;
    }
    if ((rc = upload(c, p.w, w, (size_t)nchan * 8))) return rc;
    if ((rc = p.vec.reserve((size_t)2 * nbin * 8))) return rc;
    if ((rc = p.part.reserve((size_t)nchunk * nbin * 8))) return rc;
    if ((rc = p.D.reserve(np_ * 8))) return rc;
    if ((rc = p.S.reserve((size_t)npad * mpad * 8))) return rc;
    if ((rc = p.G.reserve((size_t)n * n * 8))) return rc;
    double *mean = p.vec.as<double>(), *avg = mean + nbin;
    HIP_TRY(hipMemsetAsync(p.S.p, 0, (size_t)npad * mpad * 8, c->stream));
    const dim3 grid((nbin + 63) / 64, nchunk);
    const double* dw = p.w.as<double>();
    with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_pca_colsum<T>, grid, dim3(64), 0, c->stream, dsrc, dw, (const double*)nullptr, nchan, nbin, p.part.as<double>());
        hipLaunchKernelGGL(k_pca_colfinish, dim3(grid.x), dim3(64), 0, c->stream, p.part.as<double>(), nchunk, nbin, sumw, mean);
        hipLaunchKernelGGL(k_pca_colsum<T>, grid, dim3(64), 0, c->stream, dsrc, dw, (const double*)mean, nchan, nbin, p.part.as<double>());
        hipLaunchKernelGGL(k_pca_colfinish, dim3(grid.x), dim3(64), 0, c->stream, p.part.as<double>(), nchunk, nbin, sumw, avg);
        hipLaunchKernelGGL(k_pca_centre<T>, grid, dim3(64), 0, c->stream, dsrc, dw, (const double*)mean, (const double*)avg, nchan, nbin, dual, mpad,
                           p.D.as<double>(), p.S.as<double>());
    });
    const int nb = npad / PCA_TB;
    {
        Prof pf(c, KF_PCA);
        hipLaunchKernelGGL(k_pca_gram, dim3(nb * (nb + 1) / 2), dim3(256), 0, c->stream, p.S.as<double>(), npad, mpad, n,
                           1.0 / fact, p.G.as<double>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mean_prof, mean, (size_t)nbin * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(gram, p.G.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    p.nchan = nchan; p.nbin = nbin; p.dual = dual; p.pitch = mpad; p.fact = fact; p.nvec = 0;
    return PP_OK;
}

// ---- ppspline: the leading eigenvectors as profiles, and their significance statistics -------
// vecs[nvec][n]: the host's leading eigenvectors of pp_pca_gram's matrix (rows; n = its order), lam[nvec] their
// eigenvalues.  basis[nvec][nbin]: the eigenvectors of the covariance (dual side: mapped back through the
// centred rows).  stats[nvec][4]: what find_significant_eigvec (pplib.py:1586-1595) measures of each.
extern "C" int pp_pca_basis(pp_ctx* c, const double* vecs, const double* lam, int nvec, double* basis, double* stats) {
    if (int busy_ = ctx_busy(c, "pp_pca_basis")) return busy_;
    if (!c || !vecs || !lam || !basis || !stats) return fail(PP_EINVAL, "pp_pca_basis: null argument");
    pp_ctx::Pca& p = c->pca;
    if (!p.nchan) return fail(PP_ESTATE, "pp_pca_basis: no centred portrait is resident (pp_pca_gram first)");
    const int n = p.dual ? p.nchan : p.nbin, nbin = p.nbin, M = nbin / 2;
    if (nvec < 1 || nvec > PCA_MAXVEC || nvec > n) return fail(PP_EINVAL, "pp_pca_basis: %d eigenvectors (1 ... %d)", nvec, std::min(PCA_MAXVEC, n));
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = p.B.reserve((size_t)PCA_MAXVEC * nbin * 8))) return rc;
    if ((rc = p.small.reserve((size_t)PCA_MAXVEC * 8 * 8))) return rc;
    double *dlam = p.small.as<double>(), *dstats = dlam + PCA_MAXVEC;
    if (p.dual) {
        if ((rc = upload(c, p.U, vecs, (size_t)nvec * n * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(dlam, lam, (size_t)nvec * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_pca_backproject, dim3((nbin + 63) / 64), dim3(64), 0, c->stream, p.S.as<double>(), p.pitch,
                           p.nchan, nbin, p.U.as<double>(), dlam, nvec, p.fact, p.B.as<double>());
        hipLaunchKernelGGL(k_pca_unit, dim3(nvec), dim3(PCA_ST), 0, c->stream, p.B.as<double>(), nbin);
    } else {
        HIP_TRY(hipMemcpyAsync(p.B.p, vecs, (size_t)nvec * nbin * 8, hipMemcpyHostToDevice, c->stream));
    }
    // the vectors' harmonics, by the row transform of the fit
    if ((rc = c->X.reserve((size_t)nvec * (M + 1) * sizeof(cplx)))) return rc;
    if ((rc = rows_harmonics(c, p.B.p, PP_F64, nvec, nbin, c->X.as<cplx>()))) return rc;
    hipLaunchKernelGGL(k_pca_stats, dim3(nvec), dim3(PCA_ST), 0, c->stream, p.B.as<double>(), c->X.as<cplx>(), nbin, dstats);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(basis, p.B.p, (size_t)nvec * nbin * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stats, dstats, (size_t)nvec * 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    p.nvec = nvec;
    return PP_OK;
}

// ---- ppspline: projection onto the chosen eigenvectors and the reconstruction ----------------
// proj[nchan][ncomp] = delta . basis[ieig] and reconst[nchan][nbin] = proj . basis[ieig]^T + mean_prof
// (ppspline.py:119-129, reconstruct_portrait pplib.py:1536-1553) of the resident rows and basis
extern "C" int pp_pca_project(pp_ctx* c, const int32_t* ieig, int ncomp, double* proj, double* reconst) {
    if (int busy_ = ctx_busy(c, "pp_pca_project")) return busy_;
    if (!c || !ieig || !proj || !reconst) return fail(PP_EINVAL, "pp_pca_project: null argument");
    pp_ctx::Pca& p = c->pca;
    if (!p.nchan || !p.nvec) return fail(PP_ESTATE, "pp_pca_project: no basis is resident (pp_pca_gram, pp_pca_basis first)");
    if (ncomp < 1 || ncomp > p.nvec) return fail(PP_EINVAL, "pp_pca_project: %d components of %d", ncomp, p.nvec);
    for (int q = 0; q < ncomp; ++q)
        if (ieig[q] < 0 || ieig[q] >= p.nvec) return fail(PP_EINVAL, "pp_pca_project: eigenvector %d of %d", (int)ieig[q], p.nvec);
    HIP_TRY(hipSetDevice(c->device));
    const size_t np_ = (size_t)p.nchan * p.nbin;
    int rc;
    if ((rc = upload(c, p.idx, ieig, (size_t)ncomp * 4))) return rc;
    if ((rc = p.proj.reserve((size_t)p.nchan * ncomp * 8))) return rc;
    if ((rc = c->data.reserve(np_ * 8))) return rc;       // (the uploaded portrait is no longer needed: D holds the rows)
    hipLaunchKernelGGL(k_pca_project, dim3(p.nchan), dim3(PCA_ST), 0, c->stream, p.D.as<double>(), p.B.as<double>(),
                       p.vec.as<double>(), p.idx.as<int>(), ncomp, p.nbin, p.proj.as<double>(), c->data.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(proj, p.proj.p, (size_t)p.nchan * ncomp * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(reconst, c->data.p, np_ * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}
