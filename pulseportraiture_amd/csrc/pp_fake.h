// Simulated observations on the device (make_fake_pulsar, pplib.py:3183-3378): the general form of the synthetic
// generator of pp_extra.h.  Where k_synth takes one delay law and one noise level, the rows here take a table of delays
// [nsub][nchan] (rotations, every law the host can write down), amplitudes per (subint, polarisation, channel) and a
// noise level per channel:
//   dst[i][p][n][:] = amps[i][p][n] irfft_k(m[n][k] e^{-2 pi i k delays[i][n]}) + sigmas[n] z(seed, first_subint + i, p, n, bin)
// The model is the same in every polarisation (pplib.py:3375 "same model, same noise_stds"): one workgroup owns a
// (subint, channel) pair, forms the rotated harmonics and takes the inverse transform ONCE, and writes the npol rows from
// the row it keeps in LDS -- each with its own amplitude and its own noise.  Included at the end of pp_toas.hip.
#pragma once

namespace pp {

struct FakeArgs {
    const cplx* mft;        // [nchan][M or Mp] harmonics 1..M of the model slot
    const double* mdc;      // [nchan] DC harmonic (real)
    void* dst;              // [nsub][npol][nchan][B]
    const double* delays;   // [nsub][nchan] rotations, positive = later
    const double* amps;     // [nsub][npol][nchan], or nullptr = 1
    const double* sigmas;   // [nchan], or nullptr = 0
    const cplx* twB;
    uint64_t seed;
    int64_t first_subint;
    int nsub, npol, nchan;
};

// the polarisation goes into the counter word of the bin pair, above the 12 bits a pair of an 8192-bin row takes: no
// two of (seed, subint, polarisation, channel, bin pair) share a Philox stream (npol <= PP_FAKE_MAX_NPOL)
#define PP_FAKE_POL_SHIFT 16
#define PP_FAKE_MAX_NPOL 65536

// The npol output rows of (subint i, channel n) from the noise-free row held in LDS: row(j) is the packed pair
// (x_2j, -x_2j+1) M, as the inverse transforms leave it.  Values are formed in f64 and cast on the store, so the f32 rows
// are the rounded f64 rows; sigma == 0 adds nothing (no 0 * z), and amp == 0 leaves sigma z exactly (one fma).
template <typename Tout, typename Row>
__device__ __forceinline__ void fake_write_rows(const FakeArgs& a, int i, int n, int M, int T, int tid, Row row) {
    const double sg = a.sigmas ? a.sigmas[n] : 0.0;
    const double invM = 1.0 / (double)M;
    const int64_t sub = a.first_subint + i;
    for (int p = 0; p < a.npol; ++p) {
        const size_t orow = ((size_t)i * a.npol + p) * a.nchan + n;
        const double amp = a.amps ? a.amps[orow] : 1.0;
        Tout* out = reinterpret_cast<Tout*>(a.dst) + orow * (size_t)(2 * M);
        for (int j = tid; j < M; j += T) {
            const cplx r = row(j);
            const double v0 = r.x * invM, v1 = -r.y * invM;
            double x0, x1;
            if (sg != 0.0) {
                double z0, z1;
                normal_pair(a.seed, sub, n, j | (p << PP_FAKE_POL_SHIFT), z0, z1);
                const double n0 = sg * z0, n1 = sg * z1;
                x0 = fma(amp, v0, n0);
                x1 = fma(amp, v1, n1);
            } else {
                x0 = amp * v0;
                x1 = amp * v1;
            }
            if (sizeof(Tout) == 8) reinterpret_cast<double2*>(out)[j] = make_double2(x0, x1);
            else reinterpret_cast<float2*>(out)[j] = make_float2((float)x0, (float)x1);
        }
    }
}

// row lengths with a tuned plan
template <int M, typename Tout>
__global__ __launch_bounds__(FftPlan<M>::T) void k_fake(FakeArgs a) {
    constexpr int T = FftPlan<M>::T;
    constexpr int PL = FftPlan<M>::PADLOG;
    __shared__ cplx lds[FftPlan<M>::LDS_ELEMS];
    __shared__ cplx zin[M];
    const int tid = threadIdx.x;
    const long long nrows = (long long)a.nsub * a.nchan;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int i = (int)(row / a.nchan), n = (int)(row % a.nchan);
        const double phin = -a.delays[row];
        const cplx* mrow = a.mft + (size_t)n * M;
        const double yM = cmul(mrow[M - 1], unit_phasor((double)M, phin)).x;   // Nyquist: real part
        for (int k = tid; k < M; k += T) {
            cplx yk, ym;
            if (k == 0) { yk = make_double2(a.mdc[n], 0.0); ym = make_double2(yM, 0.0); }
            else {
                yk = cmul(mrow[k - 1], unit_phasor((double)k, phin));
                ym = cmul(mrow[M - k - 1], unit_phasor((double)(M - k), phin));
            }
            zin[k] = irfft_pack(yk, ym, a.twB[k]);
        }
        __syncthreads();
        fft_row<M, cplx>(lds, zin, a.twB, tid);
        fake_write_rows<Tout>(a, i, n, M, T, tid, [&](int j) { return lds[lds_pad<PL>(j)]; });
        __syncthreads();
    }
}

// every other even row length: the rotated harmonics back by the chirp-z route (pp_anybin.h); the slot's spectrum rows
// are pitched to Mp
template <int L, typename Tout>
__global__ __launch_bounds__(FftPlan<L>::T) void k_fake_any(FakeArgs a, AnyArgs g) {
    constexpr int T = FftPlan<L>::T;
    __shared__ cplx lds[FftPlan<L>::LDS_ELEMS];
    __shared__ cplx buf[L];
    const int tid = threadIdx.x;
    const int M = g.M;
    const long long nrows = (long long)a.nsub * a.nchan;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int i = (int)(row / a.nchan), n = (int)(row % a.nchan);
        const double phin = -a.delays[row];
        const cplx* mrow = a.mft + (size_t)n * g.Mp;
        const double yM = cmul(mrow[M - 1], unit_phasor((double)M, phin)).x;   // Nyquist: real part
        for (int k = tid; k < M; k += T) {
            cplx yk, ym;
            if (k == 0) { yk = make_double2(a.mdc[n], 0.0); ym = make_double2(yM, 0.0); }
            else {
                yk = cmul(mrow[k - 1], unit_phasor((double)k, phin));
                ym = cmul(mrow[M - k - 1], unit_phasor((double)(M - k), phin));
            }
            buf[k] = irfft_pack(yk, ym, g.twB[k]);
        }
        __syncthreads();
        czt_any<L>(buf, lds, g, tid);
        fake_write_rows<Tout>(a, i, n, M, T, tid, [&](int j) { return buf[j]; });
        __syncthreads();
    }
}

}  // namespace pp

// ---- host ------------------------------------------------------------------
extern "C" int pp_fake_portraits(pp_ctx* c, int slot, void* dst, int dtype, int nsub, int npol, const double* delays,
                                 const double* amps, const double* sigmas, uint64_t seed, int64_t first_subint) {
    if (int busy_ = ctx_busy(c, "pp_fake_portraits")) return busy_;
    if (!c || !dst || !delays) return fail(PP_EINVAL, "pp_fake_portraits: null argument");
    if (slot < 0 || slot >= PP_MAX_SLOTS || !c->slots[slot].set) return fail(PP_ESTATE, "pp_fake_portraits: slot %d not set", slot);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_fake_portraits: dtype %d", dtype);
    if (nsub < 1 || npol < 1 || npol > PP_FAKE_MAX_NPOL) return fail(PP_EINVAL, "pp_fake_portraits: bad shape %d x %d", nsub, npol);
    ModelSlot& s = c->slots[slot];
    const int C = s.nchan, B = s.nbin, M = B / 2;
    const size_t nrows = (size_t)nsub * C;
    for (size_t j = 0; j < nrows; ++j)
        if (!std::isfinite(delays[j])) return fail(PP_EINVAL, "pp_fake_portraits: delays[%zu][%zu] is not finite", j / C, j % C);
    if (sigmas)
        for (int n = 0; n < C; ++n)
            if (!(sigmas[n] >= 0.0) || std::isinf(sigmas[n])) return fail(PP_EINVAL, "pp_fake_portraits: sigmas[%d] = %g", n, sigmas[n]);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = upload(c, c->x0, delays, nrows * 8))) return rc;
    if (amps) if ((rc = upload(c, c->wts, amps, nrows * npol * 8))) return rc;
    if (sigmas) if ((rc = upload(c, c->errs, sigmas, (size_t)C * 8))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, B, &tw))) return rc;
    FakeArgs a{s.mft.as<cplx>(), s.mdc.as<double>(), dst, c->x0.as<double>(), amps ? c->wts.as<double>() : (const double*)nullptr,
               sigmas ? c->errs.as<double>() : (const double*)nullptr, tw, seed, first_subint, nsub, npol, C};
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(B)) {
            AnyArgs g;
            int L = 0;
            if ((rc = any_args(c, B, &g, &L))) return rc;
            if ((rc = with_any_len(L, [&](auto LL) {
                    with_dtype(dtype, [&](auto t) { hipLaunchKernelGGL((k_fake_any<decltype(LL)::value, decltype(t)>), dim3(any_grid((long long)nrows)), dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, a, g); });
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(dtype, [&](auto t) { hipLaunchKernelGGL((k_fake<MM, decltype(t)>), dim3(fft_grid(T, (long long)nrows)), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}
