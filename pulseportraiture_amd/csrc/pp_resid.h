// Fit residuals: the data minus the fitted model, row by row (included at the end of pp_toas.hip).
//
// What GetTOAs.show_fit(..., return_fit=True) returns in the reference (pptoas.py:1317-1419): the subint rotated by
// the fitted (phi, DM, GM) onto the template, and the template scattered by the fitted (tau, alpha) and multiplied by
// the fitted amplitudes -- and their difference.  For row (i, n), with phi_n and tau_n exactly as k_chan_chi2 forms
// them and B_k = 1 / (1 + 2 pi i k tau_n), harmonics k = 0..M:
//     frame 0 ("model", show_fit's):  D_k = d_k e^{2 pi i k phi_n},   Mo_k = a_n B_k m_k
//     frame 1 ("data"):               D_k = d_k,                      Mo_k = a_n B_k m_k e^{-2 pi i k phi_n}
// m_0 is the slot's stored DC, DC is not rotated, the Nyquist harmonic keeps its real part (irfft).
// port = irfft(D), model = irfft(Mo), resid = irfft(D - Mo); every output is optional (null = not formed).
//
// One body serves every choice of outputs, the wanted ones picked by workgroup-uniform branches: what two calls share
// they compute with the same instructions, so its bits do not depend on what else was asked for.  The row's forward
// transform and the packed spectrum of one inverse are the two LDS images k_rotate holds (139 KB at 8192 bins: one
// workgroup per CU there, as for k_rotate); the packed spectrum is linear in the harmonics, so
//     zin = pack(D)            -> inverse -> port      (zin is only read by the transform)
//     zin = zin - pack(Mo)     -> inverse -> resid     (ONE inverse, not the difference of two)
//     zin = pack(Mo)           -> inverse -> model
// needs no third image; pack(Mo) comes from the slot's spectrum in global memory (L2) and is formed again for the
// model rather than kept.  A row costs at most three inverse transforms, one when only resid is wanted.
//
// red_chi2 is k_chan_chi2's sum, term for term and with its phasor (unit_phasor), taken from the forward transform
// before the image is reused: |D - Mo| is the same in both frames, so the figure does not depend on `frame` and
// agrees with pp_channel_red_chi2.  The rows themselves use turn_phasor (exact k phi), as k_rotate does.
namespace pp {

struct ResidArgs {
    ChanChi2Args c;        // src, slots, freqs, P, par, nuref, scales, errs (null without out), twB, out = red_chi2 (or null)
    const double* mask;    // [nsub][nchan] weights: 0 or NaN = the row is not read, zeros out, chi^2 NaN; null = all live
    void *port, *model, *resid;   // [nsub][nchan][B] of the input's type, each may be null
    int frame;             // 0 model, 1 data
};

// phi_n, tau_n, the slot's row and the amplitude of row (i, n): k_chan_chi2's expressions
struct ResidRow {
    double phin, taun, m0, sc;
    const cplx* mrow;
};
__device__ __forceinline__ ResidRow resid_row(const ChanChi2Args& a, int i, int n, int pitch) {
    const double nu = a.freqs[(size_t)i * a.freqs_stride + n], P = a.P[i];
    const double* pr = a.par + (size_t)i * 5;
    const double nuDM = a.nuref[i * 3], nuGM = a.nuref[i * 3 + 1], nutau = a.nuref[i * 3 + 2];
    const double a2 = 1.0 / (nu * nu);
    const double iDM = (nuDM == INFINITY) ? 0.0 : 1.0 / (nuDM * nuDM);
    const double iGM = (nuGM == INFINITY) ? 0.0 : 1.0 / (nuGM * nuGM * nuGM * nuGM);
    ResidRow r;
    r.phin = pr[0] + PP_DCONST * pr[1] * (a2 - iDM) / P + PP_DCONST * PP_DCONST * pr[2] * (a2 * a2 - iGM) / P;
    r.taun = (pr[3] != 0.0) ? pr[3] * pow(nu / nutau, pr[4]) : 0.0;
    const int sl = a.slot ? a.slot[i] : 0;
    r.mrow = as_global(a.mft[sl]) + (size_t)n * pitch;
    r.m0 = as_global(a.mdc[sl])[n];
    r.sc = a.scales[(size_t)i * a.nchan + n];
    return r;
}
__device__ __forceinline__ bool resid_live(const double* mask, size_t row) {
    if (!mask) return true;
    const double w = mask[row];
    return w != 0.0 && w == w;
}
// Mo_k, k = 1..M (the caller keeps the real part at k = M)
__device__ __forceinline__ cplx resid_model_harm(const ResidRow& r, int frame, int k) {
    cplx m = r.mrow[k - 1];
    if (r.taun != 0.0) {
        const double x = PP_TWO_PI * (double)k * r.taun, den = 1.0 / (1.0 + x * x);
        m = cmul(m, make_double2(den, -x * den));
    }
    if (frame == 1) m = cmul(m, turn_phasor((double)k, -r.phin));
    return make_double2(r.sc * m.x, r.sc * m.y);
}

template <typename Tio>
__device__ __forceinline__ void resid_store(void* dst, size_t row, int M, int j, double x0, double x1) {
    Tio* out = reinterpret_cast<Tio*>(dst) + row * (size_t)(2 * M);
    if (sizeof(Tio) == 8) reinterpret_cast<double2*>(out)[j] = make_double2(x0, x1);
    else reinterpret_cast<float2*>(out)[j] = make_float2((float)x0, (float)x1);
}

template <int M, typename Tio>
__global__ __launch_bounds__(FftPlan<M>::T) void k_resid(ResidArgs g) {
    constexpr int T = FftPlan<M>::T;
    constexpr int PL = FftPlan<M>::PADLOG;
    __shared__ cplx lds[FftPlan<M>::LDS_ELEMS];
    __shared__ cplx zin[M];
    __shared__ double scratch[(T / 64) + 1];
    const ChanChi2Args& a = g.c;
    const int tid = threadIdx.x;
    const long long nrows = (long long)a.nsub * a.nchan;
    const double inv = 1.0 / (double)M;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int i = (int)(row / a.nchan), n = (int)(row % a.nchan);
        if (!resid_live(g.mask, (size_t)row)) {          // (uniform over the workgroup; the data row is not read)
            for (int j = tid; j < M; j += T) {
                if (g.port) resid_store<Tio>(g.port, (size_t)row, M, j, 0.0, 0.0);
                if (g.model) resid_store<Tio>(g.model, (size_t)row, M, j, 0.0, 0.0);
                if (g.resid) resid_store<Tio>(g.resid, (size_t)row, M, j, 0.0, 0.0);
            }
            if (a.out && tid == 0) a.out[row] = NAN;
            continue;
        }
        const ResidRow rw = resid_row(a, i, n, M);
        const double phin = rw.phin, taun = rw.taun, sc = rw.sc, m0 = rw.m0;
        const cplx* mrow = rw.mrow;
        auto pack_model = [&](int k) -> cplx {
            if (k == 0) return irfft_pack(make_double2(sc * m0, 0.0), make_double2(resid_model_harm(rw, g.frame, M).x, 0.0), a.twB[0]);
            return irfft_pack(resid_model_harm(rw, g.frame, k), resid_model_harm(rw, g.frame, M - k), a.twB[k]);
        };
        if (g.port || g.resid || a.out) {
            fft_row<M, Tio>(lds, reinterpret_cast<const Tio*>(a.src) + (size_t)row * (2 * M), a.twB, tid);
            const cplx z0 = lds[0];
            if (a.out) {
                // k_chan_chi2's sum, as written there
                const double sg = a.errs[(size_t)i * a.nchan + n];
                double sum = 0.0;
                for (int k = tid; k <= M; k += T) {
                    double wgt = 2.0;
                    cplx d, m;
                    if (k == 0) { d = make_double2(z0.x + z0.y, 0.0); m = make_double2(m0, 0.0); wgt = 1.0; }
                    else {
                        d = (k == M) ? make_double2(z0.x - z0.y, 0.0) : rfft_harmonic<M>(lds, a.twB, k);
                        d = cmul(d, unit_phasor((double)k, phin));
                        m = mrow[k - 1];
                        if (taun != 0.0) {
                            // B_k = 1 / (1 + 2 pi i k tau_n)
                            const double x = PP_TWO_PI * (double)k * taun, den = 1.0 / (1.0 + x * x);
                            m = cmul(m, make_double2(den, -x * den));
                        }
                    }
                    cplx rr = make_double2(d.x - sc * m.x, d.y - sc * m.y);
                    if (k == M) { rr.y = 0.0; wgt = 1.0; }     // irfft drops the imaginary part at Nyquist
                    sum = fma(wgt, cnorm(rr), sum);
                }
                sum = group_sum<64>(sum);
                if ((tid & 63) == 0) scratch[tid >> 6] = sum;
                __syncthreads();
                if (tid == 0) {
                    double tot = 0.0;
                    for (int wv = 0; wv < T / 64; ++wv) tot += scratch[wv];
                    a.out[row] = tot / (2.0 * M) / (sg * sg) / (double)(2 * M - 2);
                }
                __syncthreads();
            }
            if (g.port || g.resid) {
                // pack(D): k_rotate's rotated harmonics in frame 0, the harmonics themselves in frame 1
                const double y0 = z0.x + z0.y;
                double yM = z0.x - z0.y;
                if (g.frame == 0) yM *= turn_phasor((double)M, phin).x;
                for (int k = tid; k < M; k += T) {
                    cplx yk, ym;
                    if (k == 0) { yk = make_double2(y0, 0.0); ym = make_double2(yM, 0.0); }
                    else {
                        yk = rfft_harmonic<M>(lds, a.twB, k);
                        ym = rfft_harmonic<M>(lds, a.twB, M - k);
                        if (g.frame == 0) {
                            yk = cmul(yk, turn_phasor((double)k, phin));
                            ym = cmul(ym, turn_phasor((double)(M - k), phin));
                        }
                    }
                    zin[k] = irfft_pack(yk, ym, a.twB[k]);
                }
            }
        }
        // the wanted rows in turn through the ONE inverse below: port from pack(D) as it stands; resid from
        // zin - pack(Mo); model from pack(Mo).  (Every thread its own slots of zin, here and above.)
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            void* dst = pass == 0 ? g.port : (pass == 1 ? g.resid : g.model);
            if (!dst) continue;
            if (pass > 0) {
                for (int k = tid; k < M; k += T) {
                    const cplx p = pack_model(k);
                    cplx z = make_double2(0.0, 0.0);
                    if (pass == 1) z = zin[k];
                    zin[k] = (pass == 1) ? make_double2(z.x - p.x, z.y - p.y) : p;
                }
            }
            __syncthreads();
            fft_row<M, cplx>(lds, zin, a.twB, tid);
            for (int j = tid; j < M; j += T) {
                const cplx v = lds[lds_pad<PL>(j)];
                resid_store<Tio>(dst, (size_t)row, M, j, v.x * inv, -v.y * inv);
            }
            __syncthreads();
        }
    }
}

// ---- general row lengths: the harmonic-domain form ---------------------------
// hout: k_any's harmonics of a chunk of ns subints, channel-major (row = n ns + ii); hp / hm / hr: harmonics of port,
// model and resid, row-major [ns][nchan][M + 1] (null = not formed).  The slot's rows are pitched to Mp.  Masked rows
// get zero harmonics and red_chi2 NaN (k_chan_chi2_harm ran before and knows nothing of the mask); their hout rows
// were never written and are not read.
__global__ __launch_bounds__(256) void k_resid_harm(const cplx* hout, ResidArgs g, int s0, int ns, int M, int Mp, cplx* hp,
                                                    cplx* hm, cplx* hr) {
    const ChanChi2Args& a = g.c;
    const int tid = threadIdx.x;
    const int H = M + 1;
    const long long nrows = (long long)ns * a.nchan;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int ii = (int)(row / a.nchan), n = (int)(row % a.nchan), i = s0 + ii;
        const size_t o = (size_t)row * H;
        if (!resid_live(g.mask, (size_t)i * a.nchan + n)) {
            for (int k = tid; k <= M; k += 256) {
                if (hp) hp[o + k] = make_double2(0.0, 0.0);
                if (hm) hm[o + k] = make_double2(0.0, 0.0);
                if (hr) hr[o + k] = make_double2(0.0, 0.0);
            }
            if (a.out && tid == 0) a.out[(size_t)i * a.nchan + n] = NAN;
            continue;
        }
        const ResidRow r = resid_row(a, i, n, Mp);
        const cplx* h = hout + ((size_t)n * ns + ii) * H;
        for (int k = tid; k <= M; k += 256) {
            cplx d = make_double2(0.0, 0.0), m;
            if (hp || hr) {
                d = (k == 0 || k == M) ? make_double2(h[k].x, 0.0) : h[k];
                if (g.frame == 0 && k > 0) d = cmul(d, turn_phasor((double)k, r.phin));
            }
            if (k == 0) m = make_double2(r.sc * r.m0, 0.0);
            else m = resid_model_harm(r, g.frame, k);
            if (k == M) { d.y = 0.0; m.y = 0.0; }
            if (hp) hp[o + k] = d;
            if (hm) hm[o + k] = m;
            if (hr) hr[o + k] = make_double2(d.x - m.x, d.y - m.y);
        }
    }
}

// k_irfft_any with the output's type: numpy.fft.irfft of rows of harmonics h[row][M + 1] -> out[row][nbin]
template <int L, typename Tout>
__global__ __launch_bounds__(FftPlan<L>::T) void k_resid_irfft_any(const cplx* harm, AnyArgs g, long long nrows, Tout* out) {
    constexpr int T = FftPlan<L>::T;
    __shared__ cplx lds[FftPlan<L>::LDS_ELEMS];
    __shared__ cplx buf[L];
    const int tid = threadIdx.x;
    const int M = g.M;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const cplx* h = harm + (size_t)row * (M + 1);
        for (int k = tid; k < M; k += T) {
            const cplx yk = (k == 0) ? make_double2(h[0].x, 0.0) : h[k];
            const cplx ym = (k == 0) ? make_double2(h[M].x, 0.0) : h[M - k];
            buf[k] = irfft_pack(yk, ym, g.twB[k]);
        }
        __syncthreads();
        czt_any<L>(buf, lds, g, tid);
        Tout* o = out + (size_t)row * g.nbin;
        const double inv = 1.0 / (double)M;
        for (int j = tid; j < M; j += T) {
            const cplx r = buf[j];
            o[2 * j] = (Tout)(r.x * inv);
            o[2 * j + 1] = (Tout)(-r.y * inv);
        }
        __syncthreads();
    }
}

}  // namespace pp

// ---- host ---------------------------------------------------------------------
struct ResidOut {
    void *port, *model, *resid;
    double* red_chi2;
    int count() const { return (port ? 1 : 0) + (model ? 1 : 0) + (resid ? 1 : 0); }
};

// one run of whole subints; `out`: where the run's results go (host, or device for device input)
static int fit_residuals_run(pp_ctx* c, const Ports& in, const int32_t* model_slot, const double* nu_refs3, const double* scales,
                             const double* errs, const double* mask, int frame, const ResidOut& out) {
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    const size_t nc = (size_t)nsub * nchan, bytes = (size_t)nsub * in.sub_bytes();
    const bool anyb = !nbin_ok(nbin);
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    if ((rc = upload(c, c->nufit, nu_refs3, (size_t)nsub * 24))) return rc;
    if ((rc = upload(c, c->wts, scales, nc * 8))) return rc;
    if (out.red_chi2) if ((rc = upload(c, c->errs, errs, nc * 8))) return rc;
    if (model_slot) if ((rc = upload(c, c->slot, model_slot, (size_t)nsub * 4))) return rc;
    if (mask) if ((rc = upload(c, c->misc, mask, nc * 8))) return rc;
    // rows the general-length transform may skip (k_any's byte mask); lives until the run's last synchronise
    std::vector<unsigned char> live;
    if (mask && anyb) {
        live.resize(nc);
        for (size_t q = 0; q < nc; ++q) live[q] = (mask[q] != 0.0 && mask[q] == mask[q]) ? 1 : 0;
        if ((rc = upload(c, c->mask, live.data(), nc))) return rc;
    }
    // results of a host call are staged in c->X (port | model | resid, the wanted ones) and c->sdraw
    ResidOut dev = out;
    if (!in.on_device) {
        if ((rc = c->X.reserve((size_t)out.count() * bytes))) return rc;
        char* p = (char*)c->X.p;
        if (out.port) { dev.port = p; p += bytes; }
        if (out.model) { dev.model = p; p += bytes; }
        if (out.resid) { dev.resid = p; p += bytes; }
        if (out.red_chi2) {
            if ((rc = c->sdraw.reserve(nc * 8))) return rc;
            dev.red_chi2 = c->sdraw.as<double>();
        }
    }
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    ResidArgs g{{dsrc, (const cplx* const*)c->mft_table.p, (const double* const*)c->mdc_table.p,
                 model_slot ? c->slot.as<int>() : nullptr, c->freqs.as<double>(), (long long)in.freqs_stride,
                 c->P.as<double>(), c->x0.as<double>(), c->nufit.as<double>(), c->wts.as<double>(),
                 out.red_chi2 ? c->errs.as<double>() : nullptr, tw, dev.red_chi2, nsub, nchan},
                mask ? c->misc.as<double>() : nullptr, dev.port, dev.model, dev.resid, frame};
    {
        Prof pr(c, KF_RESID);
        if (anyb) {
            // a row length without a tuned plan: the data rows' harmonics by the chirp-z route (not needed for the model
            // alone), the entry point's arithmetic per harmonic, and one chirp-z transform back per wanted output.
            // Subints go through in chunks whose harmonics (the rows' and the outputs') fit the scratch buffer.
            const size_t H = (size_t)M + 1;
            const int Mp = c->slots[model_slot ? model_slot[0] : 0].Mp;
            const int nh = 1 + out.count();
            const int cs = harm_chunk(nsub, nchan, H * nh);
            const size_t hrows = (size_t)cs * nchan * H;
            if ((rc = c->seedbuf.reserve(hrows * nh * sizeof(cplx)))) return rc;
            cplx* hout = c->seedbuf.as<cplx>();
            cplx* q = hout + hrows;
            cplx* hp = dev.port ? q : nullptr;   if (dev.port) q += hrows;
            cplx* hm = dev.model ? q : nullptr;  if (dev.model) q += hrows;
            cplx* hr = dev.resid ? q : nullptr;
            AnyArgs ga;
            int L = 0;
            if ((rc = any_args(c, nbin, &ga, &L))) return rc;
            const bool need_d = dev.port || dev.resid || dev.red_chi2;
            if ((rc = for_runs(nsub, cs, [&](Run r) {
                    const long long rows = (long long)r.n * nchan;
                    if (need_d) {
                        XspecArgs xa;
                        memset(&xa, 0, sizeof xa);
                        xa.data = r.at((const char*)dsrc, in.sub_bytes()); xa.nsub = r.n; xa.nchan = nchan; xa.nchan_full = nchan; xa.cstep = 1;
                        if (int rc = launch_any(c, xa, nbin, in.dtype, -1, false, hout, live.empty() ? nullptr : r.at(c->mask.as<unsigned char>(), nchan)))
                            return rc;
                    }
                    const int grid = (int)std::max(1LL, std::min(rows, 4096LL));
                    // ORDER MATTERS under a mask: k_chan_chi2_harm knows nothing of it and forms a figure for the masked
                    // rows too, from hout rows k_any never wrote (allocated scratch: no fault, no meaning); k_resid_harm,
                    // queued behind it on the same stream, replaces those figures by NaN.  k_chan_chi2_harm is launched
                    // as it is so that the live rows' chi^2 is pp_channel_red_chi2's to the bit.
                    if (dev.red_chi2) hipLaunchKernelGGL(k_chan_chi2_harm, dim3(grid), dim3(256), 0, c->stream, (const cplx*)hout, g.c, r.s0, r.n, M, Mp);
                    hipLaunchKernelGGL(k_resid_harm, dim3(grid), dim3(256), 0, c->stream, (const cplx*)hout, g, r.s0, r.n, M, Mp, hp, hm, hr);
                    HIP_TRY(hipGetLastError());
                    const cplx* hs[3] = {hp, hm, hr};
                    void* ds[3] = {dev.port, dev.model, dev.resid};
                    for (int j = 0; j < 3; ++j) {
                        if (!hs[j]) continue;
                        void* dst = r.at((char*)ds[j], in.sub_bytes());
                        if (int rc = with_any_len(L, [&](auto LL) {
                                with_dtype(in.dtype, [&](auto t) {
                                    hipLaunchKernelGGL((k_resid_irfft_any<decltype(LL)::value, decltype(t)>), dim3(any_grid(rows)),
                                                       dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, hs[j], ga, rows, (decltype(t)*)dst);
                                });
                            }))
                            return rc;
                    }
                    HIP_TRY(hipGetLastError());
                    return (int)PP_OK;
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_resid<MM, decltype(t)>), dim3(fft_grid(T, (long long)nc)), dim3(T), 0, c->stream, g); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    if (!in.on_device) {
        if (out.port) HIP_TRY(hipMemcpyAsync(out.port, dev.port, bytes, hipMemcpyDeviceToHost, c->stream));
        if (out.model) HIP_TRY(hipMemcpyAsync(out.model, dev.model, bytes, hipMemcpyDeviceToHost, c->stream));
        if (out.resid) HIP_TRY(hipMemcpyAsync(out.resid, dev.resid, bytes, hipMemcpyDeviceToHost, c->stream));
        if (out.red_chi2) HIP_TRY(hipMemcpyAsync(out.red_chi2, dev.red_chi2, nc * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

extern "C" int pp_fit_residuals(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int nchan, int nbin,
                                const int32_t* model_slot, const double* freqs, int64_t freqs_stride, const double* P,
                                const double* params5, const double* nu_refs3, const double* scales, const double* errs,
                                const double* mask, int frame, void* port, void* model, void* resid, double* red_chi2) {
    if (int busy_ = ctx_busy(c, "pp_fit_residuals")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, params5, 5};
    if (int rc = in.validate("pp_fit_residuals", c && nu_refs3 && scales && (errs || !red_chi2))) return rc;
    if (!port && !model && !resid && !red_chi2) return fail(PP_EINVAL, "pp_fit_residuals: no output requested");
    if (frame != 0 && frame != 1) return fail(PP_EINVAL, "pp_fit_residuals: frame %d", frame);
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < nsub; ++i) {
        const int sl = model_slot ? model_slot[i] : 0;
        if (sl < 0 || sl >= PP_MAX_SLOTS || !c->slots[sl].set || c->slots[sl].nchan != nchan ||
            c->slots[sl].nbin != nbin)
            return fail(PP_EINVAL, "pp_fit_residuals: model slot %d is not a %d x %d template", sl, nchan, nbin);
    }
    const ResidOut out{port, model, resid, red_chi2};
    // device bytes per subint beside the portrait: the staged results and the small arrays
    return for_runs(nsub, in.cap(c, (double)out.count() * (double)in.sub_bytes() + 64.0 * nchan), [&](Run r) {
        const ResidOut o{r.at((char*)port, in.sub_bytes()), r.at((char*)model, in.sub_bytes()), r.at((char*)resid, in.sub_bytes()),
                         r.at(red_chi2, nchan)};
        return fit_residuals_run(c, in.run(r), r.at(model_slot, 1), r.at(nu_refs3, 3), r.at(scales, nchan), r.at(errs, nchan),
                                 r.at(mask, nchan), frame, o);
    });
}
