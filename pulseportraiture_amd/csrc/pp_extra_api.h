// host entry points for pp_extra.h (included at the end of pp_toas.hip)

// Host-resident inputs larger than the work-memory budget go through the device in
// runs of whole subints (every operation here is independent per subint, or a sum
// over them): how many subints of `per_sub` device bytes fit
static int aux_chunk_cap(pp_ctx* c, double per_sub, int nsub) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return nsub;
    const double budget = std::min(c->max_work_bytes, 0.85 * ((double)free_b + (double)c->data.cap + (double)c->X.cap));
    return (int)std::min<double>(nsub, std::max(1.0, std::floor(budget / std::max(per_sub, 1.0))));
}

// A run of whole subints (or rows) [s0, s0 + n) of a call's host arrays; at(p, per): where the run starts in an array
// of `per` elements per subint (a null pointer stays null), so that no entry point offsets its own arguments
struct Run {
    int s0, n;
    template <typename T>
    T* at(T* p, size_t per) const { return p ? p + (size_t)s0 * per : nullptr; }
};
// body(Run) over [0, total) in runs of at most `cap`: the caller's figure, worked out once, before the first run
template <typename F>
static int for_runs(int total, int cap, F body) {
    for (int s0 = 0; s0 < total; s0 += cap)
        if (int rc = body(Run{s0, std::min(cap, total - s0)})) return rc;
    return PP_OK;
}

// Portraits plus per-subint arrays, as four entry points take them (what InLayout is to the fit's input block): one
// check, one staging, one way to cut a host input into runs
struct Ports {
    const void* src;
    int dtype, on_device, nsub, nchan, nbin;
    const double* freqs;
    int64_t freqs_stride;
    const double *P, *par;      // par: npar doubles per subint (phi, DM, GM or nu_ref; the five fitted parameters)
    int npar;
    int npol = 1;               // portraits per subint (pp_align_add: src[nsub][npol][nchan][nbin])

    size_t esz() const { return dtype == PP_F64 ? 8 : 4; }
    size_t sub_bytes() const { return (size_t)npol * nchan * nbin * esz(); }
    // rest_ok: the entry point's other pointers are there; shape_ok: its other counts are positive
    int validate(const char* who, bool rest_ok, bool shape_ok = true) const {
        if (!rest_ok || !src || !freqs || !P || !par) return fail(PP_EINVAL, "%s: null argument", who);
        if (!nbin_any_ok(nbin)) return nbin_refuse(who, nbin);
        if (nsub < 1 || nchan < 1 || !shape_ok) return fail(PP_EINVAL, "%s: bad shape", who);
        if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "%s: dtype %d", who, dtype);
        if (freqs_stride != 0 && freqs_stride != nchan) return fail(PP_EINVAL, "freqs_stride must be 0 or nchan");
        return PP_OK;
    }
    // how many subints of a host input go through the device at once (extra: device bytes per subint beside the portrait)
    int cap(pp_ctx* c, double extra) const { return on_device ? nsub : aux_chunk_cap(c, (double)sub_bytes() + extra, nsub); }
    Ports run(Run r) const {
        return Ports{r.at((const char*)src, sub_bytes()), dtype, on_device, r.n, nchan, nbin, r.at(freqs, (size_t)freqs_stride),
                     freqs_stride, r.at(P, 1), r.at(par, npar), npar, npol};
    }
    // the portraits on the device (host ones through c->data), freqs -> c->freqs, P -> c->P, par -> c->x0
    int stage(pp_ctx* c, const void** dsrc) const {
        int rc;
        *dsrc = src;
        if (!on_device) {
            if ((rc = upload(c, c->data, src, (size_t)nsub * sub_bytes()))) return rc;
            *dsrc = c->data.p;
        }
        if ((rc = upload(c, c->freqs, freqs, (size_t)(freqs_stride ? (size_t)nsub * nchan : nchan) * 8))) return rc;
        if ((rc = upload(c, c->P, P, (size_t)nsub * 8))) return rc;
        return upload(c, c->x0, par, (size_t)nsub * npar * 8);
    }
};

// 1 / nu^2 and 1 / nu^4 of a reference frequency, 0 for "none" (infinite)
static double inv_nu2(double nu) { return std::isinf(nu) ? 0.0 : 1.0 / (nu * nu); }
static double inv_nu4(double nu) { return std::isinf(nu) ? 0.0 : 1.0 / (nu * nu * nu * nu); }

// the end of a call that fits n profiles between c->ev0 and now: seven columns each to the host, the last one the
// span's time shared out among them
static int fetch_out7(pp_ctx* c, int n, double* out7) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(out7, c->o_params.p, (size_t)n * 56, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    for (int i = 0; i < n; ++i) out7[(size_t)i * 7 + 6] = 1e-3 * ms / n;
    return PP_OK;
}

static int fit_phase_shift_run(pp_ctx* c, const double* data, const double* model, const double* noise, int nprof,
                               int nbin, double lo, double hi, int Ns, double* out7) {
    const int M = nbin / 2;
    int rc;
    // interleave rows: data_i, model_i
    const size_t rowb = (size_t)nbin * 8;
    if ((rc = c->data.reserve(2 * (size_t)nprof * rowb))) return rc;
    HIP_TRY(hipMemcpy2DAsync(c->data.p, 2 * rowb, data, rowb, rowb, nprof, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync((char*)c->data.p + rowb, 2 * rowb, model, rowb, rowb, nprof, hipMemcpyHostToDevice, c->stream));
    if ((rc = c->X.reserve((size_t)nprof * (2 * (size_t)(M + 1) + M) * sizeof(cplx)))) return rc;
    if ((rc = c->o_params.reserve((size_t)nprof * 56))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;      // (a first use copies the table: not inside the timed span)
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    cplx* spec = c->X.as<cplx>();
    cplx* xwork = spec + 2 * (size_t)nprof * (M + 1);
    {
        Prof pr(c, KF_FPS);
        if ((rc = rows_harmonics(c, c->data.p, PP_F64, 2 * nprof, nbin, spec))) return rc;
        const double* dnoise = nullptr;
        if (noise) {
            if ((rc = upload(c, c->errs, noise, (size_t)nprof * 8))) return rc;
            dnoise = c->errs.as<double>();
        }
        FpsArgs fa{spec, dnoise, c->o_params.as<double>(), lo, hi, Ns, M, nprof, c->fps_finish, nullptr, M + 1};
        hipLaunchKernelGGL(k_fps, dim3(nprof), dim3(256), 0, c->stream, fa, xwork);
    }
    return fetch_out7(c, nprof, out7);
}

extern "C" int pp_fit_phase_shift_batch(pp_ctx* c, const double* data, const double* model, const double* noise,
                                        int nprof, int nbin, double lo, double hi, int Ns, double* out7) {
    if (int busy_ = ctx_busy(c, "pp_fit_phase_shift_batch")) return busy_;
    if (!c || !data || !model || !out7) return fail(PP_EINVAL, "pp_fit_phase_shift_batch: null argument");
    if (!nbin_any_ok(nbin)) return nbin_refuse("pp_fit_phase_shift_batch", nbin);
    if (nprof < 1) return fail(PP_EINVAL, "pp_fit_phase_shift_batch: bad shape %d x %d", nprof, nbin);
    if (Ns < 1) return fail(PP_EINVAL, "pp_fit_phase_shift_batch: Ns %d", Ns);
    HIP_TRY(hipSetDevice(c->device));
    const int M = nbin / 2;
    return for_runs(nprof, aux_chunk_cap(c, 2.0 * nbin * 8 + (2.0 * (M + 1) + M) * 16 + 64, nprof), [&](Run r) {
        return fit_phase_shift_run(c, r.at(data, nbin), r.at(model, nbin), r.at(noise, 1), r.n, nbin, lo, hi, Ns, r.at(out7, 7));
    });
}

// ---- the reference's initial phase guess, data side fused --------------------
static int reference_phase_seed_run(pp_ctx* c, const Ports& in, double nu_DM, double nu_GM, const double* weights,
                                    const double* model_profs, double lo, double hi, int Ns, double* out7) {
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    const bool anyb = !nbin_ok(nbin);
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    if ((rc = upload(c, c->wts, weights, (size_t)nsub * nchan * 8))) return rc;
    if ((rc = upload(c, c->errs, model_profs, (size_t)nsub * nbin * 8))) return rc;
    // runs of channels per subint: one partial spectrum per run, the runs added in a fixed order.  The run
    // length is a function of the band alone (an eighth of it, 16 ... 256 channels), never of the number of
    // subints in the call: the reference's guess for a subint does not depend on its neighbours (pptoas.py:421-457)
    const int cpr = std::max(16, std::min(256, (((nchan + 7) / 8) + 15) / 16 * 16));
    // (general row lengths: the harmonics of every row are written out first -- nrun = nchan slots of H)
    const int nrun = anyb ? nchan : (nchan + cpr - 1) / cpr;
    const size_t H = (size_t)M + 1;
    // X: [nsub][nrun][H] partial spectra | [nsub][H] data spectra | [nsub][H] model spectra | [nsub][M] k_fps work
    if ((rc = c->X.reserve(((size_t)nsub * nrun * H + 2 * (size_t)nsub * H + (size_t)nsub * M) * sizeof(cplx)))) return rc;
    if ((rc = c->sdraw.reserve((size_t)nsub * nrun * 8))) return rc;
    if ((rc = c->o_params.reserve((size_t)nsub * 56))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    cplx* part = c->X.as<cplx>();
    cplx* dspec = part + (size_t)nsub * nrun * H;
    cplx* mspec = dspec + (size_t)nsub * H;
    cplx* xwork = mspec + (size_t)nsub * H;
    RotMeanArgs ra{dsrc, c->freqs.as<double>(), (long long)in.freqs_stride, c->P.as<double>(), c->x0.as<double>(),
                   c->wts.as<double>(), tw, inv_nu2(nu_DM), inv_nu4(nu_GM), part, c->sdraw.as<double>(), nsub, nchan, nrun, cpr};
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    {
        Prof pr(c, KF_FPS);
        if (anyb) {
            // row lengths without a tuned plan (pp_anybin.h): every row's harmonics by the chirp-z path, then
            // the weighted, rotated channel sum per harmonic
            if ((rc = harmonics_any(c, dsrc, in.dtype, nsub, nchan, nbin, part))) return rc;
            hipLaunchKernelGGL(k_rot_mean_harm, dim3((unsigned)((M + 1 + 255) / 256), nsub), dim3(256), 0, c->stream,
                               (const cplx*)part, ra, M, dspec);
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) {
                    // 2048-bin rows: the one-exchange transform (k_rot_mean_q1024)
                    if (MM == 1024 && c->one_exchange) hipLaunchKernelGGL((k_rot_mean_q1024<decltype(t)>), dim3(nsub * nrun), dim3(64), 0, c->stream, ra);
                    else hipLaunchKernelGGL((k_rot_mean<MM, decltype(t)>), dim3(nsub * nrun), dim3(T), 0, c->stream, ra);
                });
                hipLaunchKernelGGL(k_rot_mean_finish, dim3((M + 1 + 255) / 256, nsub), dim3(256), 0, c->stream,
                                   (const cplx*)part, (const double*)c->sdraw.as<double>(), nsub, nrun, M, dspec);
            });
        }
        // the template profiles' spectra
        if ((rc = rows_harmonics(c, c->errs.p, PP_F64, nsub, nbin, mspec))) return rc;
        FpsArgs fa{dspec, nullptr, c->o_params.as<double>(), lo, hi, Ns, M, nsub, c->fps_finish, mspec, M + 1};
        hipLaunchKernelGGL(k_fps, dim3(nsub), dim3(256), 0, c->stream, fa, xwork);
    }
    return fetch_out7(c, nsub, out7);
}

extern "C" int pp_reference_phase_seed(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int nchan,
                                       int nbin, const double* freqs, int64_t freqs_stride, const double* P,
                                       const double* par3, double nu_DM, double nu_GM, const double* weights,
                                       const double* model_profs, double lo, double hi, int Ns, double* out7) {
    if (int busy_ = ctx_busy(c, "pp_reference_phase_seed")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, par3, 3};
    if (int rc = in.validate("pp_reference_phase_seed", c && weights && model_profs && out7, Ns >= 1)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return for_runs(nsub, in.cap(c, 64.0 * nchan + 64.0 * nbin), [&](Run r) {
        return reference_phase_seed_run(c, in.run(r), nu_DM, nu_GM, r.at(weights, nchan), r.at(model_profs, nbin), lo, hi, Ns, r.at(out7, 7));
    });
}

// ---- general row lengths (pp_anybin.h): harmonics back ---------------------
// numpy.fft.irfft of nrows rows of M + 1 harmonics -> out[nrows][nbin] (device pointers)
static int irfft_any(pp_ctx* c, int nbin, const cplx* harm, long long nrows, double* out) {
    AnyArgs g;
    int L = 0, rc;
    if ((rc = any_args(c, nbin, &g, &L))) return rc;
    if ((rc = with_any_len(L, [&](auto LL) {
            hipLaunchKernelGGL((k_irfft_any<decltype(LL)::value>), dim3(any_grid(nrows)), dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, harm, g, nrows, out);
        })))
        return rc;
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

extern "C" int pp_synth_portraits(pp_ctx* c, int slot, void* dst, int dtype, int nsub, const double* freqs,
                                  const double* P, const double* inj, const double* gains, double sigma,
                                  uint64_t seed, int64_t first_subint) {
    if (int busy_ = ctx_busy(c, "pp_synth_portraits")) return busy_;
    if (!c || !dst || !freqs || !P || !inj) return fail(PP_EINVAL, "pp_synth_portraits: null argument");
    if (slot < 0 || slot >= PP_MAX_SLOTS || !c->slots[slot].set) return fail(PP_ESTATE, "pp_synth_portraits: slot %d not set", slot);
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_synth_portraits: dtype %d", dtype);
    if (nsub < 1) return fail(PP_EINVAL, "pp_synth_portraits: nsub %d", nsub);
    HIP_TRY(hipSetDevice(c->device));
    ModelSlot& s = c->slots[slot];
    const int C = s.nchan, B = s.nbin, M = B / 2;
    int rc;
    if ((rc = upload(c, c->freqs, freqs, (size_t)C * 8))) return rc;
    if ((rc = upload(c, c->P, P, (size_t)nsub * 8))) return rc;
    if ((rc = upload(c, c->x0, inj, (size_t)nsub * 24))) return rc;
    if (gains) if ((rc = upload(c, c->errs, gains, (size_t)nsub * C * 8))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, B, &tw))) return rc;
    SynthArgs a{s.mft.as<cplx>(), s.mdc.as<double>(), dst, c->freqs.as<double>(), c->P.as<double>(),
                c->x0.as<double>(), tw, sigma, seed, first_subint, nsub, C,
                gains ? c->errs.as<double>() : (const double*)nullptr};
    const long long nrows = (long long)nsub * C;
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(B)) {
            // a row length without a tuned plan: the rotated template's harmonics back by the chirp-z route
            AnyArgs g;
            int L = 0;
            if ((rc = any_args(c, B, &g, &L))) return rc;
            if ((rc = with_any_len(L, [&](auto LL) {
                    with_dtype(dtype, [&](auto t) { hipLaunchKernelGGL((k_synth_any<decltype(LL)::value, decltype(t)>), dim3(any_grid(nrows)), dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, a, g); });
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(dtype, [&](auto t) { hipLaunchKernelGGL((k_synth<MM, decltype(t)>), dim3(fft_grid(T, nrows)), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

// (dst: where the run's rotated portraits go; host portraits are rotated in place in c->data)
static int rotate_portraits_run(pp_ctx* c, const Ports& in, void* dst, double nu_DM, double nu_GM) {
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    const size_t bytes = (size_t)nsub * in.sub_bytes();
    const long long nrows = (long long)nsub * nchan;
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    RotateArgs a{dsrc, in.on_device ? dst : c->data.p, c->freqs.as<double>(), (long long)in.freqs_stride, c->P.as<double>(),
                 c->x0.as<double>(), tw, inv_nu2(nu_DM), inv_nu4(nu_GM), nsub, nchan};
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(nbin)) {
            // a row length without a tuned plan: the chirp-z route, forward and back (pp_anybin.h)
            AnyArgs g;
            int L = 0;
            if ((rc = any_args(c, nbin, &g, &L))) return rc;
            if ((rc = with_any_len(L, [&](auto LL) {
                    with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_rotate_any<decltype(LL)::value, decltype(t)>), dim3(any_grid(nrows)), dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, a, g); });
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_rotate<MM, decltype(t)>), dim3(fft_grid(T, nrows)), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    if (!in.on_device) HIP_TRY(hipMemcpyAsync(dst, c->data.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

extern "C" int pp_rotate_portraits(pp_ctx* c, const void* src, void* dst, int dtype, int on_device, int nsub,
                                   int nchan, int nbin, const double* freqs, int64_t freqs_stride,
                                   const double* P, const double* par3, double nu_DM, double nu_GM) {
    if (int busy_ = ctx_busy(c, "pp_rotate_portraits")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, par3, 3};
    if (int rc = in.validate("pp_rotate_portraits", c && dst)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return for_runs(nsub, in.cap(c, 64.0 * nchan), [&](Run r) {
        return rotate_portraits_run(c, in.run(r), r.at((char*)dst, in.sub_bytes()), nu_DM, nu_GM);
    });
}

// ---- ppalign accumulation -------------------------------------------------
// how many subints' harmonics (general row lengths: M + 1 per row) fit a 2 GB scratch buffer
static int harm_chunk(int nsub, int nchan, size_t H) {
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)nsub, ((size_t)2 << 30) / ((size_t)nchan * H * sizeof(cplx))));
}

static int align_accumulate_run(pp_ctx* c, const Ports& in, const double* weights, double* aligned, double* total_weights) {
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    if ((rc = upload(c, c->wts, weights, (size_t)nsub * nchan * 8))) return rc;
    if ((rc = c->X.reserve((size_t)nchan * nbin * 8))) return rc;          // aligned portrait
    if ((rc = c->sdraw.reserve((size_t)nchan * 8))) return rc;             // total weights
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    AlignArgs a{dsrc, c->freqs.as<double>(), (long long)in.freqs_stride, c->P.as<double>(), c->x0.as<double>(),
                c->wts.as<double>(), tw, c->X.as<double>(), c->sdraw.as<double>(), nsub, nchan};
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(nbin)) {
            // a row length without a tuned plan (pp_anybin.h): harmonics of every row by the chirp-z route, the weighted,
            // rotated sum per (channel, harmonic) over the subints in index order, ONE inverse transform per channel.
            // Subints go through in chunks whose harmonics fit the scratch buffer.
            const size_t H = (size_t)M + 1;
            const int cs = harm_chunk(nsub, nchan, H);
            if ((rc = c->seedbuf.reserve(((size_t)cs * nchan * H + (size_t)nchan * H) * sizeof(cplx)))) return rc;
            cplx* hout = c->seedbuf.as<cplx>();
            cplx* spec = hout + (size_t)cs * nchan * H;
            if ((rc = for_runs(nsub, cs, [&](Run r) {
                    if (int rc = harmonics_any(c, r.at((const char*)dsrc, in.sub_bytes()), in.dtype, r.n, nchan, nbin, hout)) return rc;
                    hipLaunchKernelGGL(k_align_harm, dim3((unsigned)((H + 255) / 256), nchan), dim3(256), 0, c->stream,
                                       (const cplx*)hout, a, r.s0, r.n, M, spec, c->sdraw.as<double>(), r.s0 == 0 ? 1 : 0);
                    HIP_TRY(hipGetLastError());
                    return (int)PP_OK;
                })))
                return rc;
            if ((rc = irfft_any(c, nbin, spec, nchan, c->X.as<double>()))) return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_align_accum<MM, decltype(t)>), dim3(nchan), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(aligned, c->X.p, (size_t)nchan * nbin * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(total_weights, c->sdraw.p, (size_t)nchan * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

extern "C" int pp_align_accumulate(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int nchan,
                                   int nbin, const double* freqs, int64_t freqs_stride, const double* P,
                                   const double* par3, const double* weights, double* aligned,
                                   double* total_weights) {
    if (int busy_ = ctx_busy(c, "pp_align_accumulate")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, par3, 3};
    if (int rc = in.validate("pp_align_accumulate", c && weights && aligned && total_weights)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int cap = in.cap(c, 64.0 * nchan);
    if (nsub <= cap) return align_accumulate_run(c, in, weights, aligned, total_weights);
    // the sums of the runs are added on the host
    std::vector<double> part((size_t)nchan * nbin), wpart((size_t)nchan);
    std::fill(aligned, aligned + (size_t)nchan * nbin, 0.0);
    std::fill(total_weights, total_weights + nchan, 0.0);
    return for_runs(nsub, cap, [&](Run r) {
        if (int rc = align_accumulate_run(c, in.run(r), r.at(weights, nchan), part.data(), wpart.data())) return rc;
        for (size_t j = 0; j < part.size(); ++j) aligned[j] += part[j];
        for (int j = 0; j < nchan; ++j) total_weights[j] += wpart[j];
        return (int)PP_OK;
    });
}

// ---- ppalign: the resident accumulator ------------------------------------
extern "C" int pp_align_begin(pp_ctx* c, int npol, int nchan_model, int nbin) {
    if (int busy_ = ctx_busy(c, "pp_align_begin")) return busy_;
    if (!c) return fail(PP_EINVAL, "pp_align_begin: null context");
    c->align.open = false;      // (a refused begin leaves no accumulator either)
    if (!nbin_any_ok(nbin)) return nbin_refuse("pp_align_begin", nbin);
    if (npol < 1 || npol > 4 || nchan_model < 1) return fail(PP_EINVAL, "pp_align_begin: bad shape %d x %d", npol, nchan_model);
    HIP_TRY(hipSetDevice(c->device));
    pp_ctx::Align& A = c->align;
    const size_t accb = (size_t)npol * nchan_model * (nbin / 2) * sizeof(cplx);
    int rc;
    if ((rc = A.acc.reserve(accb))) return rc;
    if ((rc = A.totw.reserve((size_t)nchan_model * 8))) return rc;
    if ((rc = A.out.reserve((size_t)npol * nchan_model * nbin * 8))) return rc;
    HIP_TRY(hipMemsetAsync(A.acc.p, 0, accb, c->stream));
    HIP_TRY(hipMemsetAsync(A.totw.p, 0, (size_t)nchan_model * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    A.npol = npol; A.nchan = nchan_model; A.nbin = nbin; A.open = true;
    return PP_OK;
}

// the contribution lists of a run (CSR): off[m] .. off[m + 1] are model row m's (subint, data channel) pairs, by subint,
// then data channel; rows of weight 0 or NaN are left out.  chan_map: [nsub][nchan] or null (identity)
static void align_lists(int nsub, int nchan, int nchan_model, const double* weights, const int32_t* chan_map,
                        std::vector<int>& off, std::vector<int>& pairs) {
    off.assign((size_t)nchan_model + 1, 0);
    auto live = [&](size_t j) { return !(weights[j] == 0.0 || weights[j] != weights[j]); };
    auto row_of = [&](size_t j, int n) { return chan_map ? (int)chan_map[j] : n; };
    for (int i = 0; i < nsub; ++i)
        for (int n = 0; n < nchan; ++n) {
            const size_t j = (size_t)i * nchan + n;
            if (live(j)) ++off[(size_t)row_of(j, n) + 1];
        }
    for (int m = 0; m < nchan_model; ++m) off[(size_t)m + 1] += off[m];
    pairs.assign(2 * (size_t)off[nchan_model], 0);
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int i = 0; i < nsub; ++i)
        for (int n = 0; n < nchan; ++n) {
            const size_t j = (size_t)i * nchan + n;
            if (!live(j)) continue;
            const int q = at[row_of(j, n)]++;
            pairs[2 * (size_t)q] = i;
            pairs[2 * (size_t)q + 1] = n;
        }
}

// the lists pp_align_add builds for one run, for callers and tests that want to see them (no device is touched):
// off[nchan_model + 1], pairs[2 x (number of live rows)] as (subint, data channel); returns the number of pairs
extern "C" int pp_align_lists(int nsub, int nchan, int nchan_model, const double* weights, const int32_t* chan_map,
                              int32_t* off, int32_t* pairs) {
    if (!weights || !off || !pairs) return fail(PP_EINVAL, "pp_align_lists: null argument");
    if (nsub < 1 || nchan < 1 || nchan_model < 1) return fail(PP_EINVAL, "pp_align_lists: bad shape");
    if (!chan_map && nchan != nchan_model)
        return fail(PP_EINVAL, "pp_align_lists: %d channels without a channel map onto %d rows", nchan, nchan_model);
    if (chan_map)
        for (size_t j = 0; j < (size_t)nsub * nchan; ++j)
            if (chan_map[j] < 0 || chan_map[j] >= nchan_model)
                return fail(PP_EINVAL, "pp_align_lists: chan_map[%zu][%zu] = %d is no row of %d", j / nchan, j % nchan, (int)chan_map[j], nchan_model);
    std::vector<int> o, p;
    align_lists(nsub, nchan, nchan_model, weights, chan_map, o, p);
    std::copy(o.begin(), o.end(), off);
    std::copy(p.begin(), p.end(), pairs);
    return (int)(p.size() / 2);
}

static int align_add_run(pp_ctx* c, const Ports& in, const double* weights, const int32_t* chan_map) {
    pp_ctx::Align& A = c->align;
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    std::vector<int> off, pairs;
    align_lists(nsub, nchan, A.nchan, weights, chan_map, off, pairs);
    if (pairs.empty()) return PP_OK;          // every row of the run is skipped
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    if ((rc = upload(c, c->wts, weights, (size_t)nsub * nchan * 8))) return rc;
    if ((rc = upload(c, A.off, off.data(), off.size() * sizeof(int)))) return rc;
    if ((rc = upload(c, A.pairs, pairs.data(), pairs.size() * sizeof(int)))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    AlignListArgs a{dsrc, c->freqs.as<double>(), (long long)in.freqs_stride, c->P.as<double>(), c->x0.as<double>(),
                    c->wts.as<double>(), tw, A.acc.as<cplx>(), A.totw.as<double>(), A.off.as<int>(), A.pairs.as<int2>(),
                    A.npol, nchan, A.nchan};
    const unsigned nrows = (unsigned)(A.npol * A.nchan);
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(nbin)) {
            // a row length without a tuned plan (pp_anybin.h): the harmonics of the run's rows by the chirp-z route, then
            // the list walk per slot of the packed row
            const size_t H = (size_t)M + 1;
            if ((rc = A.harm.reserve((size_t)nsub * A.npol * nchan * H * sizeof(cplx)))) return rc;
            if ((rc = harmonics_any(c, dsrc, in.dtype, nsub * A.npol, nchan, nbin, A.harm.as<cplx>()))) return rc;
            hipLaunchKernelGGL(k_align_harm_list, dim3((unsigned)((M + 255) / 256), nrows), dim3(256), 0, c->stream,
                               (const cplx*)A.harm.as<cplx>(), a, nsub, M);
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_align_add<MM, decltype(t)>), dim3(nrows), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the lists and the caller's arrays are free again)
    return PP_OK;
}

extern "C" int pp_align_add(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int npol, int nchan,
                            int nbin, const double* freqs, int64_t freqs_stride, const double* P, const double* par3,
                            const double* weights, const int32_t* chan_map) {
    if (int busy_ = ctx_busy(c, "pp_align_add")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, par3, 3, npol};
    if (int rc = in.validate("pp_align_add", c && weights, npol >= 1)) return rc;
    const pp_ctx::Align& A = c->align;
    if (!A.open) return fail(PP_EINVAL, "pp_align_add: no accumulator (pp_align_begin first)");
    if (npol != A.npol || nbin != A.nbin)
        return fail(PP_EINVAL, "pp_align_add: %d x %d-bin rows, the accumulator holds %d x %d-bin rows", npol, nbin, A.npol, A.nbin);
    if (!chan_map && nchan != A.nchan)
        return fail(PP_EINVAL, "pp_align_add: %d channels without a channel map, the accumulator holds %d", nchan, A.nchan);
    if (chan_map)
        for (size_t j = 0; j < (size_t)nsub * nchan; ++j)
            if (chan_map[j] < 0 || chan_map[j] >= A.nchan)
                return fail(PP_EINVAL, "pp_align_add: chan_map[%zu][%zu] = %d is no row of the %d-channel accumulator", j / nchan,
                            j % nchan, (int)chan_map[j], A.nchan);
    HIP_TRY(hipSetDevice(c->device));
    // (general row lengths: a run's harmonics, 16 (nbin / 2 + 1) bytes per sample row, are device work memory too)
    const double harm = nbin_ok(nbin) ? 0.0 : 16.0 * (nbin / 2 + 1) * npol * nchan;
    int cap = in.cap(c, 64.0 * nchan + harm);
    if (harm > 0.0) cap = std::min(cap, harm_chunk(nsub, npol * nchan, (size_t)nbin / 2 + 1));
    return for_runs(nsub, cap, [&](Run r) { return align_add_run(c, in.run(r), r.at(weights, nchan), r.at(chan_map, nchan)); });
}

extern "C" int pp_align_finish(pp_ctx* c, double rot_phase, double* aligned, double* total_weights, int to_slot) {
    if (int busy_ = ctx_busy(c, "pp_align_finish")) return busy_;
    if (!c || !aligned || !total_weights) return fail(PP_EINVAL, "pp_align_finish: null argument");
    pp_ctx::Align& A = c->align;
    if (!A.open) return fail(PP_EINVAL, "pp_align_finish: no accumulator (pp_align_begin first)");
    if (to_slot >= PP_MAX_SLOTS) return fail(PP_EINVAL, "pp_align_finish: slot %d", to_slot);
    if (rot_phase != rot_phase) return fail(PP_EINVAL, "pp_align_finish: rot_phase is NaN");
    HIP_TRY(hipSetDevice(c->device));
    const int nbin = A.nbin, M = nbin / 2, nrows = A.npol * A.nchan;
    const cplx* tw = nullptr;
    int rc;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    AlignFinishArgs a{A.acc.as<cplx>(), A.totw.as<double>(), tw, A.out.as<double>(), rot_phase, A.npol, A.nchan};
    {
        Prof pr(c, KF_SYNTH);
        if (!nbin_ok(nbin)) {
            AnyArgs g;
            int L = 0;
            if ((rc = any_args(c, nbin, &g, &L))) return rc;
            if ((rc = with_any_len(L, [&](auto LL) {
                    hipLaunchKernelGGL((k_align_finish_any<decltype(LL)::value>), dim3(any_grid(nrows)), dim3(FftPlan<decltype(LL)::value>::T), 0, c->stream, a, g);
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                hipLaunchKernelGGL((k_align_finish<MM>), dim3(fft_grid(T, nrows)), dim3(T), 0, c->stream, a);
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(aligned, A.out.p, (size_t)nrows * nbin * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(total_weights, A.totw.p, (size_t)A.nchan * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // polarisation 0 into a template slot from the device copy: the bytes pp_model_set of `aligned` would transform
    if (to_slot >= 0) return pp_model_set(c, to_slot, A.out.p, PP_F64, 1, A.nchan, nbin);
    return PP_OK;
}

// ---- per-channel reduced chi^2 of fitted subints ---------------------------
static int channel_red_chi2_run(pp_ctx* c, const Ports& in, const int32_t* model_slot, const double* nu_refs3,
                                const double* scales, const double* errs, double* red_chi2) {
    const int nsub = in.nsub, nchan = in.nchan, nbin = in.nbin, M = nbin / 2;
    const size_t nc = (size_t)nsub * nchan;
    const void* dsrc = nullptr;
    int rc;
    if ((rc = in.stage(c, &dsrc))) return rc;
    if ((rc = upload(c, c->nufit, nu_refs3, (size_t)nsub * 24))) return rc;
    if ((rc = upload(c, c->wts, scales, nc * 8))) return rc;
    if ((rc = upload(c, c->errs, errs, nc * 8))) return rc;
    if (model_slot) if ((rc = upload(c, c->slot, model_slot, (size_t)nsub * 4))) return rc;
    if ((rc = c->sdraw.reserve(nc * 8))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    ChanChi2Args a{dsrc, (const cplx* const*)c->mft_table.p, (const double* const*)c->mdc_table.p,
                   model_slot ? c->slot.as<int>() : nullptr, c->freqs.as<double>(), (long long)in.freqs_stride,
                   c->P.as<double>(), c->x0.as<double>(), c->nufit.as<double>(), c->wts.as<double>(),
                   c->errs.as<double>(), tw, c->sdraw.as<double>(), nsub, nchan};
    {
        Prof pr(c, KF_FINAL);
        if (!nbin_ok(nbin)) {
            // a row length without a tuned plan: the data rows' harmonics by the chirp-z route, then Parseval on the
            // residual spectrum exactly as k_chan_chi2 forms it (the slot's spectrum rows are pitched to Mp)
            const size_t H = (size_t)M + 1;
            const int Mp = c->slots[model_slot ? model_slot[0] : 0].Mp;
            const int cs = harm_chunk(nsub, nchan, H);
            if ((rc = c->seedbuf.reserve((size_t)cs * nchan * H * sizeof(cplx)))) return rc;
            cplx* hout = c->seedbuf.as<cplx>();
            if ((rc = for_runs(nsub, cs, [&](Run r) {
                    if (int rc = harmonics_any(c, r.at((const char*)dsrc, in.sub_bytes()), in.dtype, r.n, nchan, nbin, hout)) return rc;
                    const int grid = (int)std::max(1LL, std::min((long long)r.n * nchan, 4096LL));
                    hipLaunchKernelGGL(k_chan_chi2_harm, dim3(grid), dim3(256), 0, c->stream, (const cplx*)hout, a, r.s0, r.n, M, Mp);
                    HIP_TRY(hipGetLastError());
                    return (int)PP_OK;
                })))
                return rc;
        } else {
            PP_DISPATCH_M(M, {
                const int T = FftPlan<MM>::T;
                with_dtype(in.dtype, [&](auto t) { hipLaunchKernelGGL((k_chan_chi2<MM, decltype(t)>), dim3(fft_grid(T, (long long)nc)), dim3(T), 0, c->stream, a); });
            });
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(red_chi2, c->sdraw.p, nc * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

extern "C" int pp_channel_red_chi2(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int nchan,
                                   int nbin, const int32_t* model_slot, const double* freqs,
                                   int64_t freqs_stride, const double* P, const double* params5,
                                   const double* nu_refs3, const double* scales, const double* errs,
                                   double* red_chi2) {
    if (int busy_ = ctx_busy(c, "pp_channel_red_chi2")) return busy_;
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, freqs, freqs_stride, P, params5, 5};
    if (int rc = in.validate("pp_channel_red_chi2", c && nu_refs3 && scales && errs && red_chi2)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < nsub; ++i) {
        const int sl = model_slot ? model_slot[i] : 0;
        if (sl < 0 || sl >= PP_MAX_SLOTS || !c->slots[sl].set || c->slots[sl].nchan != nchan ||
            c->slots[sl].nbin != nbin)
            return fail(PP_EINVAL, "pp_channel_red_chi2: model slot %d is not a %d x %d template", sl, nchan, nbin);
    }
    return for_runs(nsub, in.cap(c, 64.0 * nchan), [&](Run r) {
        return channel_red_chi2_run(c, in.run(r), r.at(model_slot, 1), r.at(nu_refs3, 3), r.at(scales, nchan), r.at(errs, nchan),
                                    r.at(red_chi2, nchan));
    });
}

// A template generated on the device -- gen(dev_out) checks the generator's arguments and queues it -- into the
// caller's device buffer, to the host (portrait, !out_on_device), or, with portrait == nullptr, into model slot
// `slot` without a host copy
template <typename G>
static int generated_template(pp_ctx* c, int nchan, int nbin, G gen, double* portrait, int out_on_device, int slot) {
    const size_t bytes = (size_t)nchan * nbin * 8;
    int rc;
    double* dout = portrait;
    if (!portrait || !out_on_device) {
        // scratch for the portrait.  On its way into a slot it is c->X, except for general row lengths: there
        // pp_model_set leaves the rows' harmonics in c->X
        DevBuf& scratch = !portrait && nbin_ok(nbin) ? c->X : c->data;
        if ((rc = scratch.reserve(bytes))) return rc;
        dout = scratch.as<double>();
    }
    if ((rc = gen(dout))) return rc;
    if (!portrait) return pp_model_set(c, slot, dout, PP_F64, 1, nchan, nbin);
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(portrait, dout, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PP_OK;
}

// ---- Gaussian-component templates on the device ------------------------------
static int gauss_generate(pp_ctx* c, int nchan, int nbin, const double* freqs, const char* code, double nu_ref,
                          double dc, double tau_rot, double alpha, int ngauss, const double* comps,
                          double* dev_out) {
    if (!freqs || !code || !comps) return fail(PP_EINVAL, "gaussian portrait: null argument");
    if (!nbin_any_ok(nbin)) return nbin_refuse("gaussian portrait", nbin);
    if (nchan < 1) return fail(PP_EINVAL, "gaussian portrait: bad shape");
    if (ngauss < 1 || ngauss > PP_MAX_GAUSS) return fail(PP_EINVAL, "gaussian portrait: 1..%d components", PP_MAX_GAUSS);
    for (int j = 0; j < 3; ++j)
        if (code[j] != '0' && code[j] != '1') return fail(PP_EINVAL, "gaussian portrait: model code '%.3s'", code);
    int rc;
    if ((rc = upload(c, c->freqs, freqs, (size_t)nchan * 8))) return rc;
    if ((rc = upload(c, c->misc, comps, (size_t)ngauss * 48))) return rc;
    const cplx* tw = nullptr;
    if ((rc = get_twiddles(c, nbin, &tw))) return rc;
    GaussArgs a{c->freqs.as<double>(), c->misc.as<double>(), tw, dev_out, nu_ref, dc, tau_rot, alpha, nchan, ngauss,
                code[0] - '0', code[1] - '0', code[2] - '0'};
    const int M = nbin / 2;
    if (!nbin_ok(nbin)) {
        // a row length without a tuned plan: the rows need no transform; a scattered model's filter
        // 1 / (1 + 2 pi i k tau_n) goes through the harmonics (chirp-z route there and back)
        Prof pr(c, KF_MODEL);
        hipLaunchKernelGGL(k_gauss_rows, dim3(nchan), dim3(256), 0, c->stream, a, nbin);
        HIP_TRY(hipGetLastError());
        if (tau_rot != 0.0) {
            const size_t H = (size_t)M + 1;
            if ((rc = c->seedbuf.reserve((size_t)nchan * H * sizeof(cplx)))) return rc;
            cplx* harm = c->seedbuf.as<cplx>();
            if ((rc = harmonics_any(c, dev_out, PP_F64, 1, nchan, nbin, harm))) return rc;
            hipLaunchKernelGGL(k_scatter_harm, dim3((unsigned)((H + 255) / 256), nchan), dim3(256), 0, c->stream, harm,
                               (const double*)c->freqs.as<double>(), nu_ref, tau_rot, alpha, M);
            HIP_TRY(hipGetLastError());
            if ((rc = irfft_any(c, nbin, harm, nchan, dev_out))) return rc;
        }
        return PP_OK;
    }
    {
        Prof pr(c, KF_MODEL);
        PP_DISPATCH_M(M, {
            const int T = FftPlan<MM>::T;
            hipLaunchKernelGGL((k_gauss_portrait<MM>), dim3(nchan), dim3(T), 0, c->stream, a);
        });
    }
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

extern "C" int pp_gaussian_portrait(pp_ctx* c, int nchan, int nbin, const double* freqs, const char* code,
                                    double nu_ref, double dc, double tau_rot, double alpha, int ngauss,
                                    const double* comps, double* portrait, int out_on_device) {
    if (int busy_ = ctx_busy(c, "pp_gaussian_portrait")) return busy_;
    if (!c || !portrait) return fail(PP_EINVAL, "pp_gaussian_portrait: null argument");
    HIP_TRY(hipSetDevice(c->device));
    return generated_template(c, nchan, nbin, [&](double* dout) {
        return gauss_generate(c, nchan, nbin, freqs, code, nu_ref, dc, tau_rot, alpha, ngauss, comps, dout);
    }, portrait, out_on_device, -1);
}

extern "C" int pp_model_set_gaussian(pp_ctx* c, int slot, int nchan, int nbin, const double* freqs,
                                     const char* code, double nu_ref, double dc, double tau_rot, double alpha,
                                     int ngauss, const double* comps) {
    if (int busy_ = ctx_busy(c, "pp_model_set_gaussian")) return busy_;
    if (!c) return fail(PP_EINVAL, "pp_model_set_gaussian: null context");
    HIP_TRY(hipSetDevice(c->device));
    return generated_template(c, nchan, nbin, [&](double* dout) {
        return gauss_generate(c, nchan, nbin, freqs, code, nu_ref, dc, tau_rot, alpha, ngauss, comps, dout);
    }, nullptr, 0, slot);
}

// ---- spline (PCA + B-spline) templates on the device --------------------------
static int spline_generate(pp_ctx* c, int nchan, int nbin, const double* freqs, int ncomp, const double* basis,
                           int nknots, const double* t, const double* coefs, int degree, double* dev_out) {
    if (!freqs || !basis || (ncomp > 0 && (!t || !coefs))) return fail(PP_EINVAL, "spline portrait: null argument");
    if (nbin < 2 || nchan < 1) return fail(PP_EINVAL, "spline portrait: bad shape");
    if (ncomp < 0 || ncomp > PP_MAX_SPLINE_COMP) return fail(PP_EINVAL, "spline portrait: 0..%d components", PP_MAX_SPLINE_COMP);
    if (ncomp > 0 && (degree < 1 || degree > PP_MAX_SPLINE_DEG || nknots < 2 * (degree + 1)))
        return fail(PP_EINVAL, "spline portrait: degree %d with %d knots", degree, nknots);
    int rc;
    if ((rc = upload(c, c->freqs, freqs, (size_t)nchan * 8))) return rc;
    const size_t nb = (size_t)(ncomp + 1) * nbin, nt = (size_t)std::max(nknots, 1), ncf = (size_t)std::max(ncomp, 1) * nt;
    if ((rc = c->seedbuf.reserve((nb + nt + ncf) * 8))) return rc;
    double* dbasis = c->seedbuf.as<double>();
    double* dt = dbasis + nb;
    double* dc = dt + nt;
    HIP_TRY(hipMemcpyAsync(dbasis, basis, nb * 8, hipMemcpyHostToDevice, c->stream));
    if (ncomp > 0) {
        HIP_TRY(hipMemcpyAsync(dt, t, (size_t)nknots * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(dc, coefs, (size_t)ncomp * nknots * 8, hipMemcpyHostToDevice, c->stream));
    }
    SplineArgs a{c->freqs.as<double>(), dbasis, dt, dc, dev_out, nchan, nbin, ncomp, nknots, degree};
    {
        Prof pr(c, KF_MODEL);
        hipLaunchKernelGGL(k_spline_portrait, dim3(nchan), dim3(256), 0, c->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return PP_OK;
}

extern "C" int pp_spline_portrait(pp_ctx* c, int nchan, int nbin, const double* freqs, int ncomp,
                                  const double* basis, int nknots, const double* t, const double* coefs,
                                  int degree, double* portrait, int out_on_device) {
    if (int busy_ = ctx_busy(c, "pp_spline_portrait")) return busy_;
    if (!c || !portrait) return fail(PP_EINVAL, "pp_spline_portrait: null argument");
    HIP_TRY(hipSetDevice(c->device));
    return generated_template(c, nchan, nbin, [&](double* dout) {
        return spline_generate(c, nchan, nbin, freqs, ncomp, basis, nknots, t, coefs, degree, dout);
    }, portrait, out_on_device, -1);
}

extern "C" int pp_model_set_spline(pp_ctx* c, int slot, int nchan, int nbin, const double* freqs, int ncomp,
                                   const double* basis, int nknots, const double* t, const double* coefs,
                                   int degree) {
    if (int busy_ = ctx_busy(c, "pp_model_set_spline")) return busy_;
    if (!c) return fail(PP_EINVAL, "pp_model_set_spline: null context");
    if (!nbin_any_ok(nbin)) return nbin_refuse("pp_model_set_spline", nbin);
    HIP_TRY(hipSetDevice(c->device));
    return generated_template(c, nchan, nbin, [&](double* dout) {
        return spline_generate(c, nchan, nbin, freqs, ncomp, basis, nknots, t, coefs, degree, dout);
    }, nullptr, 0, slot);
}

// ---- instrumental response applied to a resident template ---------------------
extern "C" int pp_model_apply_response(pp_ctx* c, int slot, const double* rconst, const double* smear_wid) {
    if (int busy_ = ctx_busy(c, "pp_model_apply_response")) return busy_;
    if (!c || slot < 0 || slot >= PP_MAX_SLOTS || !c->slots[slot].set)
        return fail(PP_ESTATE, "pp_model_apply_response: slot not set");
    if (!rconst && !smear_wid) return PP_OK;
    HIP_TRY(hipSetDevice(c->device));
    ModelSlot& s = c->slots[slot];
    const int M = s.nbin / 2;
    int rc;
    const cplx* drc = nullptr;
    const double* dwid = nullptr;
    if (rconst) {
        if ((rc = upload(c, c->seedbuf, rconst, (size_t)(M + 1) * 16))) return rc;
        drc = c->seedbuf.as<cplx>();
    }
    if (smear_wid) {
        if ((rc = upload(c, c->errs, smear_wid, (size_t)s.nchan * 8))) return rc;
        dwid = c->errs.as<double>();
    }
    {
        Prof pr(c, KF_MODEL);
        hipLaunchKernelGGL(k_model_response, dim3(s.nchan), dim3(256), 0, c->stream, s.mft.as<cplx>(),
                           s.msq.as<double>(), s.msum.as<double>(), s.mmax.as<double>(), s.mdc.as<double>(), drc,
                           dwid, s.nchan, M, s.Mp);
    }
    HIP_TRY(hipGetLastError());
    return model_publish(c, slot);
}

// ---- time / frequency / polarisation scrunching (pp_scrunch.h) -----------------
// The run [in.nsub subints from subint s0] of a pp_scrunch call: the member lists of the time groups gt_lo .. that
// meet it, in ascending (subint, channel) order, and the pass.  `out`: where those groups' rows are (group gt_lo first)
static int scrunch_run(pp_ctx* c, const Ports& in, int s0, const void* dsrc, const double* weights, const int32_t* t_off,
                       int ngf, const int32_t* f_off, int pol_mode, int gt_lo, int gt_hi, const double* wtot, double* out) {
    const int n = in.nsub, nchan = in.nchan, npol = in.npol, ngt = gt_hi - gt_lo + 1;
    const int npo = pol_mode == PP_POL_KEEP ? npol : 1;
    std::vector<ScrunchMember> mem;
    std::vector<int> meta((size_t)ngt * ngf + 1 + ngt);         // off[ngt ngf + 1], then tflag[ngt]
    int* off = meta.data();
    int* tflag = off + (size_t)ngt * ngf + 1;
    off[0] = 0;
    for (int g = 0; g < ngt; ++g) {
        const int gt = gt_lo + g;
        const int sa = std::max((int)t_off[gt], s0), sb = std::min((int)t_off[gt + 1], s0 + n);
        tflag[g] = (t_off[gt] < s0 ? 1 : 0) | (t_off[gt + 1] <= s0 + n ? 2 : 0);
        for (int gf = 0; gf < ngf; ++gf) {
            if (wtot[(size_t)gt * ngf + gf] > 0.0)
                for (int s = sa; s < sb; ++s)
                    for (int ch = f_off[gf]; ch < f_off[gf + 1]; ++ch) {
                        const double w = weights[(size_t)s * nchan + ch];
                        if (w == 0.0 || w != w) continue;
                        mem.push_back(ScrunchMember{w, ((long long)(s - s0) * npol) * nchan + ch});
                    }
            off[(size_t)g * ngf + gf + 1] = (int)mem.size();
        }
    }
    int rc;
    if (!mem.empty()) if ((rc = upload(c, c->seedbuf, mem.data(), mem.size() * sizeof(ScrunchMember)))) return rc;
    if ((rc = upload(c, c->misc, meta.data(), meta.size() * sizeof(int)))) return rc;
    if ((rc = upload(c, c->sdraw, wtot + (size_t)gt_lo * ngf, (size_t)ngt * ngf * 8))) return rc;
    ScrunchArgs a{dsrc, out, c->seedbuf.as<ScrunchMember>(), c->misc.as<int>(), c->sdraw.as<double>(),
                  c->misc.as<int>() + (size_t)ngt * ngf + 1, ngt, npo, ngf, nchan, in.nbin};
    // one thread per 16 input bytes of an output row; outputs too small to give every compute unit a 256-thread
    // workgroup go out as single waves
    const int V = 16 / (int)in.esz();
    const long long nitems = (long long)ngt * npo * ngf * ((in.nbin + V - 1) / V);
    const int T = nitems >= 256LL * std::max(c->ncu, 1) ? 256 : 64;
    const unsigned grid = (unsigned)std::min<long long>((nitems + T - 1) / T, 1LL << 22);
    {
        Prof pr(c, KF_SCRUNCH);
        with_dtype(in.dtype, [&](auto t) {
            if (pol_mode == PP_POL_SUM01) hipLaunchKernelGGL((k_scrunch<decltype(t), true>), dim3(grid), dim3(T), 0, c->stream, a);
            else hipLaunchKernelGGL((k_scrunch<decltype(t), false>), dim3(grid), dim3(T), 0, c->stream, a);
        });
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));      // (the lists are free again)
    return PP_OK;
}

extern "C" int pp_scrunch(pp_ctx* c, const void* src, int dtype, int on_device, int nsub, int npol, int nchan, int nbin,
                          const double* weights, int ngt, const int32_t* t_off, int ngf, const int32_t* f_off,
                          int pol_mode, double* dst, double* wout) {
    if (int busy_ = ctx_busy(c, "pp_scrunch")) return busy_;
    if (!c || !src || !weights || !t_off || !f_off || !dst || !wout) return fail(PP_EINVAL, "pp_scrunch: null argument");
    if (!nbin_any_ok(nbin)) return nbin_refuse("pp_scrunch", nbin);
    if (nsub < 1 || npol < 1 || nchan < 1 || (long long)nsub * nchan > INT_MAX) return fail(PP_EINVAL, "pp_scrunch: bad shape");
    if (dtype != PP_F64 && dtype != PP_F32) return fail(PP_EINVAL, "pp_scrunch: dtype %d", dtype);
    if (on_device && (((uintptr_t)src & 7) || ((uintptr_t)dst & 15)))
        return fail(PP_EINVAL, "pp_scrunch: a device src must be 8-byte aligned and a device dst 16-byte aligned");
    if (pol_mode != PP_POL_KEEP && pol_mode != PP_POL_SUM01 && pol_mode != PP_POL_FIRST) return fail(PP_EINVAL, "pp_scrunch: pol_mode %d", pol_mode);
    if (pol_mode == PP_POL_SUM01 && npol < 2) return fail(PP_EINVAL, "pp_scrunch: PP_POL_SUM01 needs two polarisations, the input has %d", npol);
    auto offsets_ok = [](const int32_t* o, int ng, int n) {
        if (ng < 1 || ng > n || o[0] != 0 || o[ng] != n) return false;
        for (int g = 0; g < ng; ++g) if (o[g + 1] <= o[g]) return false;
        return true;
    };
    if (!offsets_ok(t_off, ngt, nsub)) return fail(PP_EINVAL, "pp_scrunch: t_off must ascend strictly from 0 to nsub = %d in %d groups", nsub, ngt);
    if (!offsets_ok(f_off, ngf, nchan)) return fail(PP_EINVAL, "pp_scrunch: f_off must ascend strictly from 0 to nchan = %d in %d groups", nchan, ngf);
    HIP_TRY(hipSetDevice(c->device));
    // total weights: the members' sequential sum, on the host (the weights are here)
    for (int gt = 0; gt < ngt; ++gt)
        for (int gf = 0; gf < ngf; ++gf) {
            double W = 0.0;
            for (int s = t_off[gt]; s < t_off[gt + 1]; ++s)
                for (int ch = f_off[gf]; ch < f_off[gf + 1]; ++ch) {
                    const double w = weights[(size_t)s * nchan + ch];
                    if (!(w == 0.0 || w != w)) W += w;
                }
            wout[(size_t)gt * ngf + gf] = W > 0.0 ? W : 0.0;
        }
    const Ports in{src, dtype, on_device, nsub, nchan, nbin, nullptr, 0, nullptr, nullptr, 0, npol};
    const int npo = pol_mode == PP_POL_KEEP ? npol : 1;
    const size_t slab = (size_t)npo * ngf * nbin;           // doubles of one time group's output
    int rc;
    if (on_device) return scrunch_run(c, in, 0, src, weights, t_off, ngf, f_off, pol_mode, 0, ngt - 1, wout, dst);
    // a host input goes through in runs of whole subints; a run of n subints meets at most n time groups, whose
    // rows it holds in c->X.  A group that goes on into the next run moves to the front of that buffer.  Only the
    // polarisations the mode reads cross to the device -- the first (PP_POL_FIRST) or the first two (PP_POL_SUM01) of
    // every subint, by a pitched copy --, so the run on the device has `dpol` of them
    const int dpol = pol_mode == PP_POL_FIRST ? 1 : pol_mode == PP_POL_SUM01 ? 2 : npol;
    const Ports din{src, dtype, 0, nsub, nchan, nbin, nullptr, 0, nullptr, nullptr, 0, dpol};
    const int cap = din.cap(c, (double)slab * 8 + 24.0 * nchan);
    if ((rc = c->X.reserve((size_t)std::min(cap, ngt) * slab * 8))) return rc;
    int gt = 0;                                             // the first group the next run meets
    return for_runs(nsub, cap, [&](Run r) {
        Ports run = din;
        run.nsub = r.n;
        int rc, gt_hi = gt;
        while (t_off[gt_hi + 1] < r.s0 + r.n) ++gt_hi;
        if ((rc = c->data.reserve((size_t)r.n * din.sub_bytes()))) return rc;
        HIP_TRY(hipMemcpy2DAsync(c->data.p, din.sub_bytes(), r.at((const char*)src, in.sub_bytes()), in.sub_bytes(), din.sub_bytes(),
                                 (size_t)r.n, hipMemcpyHostToDevice, c->stream));
        if ((rc = scrunch_run(c, run, r.s0, c->data.p, weights, t_off, ngf, f_off, pol_mode, gt, gt_hi, wout, c->X.as<double>()))) return rc;
        const bool open = t_off[gt_hi + 1] > r.s0 + r.n;     // the last group goes on
        const int ndone = gt_hi - gt + (open ? 0 : 1);
        if (ndone) HIP_TRY(hipMemcpyAsync(dst + (size_t)gt * slab, c->X.p, (size_t)ndone * slab * 8, hipMemcpyDeviceToHost, c->stream));
        if (open && gt_hi > gt)
            HIP_TRY(hipMemcpyAsync(c->X.p, c->X.as<double>() + (size_t)(gt_hi - gt) * slab, slab * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        gt = open ? gt_hi : gt_hi + 1;
        return (int)PP_OK;
    });
}
