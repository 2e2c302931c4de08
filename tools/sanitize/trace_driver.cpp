// Walks the HOST driver of libpptoas_hip.so through a matrix of small batches against the no-op HIP stub
// (hip_stub.cpp with PP_STUB_TRACE set): every flow, entry point and option once, so that the stub's trace -- every
// launch, copy, memset, event and wait in the order the library queues them -- can be compared between two builds of
// the library (make trace-run; a refactor of the driver must leave the trace byte-identical).  Single-threaded, C ABI
// only: the same source builds against any commit's library.  Kernels do not run and the stub's device memory is all
// zeros, so every host decision that reads a device count sees "all done": the weak-pilot re-seed, the recentre loop,
// the re-transform of listed subints and the re-fit on collect are NOT reached here (the GPU suite asserts those).
// aux_cases() walks the auxiliary entry points the same way, and checks where their outputs land.
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/pp_toas.h"

static void (*g_mark)(const char*) = nullptr;
static void mark(const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g_mark) g_mark(buf);
}
#define MUST(x) do { int rc_ = (x); if (rc_ != PP_OK) { fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc_, pp_last_error()); exit(1); } } while (0)

struct Spec {
    int ns = 3, C = 256, B = 2048;
    int f32 = 0, noerrs = 0, mask = 0, slot = -1, fstride = 0, chanout = 0, objout = 0;
    int gm = 0, scat = 0, log10tau = 0, method = PP_METHOD_TRUST_NCG, seed_ns = 0, refseed = 0;
};

struct Batch {
    Spec s;
    std::vector<double> d64, freqs, errs, P, x0, nufit, numean, mprof;
    std::vector<float> d32;
    std::vector<uint8_t> mask;
    std::vector<int32_t> slot, nfev, rcode, npass;
    std::vector<double> params, perr, nu, cov, chi2, rchi2, snr, seedph, scales, serrs, csnr, f0, g0, H0;
    double duration = 0;
    pp_seed_ref rs;
    pp_fit_in in;
    pp_fit_out out;
    explicit Batch(const Spec& sp) : s(sp) {
        const int ns = s.ns, C = s.C, B = s.B;
        const size_t n = (size_t)ns * C * B;
        if (s.f32) d32.assign(n, 0.5f); else d64.assign(n, 0.5);
        freqs.resize(s.fstride ? (size_t)ns * C : (size_t)C);
        for (size_t j = 0; j < freqs.size(); ++j) freqs[j] = 1100.0 + 800.0 * ((j % C) + 0.5) / C;
        errs.assign((size_t)ns * C, 0.05); P.assign(ns, 0.003); x0.assign((size_t)ns * 5, 0.0);
        nufit.assign((size_t)ns * 3, 1500.0); numean.assign(ns, 1500.0); mprof.assign(B, 1.0);
        if (s.scat) for (int i = 0; i < ns; ++i) { x0[(size_t)i * 5 + 3] = s.log10tau ? -3.0 : 1e-3; x0[(size_t)i * 5 + 4] = -4.0; }
        if (s.mask) { mask.assign((size_t)ns * C, 1); for (size_t j = 0; j < mask.size(); j += 7) mask[j] = 0; }
        if (s.slot >= 0) slot.assign(ns, s.slot);
        params.resize((size_t)ns * 5); perr.resize((size_t)ns * 5); nu.resize((size_t)ns * 3); cov.resize((size_t)ns * 25);
        chi2.resize(ns); rchi2.resize(ns); snr.resize(ns); seedph.resize(ns); nfev.resize(ns); rcode.resize(ns); npass.resize(ns);
        memset(&in, 0, sizeof in); memset(&out, 0, sizeof out); memset(&rs, 0, sizeof rs);
        in.nsub = ns; in.nchan = C; in.nbin = B;
        in.data = s.f32 ? (const void*)d32.data() : (const void*)d64.data(); in.data_dtype = s.f32 ? PP_F32 : PP_F64;
        in.model_slot = s.slot >= 0 ? slot.data() : nullptr;
        in.freqs = freqs.data(); in.freqs_stride = s.fstride ? C : 0;
        in.errs = s.noerrs ? nullptr : errs.data(); in.chan_mask = s.mask ? mask.data() : nullptr;
        in.P = P.data(); in.init_params = x0.data(); in.nu_fits = s.fstride ? nullptr : nufit.data();
        in.fit_flags[0] = in.fit_flags[1] = 1; in.fit_flags[2] = s.gm; in.fit_flags[3] = s.scat; in.fit_flags[4] = 0;
        in.log10_tau = s.log10tau; in.is_toa = 1; in.method = s.method; in.seed_ns = s.seed_ns;
        if (s.refseed) {
            rs.model_profs = mprof.data(); rs.nu_mean = numean.data(); rs.lo = -0.5; rs.hi = 0.5; rs.Ns = 100; rs.finish = 1;
            rs.seed_phase = seedph.data();
            in.ref_seed = &rs;
        }
        out.params = params.data(); out.param_errs = perr.data(); out.nu_refs = nu.data(); out.cov = cov.data();
        out.chi2 = chi2.data(); out.red_chi2 = rchi2.data(); out.snr = snr.data(); out.nfeval = nfev.data();
        out.return_code = rcode.data(); out.npass = npass.data(); out.duration = &duration;
        if (s.chanout) {
            scales.resize((size_t)ns * C); serrs.resize((size_t)ns * C); csnr.resize((size_t)ns * C);
            out.scales = scales.data(); out.scale_errs = serrs.data(); out.channel_snrs = csnr.data();
        }
        if (s.objout) {
            f0.resize(ns); g0.resize((size_t)ns * 5); H0.resize((size_t)ns * 25);
            out.obj_f = f0.data(); out.obj_grad = g0.data(); out.obj_hess = H0.data();
        }
    }
};

// a context with a template of shape C x B in slots 0 and 1
static void set_model(pp_ctx* c, int slot, int C, int B) {
    std::vector<double> model((size_t)C * B, 0.0);
    for (int n = 0; n < C; ++n) for (int b = 0; b < B; ++b) model[(size_t)n * B + b] = (b % 7) * 0.1 + n * 1e-3;
    MUST(pp_model_set(c, slot, model.data(), PP_F64, 0, C, B));
}
static pp_ctx* make_ctx(int C, int B) {
    pp_ctx* c = nullptr;
    MUST(pp_create(0, &c));
    set_model(c, 0, C, B);
    set_model(c, 1, C, B);
    return c;
}

enum Entry { SYNC, SUBMIT, ENQUEUE };
// one batch by one entry point on a context of its shape; the return code goes into the trace
static void run_on(pp_ctx* c, const char* name, const Spec& s, Entry e = SYNC) {
    Batch b(s);
    mark("case %s", name);
    int rc;
    if (e == SUBMIT) { rc = pp_fit_submit(c, &b.in, &b.out); if (rc == PP_OK) rc = pp_fit_wait(c); }
    else if (e == ENQUEUE) { rc = pp_fit_enqueue(c, &b.in, &b.out); if (rc == PP_OK) rc = pp_fit_collect(c); }
    else rc = pp_fit_portrait_batch(c, &b.in, &b.out);
    mark("rc %d", rc);
}
static void run(const char* name, const Spec& s, Entry e = SYNC) {
    pp_ctx* c = make_ctx(s.C, s.B);
    run_on(c, name, s, e);
    MUST(pp_destroy(c));
}

// the flows of one shape: inputs, fit flags, seeds
static void shape_cases(int B, int C) {
    char nm[128];
    pp_ctx* c = make_ctx(C, B);
    int k = 0;
    auto go = [&](const char* what, Spec s) {
        s.B = B; s.C = C; s.ns = 2 + (k++ % 4);
        snprintf(nm, sizeof nm, "%dx%d %s", C, B, what);
        run_on(c, nm, s);
    };
    { Spec s; go("phiDM f64", s); }
    { Spec s; s.f32 = 1; go("phiDM f32", s); }
    { Spec s; s.noerrs = 1; go("phiDM noise measured", s); }
    { Spec s; s.f32 = 1; s.noerrs = 1; go("phiDM f32 noise measured", s); }
    { Spec s; s.mask = 1; go("phiDM mask", s); }
    { Spec s; s.mask = 1; s.noerrs = 1; s.slot = 1; s.fstride = 1; s.chanout = 1; go("phiDM mask noise measured slot freqs_stride channel outputs", s); }
    { Spec s; s.gm = 1; go("phiDMGM", s); }
    { Spec s; s.gm = 1; s.method = PP_METHOD_NEWTON; s.f32 = 1; go("phiDMGM newton f32", s); }
    { Spec s; s.scat = 1; s.log10tau = 1; go("scat trust-ncg log10_tau", s); }
    { Spec s; s.scat = 1; go("scat trust-ncg", s); }
    { Spec s; s.scat = 1; s.method = PP_METHOD_NEWTON; go("scat newton", s); }
    { Spec s; s.scat = 1; s.method = PP_METHOD_NEWTON; s.log10tau = 1; s.f32 = 1; s.mask = 1; go("scat newton log10_tau f32 mask", s); }
    { Spec s; s.scat = 1; s.noerrs = 1; go("scat trust-ncg noise measured", s); }
    { Spec s; s.seed_ns = 100; go("seed_ns", s); }
    { Spec s; s.seed_ns = 100; s.noerrs = 1; s.mask = 1; go("seed_ns noise measured mask", s); }
    { Spec s; s.seed_ns = 100; s.scat = 1; go("seed_ns scat", s); }
    { Spec s; s.refseed = 1; go("ref_seed", s); }                    // (refused where no single-pass path exists: rc -5)
    { Spec s; s.refseed = 1; s.f32 = 1; s.mask = 1; go("ref_seed f32 mask", s); }
    { Spec s; s.refseed = 1; s.scat = 1; go("ref_seed scat", s); }
    { Spec s; s.refseed = 1; s.noerrs = 1; go("ref_seed without errs (refused)", s); }
    MUST(pp_destroy(c));
}

static void entry_cases() {
    { Spec s; s.ns = 5; pp_ctx* c = make_ctx(s.C, s.B); MUST(pp_set_option(c, "max_work_bytes", 1e7)); run_on(c, "entry sub-batched", s); MUST(pp_destroy(c)); }
    { Spec s; s.ns = 5; s.scat = 1; pp_ctx* c = make_ctx(s.C, s.B); MUST(pp_set_option(c, "max_work_bytes", 1e7)); run_on(c, "entry sub-batched scat enqueue", s, ENQUEUE); MUST(pp_destroy(c)); }
    // (a wide band with seed_chan_stride = 1, i.e. no pilot: ref_seed without scattering has no single-pass path)
    { Spec s; s.C = 2304; s.refseed = 1; pp_ctx* c = make_ctx(s.C, s.B); MUST(pp_set_option(c, "seed_chan_stride", 1)); run_on(c, "entry ref_seed refused at seed_chan_stride=1", s); MUST(pp_destroy(c)); }
    { Spec s; run("entry submit/wait", s, SUBMIT); }
    { Spec s; s.scat = 1; run("entry submit/wait scat", s, SUBMIT); }
    { Spec s; run("entry enqueue/collect", s, ENQUEUE); }
    { Spec s; s.refseed = 1; run("entry enqueue/collect ref_seed", s, ENQUEUE); }
}

// pp_fit_enqueue three deep over a mixed sequence, pp_synchronize and pp_fit_collect interleaved.  Slots: 0 = 256 x 2048,
// 1 = 48 x 2048 (the small batch behind a large one: fewer waves than half the carried tickets), 2 = 256 x 1024
static void chain(const char* name, const char* opt = nullptr, double val = 0) {
    pp_ctx* c = nullptr;
    MUST(pp_create(0, &c));
    set_model(c, 0, 256, 2048); set_model(c, 1, 48, 2048); set_model(c, 2, 256, 1024);
    if (opt) MUST(pp_set_option(c, opt, val));
    Spec plain, plain32, refs, refscat, big, small_, b1024, scat, seeded;
    plain32.f32 = 1; plain32.mask = 1; refs.refseed = 1; refscat.refseed = 1; refscat.scat = 1;
    big.C = 48; big.slot = 1; big.ns = 200; small_.C = 48; small_.slot = 1; small_.ns = 2;
    b1024.B = 1024; b1024.slot = 2; scat.scat = 1; seeded.seed_ns = 100;
    const Spec* seq[] = {&plain, &plain32, &refs, &plain, &big, &small_, &plain, &b1024, &plain, &refs, &refs, &scat, &plain,
                         &refscat, &refs, &seeded, &plain, &plain};
    const int nseq = (int)(sizeof seq / sizeof seq[0]);
    mark("case %s", name);
    std::vector<Batch*> live;
    for (int r = 0; r < nseq; ++r) {
        Spec s = *seq[r];
        if (s.ns == 3) s.ns = 2 + r % 4;
        Batch* b = new Batch(s);
        int rc = pp_fit_enqueue(c, &b->in, &b->out);
        mark("enqueue %d rc %d pending %d", r, rc, pp_fit_pending(c));
        if (rc == PP_OK) live.push_back(b); else delete b;
        if (r % 5 == 4) { rc = pp_synchronize(c); mark("synchronize rc %d", rc); }
        if (live.size() >= 3 || r % 7 == 6) {
            while (live.size() >= 3 || (r % 7 == 6 && !live.empty())) {
                rc = pp_fit_collect(c); mark("collect rc %d", rc);
                delete live.front(); live.erase(live.begin());
            }
        }
    }
    while (!live.empty()) { int rc = pp_fit_collect(c); mark("collect rc %d", rc); delete live.front(); live.erase(live.begin()); }
    MUST(pp_destroy(c));
}

// every option once from its default, over one batch of each flow (and the chain for those that touch deferred batches)
static void option_cases() {
    struct Opt { const char* name; double val; const char* name2; double val2; };
    const Opt opts[] = {
        {"taylor", 0, nullptr, 0}, {"moments_in_xspec", 0, nullptr, 0}, {"one_exchange", 0, nullptr, 0}, {"paired_split", 0, nullptr, 0},
        {"fuse_scat", 0, nullptr, 0}, {"scat_model", 0, nullptr, 0}, {"scat_model", 2, nullptr, 0}, {"x_f32", 1, nullptr, 0},
        {"x_pad", 8, nullptr, 0}, {"coarse_newton", 0, nullptr, 0}, {"lagged_check", 0, nullptr, 0}, {"copy_kernels", 0, nullptr, 0},
        {"overlap_post", 1, nullptr, 0}, {"fuse_tail", 0, nullptr, 0}, {"tail_virtual", 1, nullptr, 0}, {"finalize_regs", 0, nullptr, 0},
        {"skip_masked", 0, nullptr, 0}, {"seed_ndm", 3, "seed_dm_step", 1e-3}, {"solve_threads", 128, nullptr, 0},
        {"debug_poison", 255, nullptr, 0}, {"profile", 1, nullptr, 0}, {"max_iter", 0, nullptr, 0},
    };
    char nm[160];
    for (const Opt& o : opts) {
        for (int C : {256, 640}) {
            pp_ctx* c = make_ctx(C, 2048);
            MUST(pp_set_option(c, o.name, o.val));
            if (o.name2) MUST(pp_set_option(c, o.name2, o.val2));
            int k = 0;
            auto go = [&](const char* what, Spec s, Entry e = SYNC) {
                s.C = C; s.ns = 2 + (k++ % 4); s.objout = 1;
                snprintf(nm, sizeof nm, "option %s=%g %dx2048 %s", o.name, o.val, C, what);
                run_on(c, nm, s, e);
            };
            { Spec s; go("phiDM", s); }
            { Spec s; s.f32 = 1; s.mask = 1; s.noerrs = 1; s.chanout = 1; go("phiDM f32 mask noise measured", s); }
            { Spec s; s.scat = 1; go("scat trust-ncg", s); }
            { Spec s; s.scat = 1; s.method = PP_METHOD_NEWTON; go("scat newton", s); }
            { Spec s; s.seed_ns = 100; go("seed_ns", s); }
            { Spec s; s.refseed = 1; go("ref_seed", s); }
            { Spec s; s.refseed = 1; s.scat = 1; go("ref_seed scat", s); }
            { Spec s; go("phiDM enqueue", s, ENQUEUE); }
            MUST(pp_destroy(c));
        }
        snprintf(nm, sizeof nm, "option %s=%g chain", o.name, o.val);
        chain(nm, o.name, o.val);
    }
}

// ---- the auxiliary entry points (everything in the C ABI that is no fit) ----------------------------------------
// Host arrays are sized exactly (a write past one is AddressSanitizer's to catch: make asan-run) and every output is
// all 0xFF bytes -- NaN for floating point -- before the call.  The stub really copies and its device memory is
// zeros, so after a successful call a D2H that landed where it should has left no such element: that pins the output
// offsets of the runs a large host input is split into.  A refused call marks its code AND its message.
struct Outs {
    struct A { unsigned char* p; size_t n, elem; };
    std::vector<A> v;
    void* raw(size_t n, size_t elem) {
        unsigned char* p = new unsigned char[n * elem];
        memset(p, 0xFF, n * elem);
        v.push_back({p, n, elem});
        return p;
    }
    double* d(size_t n) { return (double*)raw(n, 8); }
    ~Outs() { for (A& a : v) delete[] a.p; }
    void require_filled(const char* what) const {
        for (size_t k = 0; k < v.size(); ++k)
            for (size_t i = 0; i < v[k].n; ++i) {
                size_t ff = 0;
                for (size_t b = 0; b < v[k].elem; ++b) ff += v[k].p[i * v[k].elem + b] == 0xFF;
                if (ff == v[k].elem) { fprintf(stderr, "%s: output %zu, element %zu of %zu was not written\n", what, k, i, v[k].n); exit(1); }
            }
    }
};
static int g_ncase = 0;
// the end of one call: its code, its message when refused, its outputs when not
static void done(const char* what, int rc, const Outs& o) {
    mark("rc %d", rc);
    if (rc != PP_OK) mark("err %s", pp_last_error());
    else o.require_filled(what);
}
#define AUX(o, what, call) do { mark("case aux %s", what); ++g_ncase; done(what, (call), o); } while (0)

// "device" memory of the stub is host memory: a copy of a host array as an on_device input
static void* dev_copy(const void* h, size_t bytes) {
    static auto mal = (int (*)(void**, size_t))dlsym(RTLD_DEFAULT, "hipMalloc");
    void* p = nullptr;
    if (!mal || mal(&p, bytes) != 0) { fprintf(stderr, "trace_driver: no hipMalloc (the stub is not loaded)\n"); exit(1); }
    if (h) memcpy(p, h, bytes);
    return p;
}
static void dev_free(void* p) {
    static auto fr = (int (*)(void*))dlsym(RTLD_DEFAULT, "hipFree");
    if (fr) fr(p);
}

struct AuxCfg { int B, C, ns, f32, dev, fstride, slot, small; };
// the inputs of one configuration, every array exactly as long as the entry points read
struct AuxIn {
    AuxCfg k;
    size_t esz, nrow;
    std::vector<unsigned char> ports;      // [ns][C][B] of the dtype
    void* dports = nullptr;
    std::vector<double> freqs, P, par3, params5, nus3, w, mprof, scales, errs;
    std::vector<int32_t> slots;
    explicit AuxIn(const AuxCfg& kk) : k(kk), esz(kk.f32 ? 4 : 8), nrow((size_t)kk.ns * kk.C) {
        const int ns = k.ns, C = k.C, B = k.B;
        ports.resize(nrow * B * esz);
        for (size_t j = 0; j < nrow * B; ++j) {
            const double v = 0.5 + (j % 13) * 0.01;
            if (k.f32) ((float*)ports.data())[j] = (float)v; else ((double*)ports.data())[j] = v;
        }
        if (k.dev) dports = dev_copy(ports.data(), ports.size());
        freqs.resize(k.fstride ? nrow : (size_t)C);
        for (size_t j = 0; j < freqs.size(); ++j) freqs[j] = 1100.0 + 800.0 * ((j % C) + 0.5) / C + (j / C);
        P.assign(ns, 0.003); par3.assign((size_t)ns * 3, 0.0); params5.assign((size_t)ns * 5, 0.0); nus3.assign((size_t)ns * 3, 1500.0);
        for (int i = 0; i < ns; ++i) { par3[(size_t)i * 3] = 0.01 * i; par3[(size_t)i * 3 + 2] = 1500.0; params5[(size_t)i * 5] = 0.01 * i; }
        w.assign(nrow, 1.0); mprof.assign((size_t)ns * B, 1.0); scales.assign(nrow, 1.0); errs.assign(nrow, 0.05);
        if (k.slot) { slots.resize(ns); for (int i = 0; i < ns; ++i) slots[i] = i % 2; }
    }
    ~AuxIn() { if (dports) dev_free(dports); }
    const void* src() const { return k.dev ? dports : (const void*)ports.data(); }
    int dtype() const { return k.f32 ? PP_F32 : PP_F64; }
    int64_t fstride() const { return k.fstride ? k.C : 0; }
    const int32_t* slot() const { return k.slot ? slots.data() : nullptr; }
};

// the four entry points that take portraits plus per-subint arrays: every configuration
static void aux_ports_calls(pp_ctx* c, const AuxCfg& k, const char* tag) {
    AuxIn in(k);
    const int ns = k.ns, C = k.C, B = k.B;
    char nm[200];
    auto name = [&](const char* fn) {
        snprintf(nm, sizeof nm, "%s %s %dx%dx%d %s %s fstride=%d slot=%d", fn, tag, ns, C, B, k.f32 ? "f32" : "f64", k.dev ? "device" : "host",
                 (int)in.fstride(), k.slot);
        return nm;
    };
    { Outs o; double* out7 = o.d((size_t)ns * 7);
      AUX(o, name("pp_reference_phase_seed"), pp_reference_phase_seed(c, in.src(), in.dtype(), k.dev, ns, C, B, in.freqs.data(), in.fstride(), in.P.data(),
          in.par3.data(), k.slot ? 1500.0 : INFINITY, k.slot ? 1400.0 : INFINITY, in.w.data(), in.mprof.data(), -0.5, 0.5, 20, out7)); }
    { Outs o; void* dst = k.dev ? in.dports : o.raw(in.nrow * B, in.esz);
      AUX(o, name("pp_rotate_portraits"), pp_rotate_portraits(c, in.src(), dst, in.dtype(), k.dev, ns, C, B, in.freqs.data(), in.fstride(), in.P.data(),
          in.par3.data(), k.slot ? 1500.0 : INFINITY, INFINITY)); }
    { Outs o; double* al = o.d((size_t)C * B); double* tw = o.d(C);
      AUX(o, name("pp_align_accumulate"), pp_align_accumulate(c, in.src(), in.dtype(), k.dev, ns, C, B, in.freqs.data(), in.fstride(), in.P.data(),
          in.par3.data(), in.w.data(), al, tw)); }
    { Outs o; double* rc2 = o.d(in.nrow);
      AUX(o, name("pp_channel_red_chi2"), pp_channel_red_chi2(c, in.src(), in.dtype(), k.dev, ns, C, B, in.slot(), in.freqs.data(), in.fstride(), in.P.data(),
          in.params5.data(), in.nus3.data(), in.scales.data(), in.errs.data(), rc2)); }
    // pp_fit_residuals: all four outputs, the residual alone (no errs), and the model with chi^2 under a mask that
    // drops the first and the last row; outputs live where the input lives
    std::vector<double> mask(in.nrow, 1.0);
    mask[0] = 0.0; mask[in.nrow - 1] = NAN;
    for (int variant = 0; variant < 3; ++variant) {
        Outs o;
        const bool want[4] = {variant == 0, variant != 1, variant != 2, variant != 1};      // port, model, resid, red_chi2
        void* out[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < 4; ++j) {
            if (!want[j]) continue;
            const size_t n = j == 3 ? in.nrow : in.nrow * B, elem = j == 3 ? 8 : in.esz;
            out[j] = k.dev ? dev_copy(nullptr, n * elem) : o.raw(n, elem);
        }
        static const char* names[3] = {"pp_fit_residuals all", "pp_fit_residuals resid", "pp_fit_residuals model chi2 masked"};
        AUX(o, name(names[variant]), pp_fit_residuals(c, in.src(), in.dtype(), k.dev, ns, C, B, in.slot(), in.freqs.data(), in.fstride(), in.P.data(),
            in.params5.data(), in.nus3.data(), in.scales.data(), variant == 1 ? nullptr : in.errs.data(), variant == 2 ? mask.data() : nullptr,
            variant % 2, out[0], out[1], out[2], (double*)out[3]));
        if (k.dev) for (int j = 0; j < 4; ++j) if (out[j]) dev_free(out[j]);
    }
}

// the entry points that take rows: dtype and where the rows are
static void aux_rows_calls(pp_ctx* c, const AuxCfg& k, const char* tag) {
    AuxIn in(k);
    const int ns = k.ns, C = k.C, B = k.B, nrows = ns * C;
    char nm[200];
    auto name = [&](const char* fn) {
        snprintf(nm, sizeof nm, "%s %s %dx%d %s %s", fn, tag, nrows, B, k.f32 ? "f32" : "f64", k.dev ? "device" : "host");
        return nm;
    };
    for (int method : {PP_NORM_NONE, PP_NORM_PROF}) {
        Outs o; double* norms = o.d(nrows); double* noise = o.d(nrows);
        AUX(o, name(method == PP_NORM_PROF ? "pp_channel_noise prof" : "pp_channel_noise"),
            pp_channel_noise(c, in.src(), in.dtype(), k.dev, nrows, B, method, method == PP_NORM_PROF ? in.scales.data() : nullptr, norms, noise));
    }
    { Outs o; double* snrs = o.d(nrows);
      AUX(o, name("pp_channel_snrs"), pp_channel_snrs(c, in.src(), in.dtype(), k.dev, nrows, B, 3.25, snrs)); }
    // the 'fit' noise method: both model functions, with and without the optional outputs
    for (int fn : {PP_KC_EXP_DC, PP_KC_HALF_TRI}) {
        Outs o; double* norms = o.d(nrows); double* noise = o.d(nrows);
        int32_t* kc = (int32_t*)o.raw(nrows, 4); int32_t* cell = (int32_t*)o.raw((size_t)nrows * 3, 4);
        AUX(o, name(fn == PP_KC_EXP_DC ? "pp_channel_noise_fit exp_dc" : "pp_channel_noise_fit half_tri"),
            pp_channel_noise_fit(c, in.src(), in.dtype(), k.dev, nrows, B, PP_NOISEFIT_ROWS, fn, 1.1, PP_NORM_RMS, nullptr, norms, noise, kc, cell));
    }
    { Outs o; double* norms = o.d(nrows); double* noise = o.d(nrows);
      AUX(o, name("pp_channel_noise_fit prof"),
          pp_channel_noise_fit(c, in.src(), in.dtype(), k.dev, nrows, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_PROF, in.scales.data(), norms, noise,
                               nullptr, nullptr)); }
    { Outs o; double* snrs = o.d(nrows);
      AUX(o, name("pp_channel_snrs_fit"), pp_channel_snrs_fit(c, in.src(), in.dtype(), k.dev, nrows, B, PP_KC_EXP_DC, 1.1, 3.25, snrs)); }
    if (!k.f32) {       // rows that already are power spectra: H = B / 2 + 1 f64 values each, read from the front of the rows
        const int H = B / 2 + 1;
        const int np_ = (int)((size_t)nrows * B / H);
        Outs o; double* norms = o.d(np_); double* noise = o.d(np_);
        int32_t* kc = (int32_t*)o.raw(np_, 4); int32_t* cell = (int32_t*)o.raw((size_t)np_ * 3, 4);
        AUX(o, name("pp_channel_noise_fit pows"),
            pp_channel_noise_fit(c, in.src(), PP_F64, k.dev, np_, B, PP_NOISEFIT_POWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, norms, noise, kc, cell));
    }
    // pca: the first C rows as a portrait (C < B: the dual side), then, for the shortest rows, 80 of them (nchan >= nbin)
    for (int nchan : {C, 80}) {
        if (nchan > nrows || (nchan == 80 && B != 64)) continue;
        const int n = nchan < B ? nchan : B, nvec = 3;
        snprintf(nm, sizeof nm, "pca %s %dx%d %s %s", tag, nchan, B, k.f32 ? "f32" : "f64", k.dev ? "device" : "host");
        std::vector<double> vecs((size_t)nvec * n, 0.1), lam(nvec, 2.0);
        const int32_t ieig[2] = {2, 0};
        { Outs o; double* mean = o.d(B); double* gram = o.d((size_t)n * n);
          AUX(o, nm, pp_pca_gram(c, in.src(), in.dtype(), k.dev, nchan, B, in.w.data(), (double)nchan, nchan - 1.0, mean, gram)); }
        { Outs o; double* basis = o.d((size_t)nvec * B); double* stats = o.d((size_t)nvec * 4);
          AUX(o, "pp_pca_basis", pp_pca_basis(c, vecs.data(), lam.data(), nvec, basis, stats)); }
        { Outs o; double* proj = o.d((size_t)nchan * 2); double* rec = o.d((size_t)nchan * B);
          AUX(o, "pp_pca_project", pp_pca_project(c, ieig, 2, proj, rec)); }
    }
    if (!k.dev) {
        Outs o; double* out = o.d((size_t)nrows * (B / 2 + 1) * 2);
        AUX(o, name("pp_rfft_rows"), pp_rfft_rows(c, in.ports.data(), in.dtype(), nrows, B, out));
    }
    { Outs o; void* dst = dev_copy(nullptr, in.nrow * B * in.esz);
      std::vector<double> inj((size_t)ns * 3, 0.0);
      AUX(o, name("pp_synth_portraits"), pp_synth_portraits(c, k.dev, dst, in.dtype(), ns, in.freqs.data(), in.P.data(), inj.data(),
          k.dev ? in.scales.data() : nullptr, 0.05, 7, 3));
      dev_free(dst); }
    // simulated observations: delays [ns][C], amps [ns][npol][C] and sigmas [C] sized exactly, with and without the optional ones
    for (int npol : {1, 3}) {
        Outs o; void* dst = dev_copy(nullptr, in.nrow * npol * B * in.esz);
        std::vector<double> delays((size_t)ns * C, 0.25), amps((size_t)ns * npol * C, 1.5), sigmas(C, 0.05);
        snprintf(nm, sizeof nm, "pp_fake_portraits %s %dx%dx%d %s slot %d", tag, ns * npol, C, B, k.f32 ? "f32" : "f64", k.dev);
        AUX(o, nm, pp_fake_portraits(c, k.dev, dst, in.dtype(), ns, npol, delays.data(), npol == 1 ? nullptr : amps.data(),
                                     npol == 1 ? nullptr : sigmas.data(), 7, 3));
        dev_free(dst); }
    // scrunching: weights [ns][C], offsets [3], dst [2][1][2][B] and wout [2][2] sized exactly; the first of the two time
    // groups is longer than a run of the small budget: it straddles runs and carries its partial sums
    for (int mode : {PP_POL_KEEP, PP_POL_FIRST}) {
        Outs o;
        const int32_t t_off[3] = {0, ns - 1, ns}, f_off[3] = {0, C / 2, C};
        std::vector<double> w((size_t)ns * C, 1.25);
        w[1] = 0.0;
        const size_t nout = (size_t)4 * B;
        double* wout = o.d(4);
        double* dst = k.dev ? (double*)dev_copy(nullptr, nout * 8) : o.d(nout);
        snprintf(nm, sizeof nm, "pp_scrunch %s %dx%dx%d %s %s mode %d", tag, ns, C, B, k.f32 ? "f32" : "f64", k.dev ? "device" : "host", mode);
        AUX(o, nm, pp_scrunch(c, in.src(), in.dtype(), k.dev, ns, 1, C, B, w.data(), 2, t_off, 2, f_off, mode, dst, wout));
        if (k.dev) dev_free(dst);
    }
    // ... and Coherence -> Intensity of three polarisations (the third is not read, and not copied): src [ns][3][C][B] of its own,
    // sized exactly; the second polarisation's rows lie a plane behind the first's
    {
        Outs o;
        const int32_t t_off[3] = {0, ns - 1, ns}, f_off[3] = {0, C / 2, C};
        std::vector<double> w((size_t)ns * C, 0.75);
        w[(size_t)ns * C - 1] = 0.0;
        std::vector<unsigned char> src3((size_t)ns * 3 * C * B * in.esz, 0);
        void* dsrc3 = k.dev ? dev_copy(src3.data(), src3.size()) : nullptr;
        const size_t nout = (size_t)4 * B;
        double* wout = o.d(4);
        double* dst = k.dev ? (double*)dev_copy(nullptr, nout * 8) : o.d(nout);
        snprintf(nm, sizeof nm, "pp_scrunch %s %dx3x%dx%d %s %s sum01", tag, ns, C, B, k.f32 ? "f32" : "f64", k.dev ? "device" : "host");
        AUX(o, nm, pp_scrunch(c, k.dev ? dsrc3 : (const void*)src3.data(), in.dtype(), k.dev, ns, 3, C, B, w.data(), 2, t_off, 2, f_off,
                              PP_POL_SUM01, dst, wout));
        if (k.dev) { dev_free(dst); dev_free(dsrc3); }
    }
    { Outs o; int shape[2] = {0, 0};
      AUX(o, "pp_model_shape", pp_model_shape(c, k.dev, &shape[0], &shape[1]));
      if (shape[0] != C || shape[1] != B) { fprintf(stderr, "pp_model_shape: %d x %d, not %d x %d\n", shape[0], shape[1], C, B); exit(1); } }
}

// the entry points whose inputs are all double precision on the host
static void aux_host_calls(pp_ctx* c, int ns, int C, int B, const char* tag) {
    char nm[200];
    auto name = [&](const char* fn) { snprintf(nm, sizeof nm, "%s %s %dx%dx%d", fn, tag, ns, C, B); return nm; };
    std::vector<double> freqs(C);
    for (int j = 0; j < C; ++j) freqs[j] = 1100.0 + 800.0 * (j + 0.5) / C;
    for (int with_noise : {0, 1}) {
        const int nprof = 2 * ns + 1 + 17 * with_noise;
        std::vector<double> data((size_t)nprof * B, 0.5), model((size_t)nprof * B, 1.0), noise(nprof, 0.05);
        Outs o; double* out7 = o.d((size_t)nprof * 7);
        AUX(o, name(with_noise ? "pp_fit_phase_shift_batch noise" : "pp_fit_phase_shift_batch"),
            pp_fit_phase_shift_batch(c, data.data(), model.data(), with_noise ? noise.data() : nullptr, nprof, B, -0.5, 0.5, 20, out7));
        // the narrowband scattering fit: guess [nprof][2] (a NaN phase asks for the grid), out [nprof][PP_NBS_NOUT]
        for (int log10_tau : {0, 1}) {
            std::vector<double> guess((size_t)nprof * 2);
            for (int i = 0; i < nprof; ++i) { guess[2 * i] = (i & 1) ? 0.1 : NAN; guess[2 * i + 1] = log10_tau ? -2.0 : 0.0; }
            Outs o2; double* outs = o2.d((size_t)nprof * PP_NBS_NOUT);
            AUX(o2, name(log10_tau ? "pp_fit_phase_tau_batch log10" : "pp_fit_phase_tau_batch"),
                pp_fit_phase_tau_batch(c, data.data(), model.data(), with_noise ? noise.data() : nullptr, guess.data(), nprof, B, -0.5, 0.5, 20,
                                       log10_tau, outs));
        }
    }
    // templates generated on the device: to the host, to a device buffer, into a slot; then the response on that slot
    const double comps[12] = {0.3, 0.0, 0.02, 0.0, 1.0, 0.0, 0.6, 0.0, 0.05, 0.0, 0.5, -1.0};
    for (double tau : {0.0, 1e-3}) {
        snprintf(nm, sizeof nm, "pp_gaussian_portrait %s %dx%d tau=%g", tag, C, B, tau);
        { Outs o; double* port = o.d((size_t)C * B);
          AUX(o, nm, pp_gaussian_portrait(c, C, B, freqs.data(), "000", 1500.0, 0.1, tau, -4.0, 2, comps, port, 0)); }
        { Outs o; double* dport = (double*)dev_copy(nullptr, (size_t)C * B * 8);
          AUX(o, "pp_gaussian_portrait to the device", pp_gaussian_portrait(c, C, B, freqs.data(), "101", 1500.0, 0.1, tau, -4.0, 2, comps, dport, 1));
          dev_free(dport); }
        { Outs o; AUX(o, "pp_model_set_gaussian", pp_model_set_gaussian(c, 2, C, B, freqs.data(), "000", 1500.0, 0.1, tau, -4.0, 2, comps)); }
    }
    for (int ncomp : {0, 2}) {
        const int deg = 3, nknots = 8;
        std::vector<double> basis((size_t)(ncomp + 1) * B, 0.25), t(nknots), coefs((size_t)(ncomp ? ncomp : 1) * nknots, 0.5);
        for (int j = 0; j < nknots; ++j) t[j] = j < 4 ? 1100.0 : 1900.0;
        snprintf(nm, sizeof nm, "pp_spline_portrait %s %dx%d ncomp=%d", tag, C, B, ncomp);
        { Outs o; double* port = o.d((size_t)C * B);
          AUX(o, nm, pp_spline_portrait(c, C, B, freqs.data(), ncomp, basis.data(), nknots, ncomp ? t.data() : nullptr, ncomp ? coefs.data() : nullptr, deg, port, 0)); }
        { Outs o; double* dport = (double*)dev_copy(nullptr, (size_t)C * B * 8);
          AUX(o, "pp_spline_portrait to the device", pp_spline_portrait(c, C, B, freqs.data(), ncomp, basis.data(), nknots, t.data(), coefs.data(), deg, dport, 1));
          dev_free(dport); }
        { Outs o; AUX(o, "pp_model_set_spline", pp_model_set_spline(c, 3, C, B, freqs.data(), ncomp, basis.data(), nknots, t.data(), coefs.data(), deg)); }
    }
    {
        std::vector<double> rconst((size_t)(B / 2 + 1) * 2, 1.0), wid(C, 1e-3);
        Outs o;
        AUX(o, name("pp_model_apply_response both"), pp_model_apply_response(c, 2, rconst.data(), wid.data()));
        AUX(o, "pp_model_apply_response rconst", pp_model_apply_response(c, 3, rconst.data(), nullptr));
        AUX(o, "pp_model_apply_response smear", pp_model_apply_response(c, 3, nullptr, wid.data()));
        AUX(o, "pp_model_apply_response neither", pp_model_apply_response(c, 3, nullptr, nullptr));
    }
    {
        std::vector<double> noise((size_t)ns * C, 1.0);
        std::vector<unsigned char> good((size_t)ns * C, 1);
        Outs o; unsigned char* zap = (unsigned char*)o.raw((size_t)ns * C, 1);
        AUX(o, name("pp_zap_median"), pp_zap_median(c, noise.data(), good.data(), ns, C, 5.0, zap));
    }
}

// every refusal the preambles can give, on one context with C x B templates in slots 0 and 1
static void aux_refusals(int C, int B) {
    mark("case aux context %dx%d for the refusals", C, B);
    pp_ctx* c = make_ctx(C, B);
    const int ns = 3;
    AuxCfg k{B, C, ns, 0, 0, 0, 0, 0};
    AuxIn in(k);
    // (no output is checked here: a refused call writes nothing, and in the null-pointer loop the calls that do not
    // take the pointer in turn succeed, into `out`, which is large enough for each of them)
    const Outs o;
    std::vector<double> outv((size_t)ns * C * B);
    double* out = outv.data();
    std::vector<int32_t> badslot(ns, 9);
    const void* src = in.src();
    const double *f = in.freqs.data(), *P = in.P.data(), *p3 = in.par3.data(), *w = in.w.data(), *mp = in.mprof.data();
    const double *p5 = in.params5.data(), *n3 = in.nus3.data(), *sc = in.scales.data(), *er = in.errs.data();
#define REF(what, call) AUX(o, "refused: " what, call)
    // the shared preamble, entry point by entry point: null, nbin, shape, dtype, freqs_stride
    for (int B2 : {B + 1, 6, 4098}) {
        REF("pp_reference_phase_seed nbin", pp_reference_phase_seed(c, src, PP_F64, 0, ns, C, B2, f, 0, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 20, out));
        REF("pp_rotate_portraits nbin", pp_rotate_portraits(c, src, out, PP_F64, 0, ns, C, B2, f, 0, P, p3, INFINITY, INFINITY));
        REF("pp_align_accumulate nbin", pp_align_accumulate(c, src, PP_F64, 0, ns, C, B2, f, 0, P, p3, w, out, out));
        REF("pp_channel_red_chi2 nbin", pp_channel_red_chi2(c, src, PP_F64, 0, ns, C, B2, nullptr, f, 0, P, p5, n3, sc, er, out));
        REF("pp_fit_residuals nbin", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B2, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
        REF("pp_fit_phase_shift_batch nbin", pp_fit_phase_shift_batch(c, mp, mp, nullptr, ns, B2, -0.5, 0.5, 20, out));
        REF("pp_fit_phase_tau_batch nbin", pp_fit_phase_tau_batch(c, mp, mp, nullptr, mp, ns, B2, -0.5, 0.5, 20, 1, out));
        REF("pp_rfft_rows nbin", pp_rfft_rows(c, src, PP_F64, ns, B2, out));
        REF("pp_channel_noise nbin", pp_channel_noise(c, src, PP_F64, 0, ns, B2, PP_NORM_NONE, nullptr, out, out));
        REF("pp_channel_snrs nbin", pp_channel_snrs(c, src, PP_F64, 0, ns, B2, 3.25, out));
        REF("pp_channel_noise_fit nbin", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B2, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
        REF("pp_channel_snrs_fit nbin", pp_channel_snrs_fit(c, src, PP_F64, 0, ns, B2, PP_KC_EXP_DC, 1.1, 3.25, out));
        REF("pp_pca_gram nbin", pp_pca_gram(c, src, PP_F64, 0, C, B2, w, (double)C, C - 1.0, out, out));
        REF("pp_gaussian_portrait nbin", pp_gaussian_portrait(c, C, B2, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5, out, 0));
        REF("pp_model_set_gaussian nbin", pp_model_set_gaussian(c, 2, C, B2, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5));
        REF("pp_model_set_spline nbin", pp_model_set_spline(c, 2, C, B2, f, 0, mp, 0, nullptr, nullptr, 3));
        REF("pp_model_set nbin", pp_model_set(c, 2, src, PP_F64, 0, C, B2));
    }
    for (int which = 0; which < 2; ++which) {        // 0: nsub 0, 1: nchan 0
        const int s = which == 0 ? 0 : ns, ch = which == 1 ? 0 : C;
        REF("pp_reference_phase_seed shape", pp_reference_phase_seed(c, src, PP_F64, 0, s, ch, B, f, 0, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 20, out));
        REF("pp_rotate_portraits shape", pp_rotate_portraits(c, src, out, PP_F64, 0, s, ch, B, f, 0, P, p3, INFINITY, INFINITY));
        REF("pp_align_accumulate shape", pp_align_accumulate(c, src, PP_F64, 0, s, ch, B, f, 0, P, p3, w, out, out));
        REF("pp_channel_red_chi2 shape", pp_channel_red_chi2(c, src, PP_F64, 0, s, ch, B, nullptr, f, 0, P, p5, n3, sc, er, out));
        REF("pp_fit_residuals shape", pp_fit_residuals(c, src, PP_F64, 0, s, ch, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
    }
    REF("pp_reference_phase_seed Ns", pp_reference_phase_seed(c, src, PP_F64, 0, ns, C, B, f, 0, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 0, out));
    REF("pp_fit_phase_shift_batch nprof", pp_fit_phase_shift_batch(c, mp, mp, nullptr, 0, B, -0.5, 0.5, 20, out));
    REF("pp_fit_phase_shift_batch Ns", pp_fit_phase_shift_batch(c, mp, mp, nullptr, ns, B, -0.5, 0.5, 0, out));
    REF("pp_fit_phase_tau_batch nprof", pp_fit_phase_tau_batch(c, mp, mp, nullptr, mp, 0, B, -0.5, 0.5, 20, 1, out));
    REF("pp_fit_phase_tau_batch Ns", pp_fit_phase_tau_batch(c, mp, mp, nullptr, mp, ns, B, -0.5, 0.5, 0, 1, out));
    REF("pp_fit_phase_tau_batch bounds", pp_fit_phase_tau_batch(c, mp, mp, nullptr, mp, ns, B, 0.5, -0.5, 20, 1, out));
    REF("pp_rfft_rows nrows", pp_rfft_rows(c, src, PP_F64, 0, B, out));
    REF("pp_synth_portraits nsub", pp_synth_portraits(c, 0, out, PP_F64, 0, f, P, p3, nullptr, 0.05, 7, 0));
    REF("pp_channel_noise nrows", pp_channel_noise(c, src, PP_F64, 0, 0, B, PP_NORM_NONE, nullptr, out, out));
    REF("pp_channel_noise method", pp_channel_noise(c, src, PP_F64, 0, ns, B, 9, nullptr, out, out));
    REF("pp_channel_noise prof without divisors", pp_channel_noise(c, src, PP_F64, 0, ns, B, PP_NORM_PROF, nullptr, out, out));
    REF("pp_channel_snrs nrows", pp_channel_snrs(c, src, PP_F64, 0, 0, B, 3.25, out));
    REF("pp_channel_snrs null", pp_channel_snrs(c, src, PP_F64, 0, ns, B, 3.25, nullptr));
    REF("pp_channel_noise_fit nrows", pp_channel_noise_fit(c, src, PP_F64, 0, 0, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit kind", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, 2, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit fn", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, 2, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit fact", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, -1.0, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit method", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, 9, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit prof without divisors", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_PROF, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit pows f32", pp_channel_noise_fit(c, src, PP_F32, 0, ns, B, PP_NOISEFIT_POWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit pows norm", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_POWS, PP_KC_EXP_DC, 1.1, PP_NORM_RMS, nullptr, out, out, nullptr, nullptr));
    REF("pp_channel_noise_fit null", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, nullptr, out, nullptr, nullptr));
    REF("pp_channel_snrs_fit null", pp_channel_snrs_fit(c, src, PP_F64, 0, ns, B, PP_KC_EXP_DC, 1.1, 3.25, nullptr));
    { double a20[20]; int32_t kc20[20];
      REF("pp_noise_fit_grid fn", pp_noise_fit_grid(33, 5, a20, kc20));
      REF("pp_noise_fit_grid null", pp_noise_fit_grid(33, PP_KC_EXP_DC, nullptr, kc20));
      mark("case aux pp_noise_fit_grid"); ++g_ncase;
      for (int H : {5, 33, 2049})
          for (int fn : {PP_KC_EXP_DC, PP_KC_HALF_TRI})
              if (pp_noise_fit_grid(H, fn, a20, kc20) != PP_OK || kc20[0] < 1 || kc20[19] > H) { fprintf(stderr, "pp_noise_fit_grid(%d, %d)\n", H, fn); exit(1); } }
    REF("pp_zap_median shape", pp_zap_median(c, sc, (const unsigned char*)src, 0, C, 5.0, (unsigned char*)out));
    REF("pp_zap_median channels", pp_zap_median(c, sc, (const unsigned char*)src, ns, 5000, 5.0, (unsigned char*)out));
    REF("pp_pca_gram nchan", pp_pca_gram(c, src, PP_F64, 0, 1, B, w, 1.0, 1.0, out, out));
    REF("pp_pca_gram weights", pp_pca_gram(c, src, PP_F64, 0, C, B, w, 0.0, 1.0, out, out));
    for (int dt : {7, -1}) {
        REF("pp_reference_phase_seed dtype", pp_reference_phase_seed(c, src, dt, 0, ns, C, B, f, 0, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 20, out));
        REF("pp_rotate_portraits dtype", pp_rotate_portraits(c, src, out, dt, 0, ns, C, B, f, 0, P, p3, INFINITY, INFINITY));
        REF("pp_align_accumulate dtype", pp_align_accumulate(c, src, dt, 0, ns, C, B, f, 0, P, p3, w, out, out));
        REF("pp_channel_red_chi2 dtype", pp_channel_red_chi2(c, src, dt, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, out));
        REF("pp_fit_residuals dtype", pp_fit_residuals(c, src, dt, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
        REF("pp_synth_portraits dtype", pp_synth_portraits(c, 0, out, dt, ns, f, P, p3, nullptr, 0.05, 7, 0));
        REF("pp_channel_noise dtype", pp_channel_noise(c, src, dt, 0, ns, B, PP_NORM_NONE, nullptr, out, out));
        REF("pp_channel_snrs dtype", pp_channel_snrs(c, src, dt, 0, ns, B, 3.25, out));
        REF("pp_channel_noise_fit dtype", pp_channel_noise_fit(c, src, dt, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
        REF("pp_pca_gram dtype", pp_pca_gram(c, src, dt, 0, C, B, w, (double)C, C - 1.0, out, out));
        REF("pp_model_set dtype", pp_model_set(c, 2, src, dt, 0, C, B));
    }
    for (int64_t fs : {(int64_t)5, (int64_t)-1, (int64_t)C + 1}) {
        REF("pp_reference_phase_seed freqs_stride", pp_reference_phase_seed(c, src, PP_F64, 0, ns, C, B, f, fs, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 20, out));
        REF("pp_rotate_portraits freqs_stride", pp_rotate_portraits(c, src, out, PP_F64, 0, ns, C, B, f, fs, P, p3, INFINITY, INFINITY));
        REF("pp_align_accumulate freqs_stride", pp_align_accumulate(c, src, PP_F64, 0, ns, C, B, f, fs, P, p3, w, out, out));
        REF("pp_channel_red_chi2 freqs_stride", pp_channel_red_chi2(c, src, PP_F64, 0, ns, C, B, nullptr, f, fs, P, p5, n3, sc, er, out));
        REF("pp_fit_residuals freqs_stride", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B, nullptr, f, fs, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
    }
    // one null pointer at a time
    for (int z = 0; z < 9; ++z) {
#define NZ(i, p) (z == (i) ? nullptr : (p))
        REF("pp_reference_phase_seed null", pp_reference_phase_seed(NZ(8, c), NZ(0, src), PP_F64, 0, ns, C, B, NZ(1, f), 0, NZ(2, P), NZ(3, p3), INFINITY, INFINITY,
                                                                   NZ(4, w), NZ(5, mp), -0.5, 0.5, 20, NZ(6, out)));
        REF("pp_rotate_portraits null", pp_rotate_portraits(NZ(8, c), NZ(0, src), NZ(6, out), PP_F64, 0, ns, C, B, NZ(1, f), 0, NZ(2, P), NZ(3, p3), INFINITY, INFINITY));
        REF("pp_align_accumulate null", pp_align_accumulate(NZ(8, c), NZ(0, src), PP_F64, 0, ns, C, B, NZ(1, f), 0, NZ(2, P), NZ(3, p3), NZ(4, w), NZ(6, out), NZ(7, out)));
        REF("pp_channel_red_chi2 null", pp_channel_red_chi2(NZ(8, c), NZ(0, src), PP_F64, 0, ns, C, B, nullptr, NZ(1, f), 0, NZ(2, P), NZ(3, p5), NZ(4, n3), NZ(5, sc),
                                                           NZ(7, er), NZ(6, out)));
        REF("pp_fit_residuals null", pp_fit_residuals(NZ(8, c), NZ(0, src), PP_F64, 0, ns, C, B, nullptr, NZ(1, f), 0, NZ(2, P), NZ(3, p5), NZ(4, n3), NZ(5, sc),
                                                     NZ(7, er), nullptr, 0, nullptr, nullptr, nullptr, NZ(6, out)));
        REF("pp_fit_phase_shift_batch null", pp_fit_phase_shift_batch(NZ(8, c), NZ(0, mp), NZ(1, mp), nullptr, ns, B, -0.5, 0.5, 20, NZ(6, out)));
        REF("pp_fit_phase_tau_batch null", pp_fit_phase_tau_batch(NZ(8, c), NZ(0, mp), NZ(1, mp), nullptr, NZ(2, mp), ns, B, -0.5, 0.5, 20, 1, NZ(6, out)));
        REF("pp_rfft_rows null", pp_rfft_rows(NZ(8, c), NZ(0, src), PP_F64, ns, B, NZ(6, out)));
        REF("pp_synth_portraits null", pp_synth_portraits(NZ(8, c), 0, NZ(6, out), PP_F64, ns, NZ(1, f), NZ(2, P), NZ(3, p3), nullptr, 0.05, 7, 0));
        REF("pp_channel_noise null", pp_channel_noise(NZ(8, c), NZ(0, src), PP_F64, 0, ns, B, PP_NORM_NONE, nullptr, NZ(6, out), NZ(7, out)));
        REF("pp_zap_median null", pp_zap_median(NZ(8, c), NZ(0, sc), NZ(1, (const unsigned char*)src), ns, C, 5.0, NZ(6, (unsigned char*)out)));
        REF("pp_pca_gram null", pp_pca_gram(NZ(8, c), NZ(0, src), PP_F64, 0, C, B, NZ(4, w), (double)C, C - 1.0, NZ(6, out), NZ(7, out)));
        REF("pp_gaussian_portrait null", pp_gaussian_portrait(NZ(8, c), C, B, NZ(1, f), NZ(0, "000"), 1500.0, 0.0, 0.0, -4.0, 1, NZ(3, p5), NZ(6, out), 0));
        REF("pp_model_set_gaussian null", pp_model_set_gaussian(NZ(8, c), 2, C, B, NZ(1, f), NZ(0, "000"), 1500.0, 0.0, 0.0, -4.0, 1, NZ(3, p5)));
        REF("pp_spline_portrait null", pp_spline_portrait(NZ(8, c), C, B, NZ(1, f), 1, NZ(0, mp), 8, NZ(2, sc), NZ(3, sc), 3, NZ(6, out), 0));
        REF("pp_model_set_spline null", pp_model_set_spline(NZ(8, c), 2, C, B, NZ(1, f), 1, NZ(0, mp), 8, NZ(2, sc), NZ(3, sc), 3));
        REF("pp_model_set null", pp_model_set(NZ(8, c), 2, NZ(0, src), PP_F64, 0, C, B));
        REF("pp_model_apply_response null", pp_model_apply_response(NZ(8, c), 0, NZ(0, mp), NZ(1, sc)));
#undef NZ
    }
    // slots
    REF("pp_synth_portraits unset slot", pp_synth_portraits(c, 9, out, PP_F64, ns, f, P, p3, nullptr, 0.05, 7, 0));
    REF("pp_synth_portraits slot out of range", pp_synth_portraits(c, PP_MAX_SLOTS, out, PP_F64, ns, f, P, p3, nullptr, 0.05, 7, 0));
    {   // pp_fake_portraits: its own preamble (the arrays sized for ns x 2 x C)
        std::vector<double> dl((size_t)ns * C, 0.1), am((size_t)ns * 2 * C, 1.0), sg(C, 0.05), bad;
        REF("pp_fake_portraits unset slot", pp_fake_portraits(c, 9, out, PP_F64, ns, 2, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits slot out of range", pp_fake_portraits(c, -1, out, PP_F64, ns, 2, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits npol", pp_fake_portraits(c, 0, out, PP_F64, ns, 0, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits nsub", pp_fake_portraits(c, 0, out, PP_F64, 0, 2, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits dtype", pp_fake_portraits(c, 0, out, 7, ns, 2, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits null delays", pp_fake_portraits(c, 0, out, PP_F64, ns, 2, nullptr, am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits null dst", pp_fake_portraits(c, 0, nullptr, PP_F64, ns, 2, dl.data(), am.data(), sg.data(), 7, 0));
        REF("pp_fake_portraits null context", pp_fake_portraits(nullptr, 0, out, PP_F64, ns, 2, dl.data(), am.data(), sg.data(), 7, 0));
        bad = sg; bad[C - 1] = -0.5;
        REF("pp_fake_portraits negative sigma", pp_fake_portraits(c, 0, out, PP_F64, ns, 2, dl.data(), am.data(), bad.data(), 7, 0));
        bad = sg; bad[0] = NAN;
        REF("pp_fake_portraits NaN sigma", pp_fake_portraits(c, 0, out, PP_F64, ns, 2, dl.data(), am.data(), bad.data(), 7, 0));
        bad = dl; bad[(size_t)ns * C - 1] = INFINITY;
        REF("pp_fake_portraits infinite delay", pp_fake_portraits(c, 0, out, PP_F64, ns, 2, bad.data(), am.data(), sg.data(), 7, 0));
        int nc = 0, nb = 0;
        REF("pp_model_shape unset slot", pp_model_shape(c, 9, &nc, &nb));
        REF("pp_model_shape null", pp_model_shape(c, 0, nullptr, &nb));
    }
    REF("pp_channel_red_chi2 unset slot", pp_channel_red_chi2(c, src, PP_F64, 0, ns, C, B, badslot.data(), f, 0, P, p5, n3, sc, er, out));
    REF("pp_channel_red_chi2 slot of another shape", pp_channel_red_chi2(c, src, PP_F64, 0, ns, C / 2, B, nullptr, f, 0, P, p5, n3, sc, er, out));
    REF("pp_fit_residuals unset slot", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B, badslot.data(), f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
    REF("pp_fit_residuals slot of another shape", pp_fit_residuals(c, src, PP_F64, 0, ns, C / 2, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
    REF("pp_fit_residuals frame", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 2, out, nullptr, nullptr, nullptr));
    REF("pp_fit_residuals no output", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, nullptr, nullptr, nullptr, nullptr));
    REF("pp_model_apply_response unset slot", pp_model_apply_response(c, 9, mp, nullptr));
    REF("pp_model_apply_response slot out of range", pp_model_apply_response(c, -1, mp, nullptr));
    REF("pp_model_set slot", pp_model_set(c, PP_MAX_SLOTS, src, PP_F64, 0, C, B));
    REF("pp_model_set nchan", pp_model_set(c, 2, src, PP_F64, 0, 0, B));
    // generators
    REF("pp_gaussian_portrait shape", pp_gaussian_portrait(c, 0, B, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5, out, 0));
    REF("pp_gaussian_portrait components", pp_gaussian_portrait(c, C, B, f, "000", 1500.0, 0.0, 0.0, -4.0, 65, p5, out, 0));
    REF("pp_gaussian_portrait code", pp_gaussian_portrait(c, C, B, f, "0x0", 1500.0, 0.0, 0.0, -4.0, 1, p5, out, 0));
    REF("pp_model_set_gaussian code", pp_model_set_gaussian(c, 2, C, B, f, "002", 1500.0, 0.0, 0.0, -4.0, 1, p5));
    REF("pp_model_set_gaussian slot", pp_model_set_gaussian(c, -1, C, B, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5));
    REF("pp_spline_portrait shape", pp_spline_portrait(c, 0, B, f, 0, mp, 0, nullptr, nullptr, 3, out, 0));
    REF("pp_spline_portrait components", pp_spline_portrait(c, C, B, f, 33, mp, 8, sc, sc, 3, out, 0));
    REF("pp_spline_portrait degree", pp_spline_portrait(c, C, B, f, 1, mp, 8, sc, sc, 6, out, 0));
    REF("pp_model_set_spline knots", pp_model_set_spline(c, 2, C, B, f, 1, mp, 7, sc, sc, 3));
    // the pca calls out of order, then their own argument checks
    std::vector<double> vecs((size_t)3 * C, 0.1), lam(3, 2.0);
    const int32_t ieig[2] = {2, 0}, ieig_bad[2] = {0, 5};
    REF("pp_pca_basis before pp_pca_gram", pp_pca_basis(c, vecs.data(), lam.data(), 3, out, out));
    REF("pp_pca_project before pp_pca_gram", pp_pca_project(c, ieig, 2, out, out));
    { Outs g; double* mean = g.d(B); double* gram = g.d((size_t)C * C);
      AUX(g, "pp_pca_gram for the refusals", pp_pca_gram(c, src, PP_F64, 0, C, B, w, (double)C, C - 1.0, mean, gram)); }
    REF("pp_pca_project before pp_pca_basis", pp_pca_project(c, ieig, 2, out, out));
    REF("pp_pca_basis nvec", pp_pca_basis(c, vecs.data(), lam.data(), 17, out, out));
    REF("pp_pca_basis null", pp_pca_basis(c, vecs.data(), nullptr, 3, out, out));
    { Outs g; double* basis = g.d((size_t)3 * B); double* stats = g.d(12);
      AUX(g, "pp_pca_basis for the refusals", pp_pca_basis(c, vecs.data(), lam.data(), 3, basis, stats)); }
    REF("pp_pca_project ncomp", pp_pca_project(c, ieig, 4, out, out));
    REF("pp_pca_project index", pp_pca_project(c, ieig_bad, 2, out, out));
    REF("pp_pca_project null", pp_pca_project(c, nullptr, 2, out, out));
    REF("pp_pca_gram refused drops the resident rows", pp_pca_gram(c, src, PP_F64, 0, C, B, w, (double)C, -1.0, out, out));
    REF("pp_pca_basis after a refused pp_pca_gram", pp_pca_basis(c, vecs.data(), lam.data(), 3, out, out));
    // an enqueued batch owns the context: every auxiliary call refuses until it is collected
    {
        Spec s; s.C = C; s.B = B;
        Batch b(s);
        mark("case aux refused: a batch is pending");
        ++g_ncase;
        mark("enqueue rc %d", pp_fit_enqueue(c, &b.in, &b.out));
        REF("pending pp_fit_phase_shift_batch", pp_fit_phase_shift_batch(c, mp, mp, nullptr, ns, B, -0.5, 0.5, 20, out));
        REF("pending pp_fit_phase_tau_batch", pp_fit_phase_tau_batch(c, mp, mp, nullptr, mp, ns, B, -0.5, 0.5, 20, 1, out));
        REF("pending pp_reference_phase_seed", pp_reference_phase_seed(c, src, PP_F64, 0, ns, C, B, f, 0, P, p3, INFINITY, INFINITY, w, mp, -0.5, 0.5, 20, out));
        REF("pending pp_synth_portraits", pp_synth_portraits(c, 0, out, PP_F64, ns, f, P, p3, nullptr, 0.05, 7, 0));
        REF("pending pp_fake_portraits", pp_fake_portraits(c, 0, out, PP_F64, ns, 1, w, nullptr, nullptr, 7, 0));
        REF("pending pp_rotate_portraits", pp_rotate_portraits(c, src, out, PP_F64, 0, ns, C, B, f, 0, P, p3, INFINITY, INFINITY));
        REF("pending pp_align_accumulate", pp_align_accumulate(c, src, PP_F64, 0, ns, C, B, f, 0, P, p3, w, out, out));
        REF("pending pp_channel_red_chi2", pp_channel_red_chi2(c, src, PP_F64, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, out));
        REF("pending pp_fit_residuals", pp_fit_residuals(c, src, PP_F64, 0, ns, C, B, nullptr, f, 0, P, p5, n3, sc, er, nullptr, 0, out, nullptr, nullptr, nullptr));
        REF("pending pp_gaussian_portrait", pp_gaussian_portrait(c, C, B, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5, out, 0));
        REF("pending pp_model_set_gaussian", pp_model_set_gaussian(c, 2, C, B, f, "000", 1500.0, 0.0, 0.0, -4.0, 1, p5));
        REF("pending pp_spline_portrait", pp_spline_portrait(c, C, B, f, 0, mp, 0, nullptr, nullptr, 3, out, 0));
        REF("pending pp_model_set_spline", pp_model_set_spline(c, 2, C, B, f, 0, mp, 0, nullptr, nullptr, 3));
        REF("pending pp_model_apply_response", pp_model_apply_response(c, 0, mp, nullptr));
        REF("pending pp_rfft_rows", pp_rfft_rows(c, src, PP_F64, ns, B, out));
        REF("pending pp_channel_noise", pp_channel_noise(c, src, PP_F64, 0, ns, B, PP_NORM_NONE, nullptr, out, out));
        REF("pending pp_channel_snrs", pp_channel_snrs(c, src, PP_F64, 0, ns, B, 3.25, out));
        REF("pending pp_channel_noise_fit", pp_channel_noise_fit(c, src, PP_F64, 0, ns, B, PP_NOISEFIT_ROWS, PP_KC_EXP_DC, 1.1, PP_NORM_NONE, nullptr, out, out, nullptr, nullptr));
        REF("pending pp_zap_median", pp_zap_median(c, sc, (const unsigned char*)src, ns, C, 5.0, (unsigned char*)out));
        REF("pending pp_pca_gram", pp_pca_gram(c, src, PP_F64, 0, C, B, w, (double)C, C - 1.0, out, out));
        REF("pending pp_pca_basis", pp_pca_basis(c, vecs.data(), lam.data(), 3, out, out));
        REF("pending pp_pca_project", pp_pca_project(c, ieig, 2, out, out));
        REF("pending pp_model_set", pp_model_set(c, 2, src, PP_F64, 0, C, B));
        mark("collect rc %d", pp_fit_collect(c));
    }
#undef REF
    MUST(pp_destroy(c));
}

// row lengths 64, 2048 (with option one_exchange 0 and 1) and 1000; option profile 0 and 1; the work budget large, and
// small enough that a host input goes through in three or more runs with a short last one; inside each: f64 / f32,
// host / device rows, freqs_stride 0 / nchan, model_slot null / set
static void aux_cases() {
    struct Len { int B, one_exchange; };
    const Len lens[] = {{64, -1}, {2048, 0}, {2048, 1}, {1000, -1}};
    const int chans[3] = {8, 24, 48};
    int q = 0;
    char tag[96];
    for (const Len& L : lens)
        for (int profile : {0, 1})
            for (int small : {0, 1}) {
                const int C = chans[q % 3];
                const int ns_of[2][3] = {{3, 5, 11}, {7, 10, 11}};
                mark("case aux context %dx%d one_exchange=%d profile=%d budget=%s", C, L.B, L.one_exchange, profile, small ? "small" : "large");
                pp_ctx* c = make_ctx(C, L.B);
                if (L.one_exchange >= 0) MUST(pp_set_option(c, "one_exchange", L.one_exchange));
                MUST(pp_set_option(c, "profile", profile));
                snprintf(tag, sizeof tag, "one_exchange=%d profile=%d budget=%s", L.one_exchange, profile, small ? "small" : "large");
                int j = q;
                for (int f32 : {0, 1})
                    for (int dev : {0, 1}) {
                        // the budget: 3.4 subints' portraits of this element size
                        if (small) MUST(pp_set_option(c, "max_work_bytes", 3.4 * C * L.B * (f32 ? 4 : 8)));
                        for (int fstride : {0, 1})
                            for (int slot : {0, 1})
                                aux_ports_calls(c, AuxCfg{L.B, C, ns_of[small][j++ % 3], f32, dev, fstride, slot, small}, tag);
                        aux_rows_calls(c, AuxCfg{L.B, C, ns_of[small][j++ % 3], f32, dev, 0, 0, small}, tag);
                    }
                if (small) MUST(pp_set_option(c, "max_work_bytes", 3.4 * C * L.B * 8));
                aux_host_calls(c, ns_of[small][j % 3], C, L.B, tag);
                MUST(pp_destroy(c));
                ++q;
            }
    aux_refusals(24, 64);
    aux_refusals(8, 1000);
}

// ---- the resident alignment accumulator: pp_align_begin / pp_align_add / pp_align_finish ------------------------
// (after aux_cases(), so that everything in front keeps its place in the trace)  Every array exactly as long as the
// entry points read or write; rows of f64 / f32, host / device, one polarisation / four, identity / many-to-one map
// with a row nothing lands on, weights with a zero and a NaN, adds of a host input in one run and in several, a second
// add into the same accumulator, finish into a slot and with a rotation
static void aux_align_calls(pp_ctx* c, int B, int Cm, int ns, int f32, int dev, int npol, int mapped, const char* tag) {
    const int C = mapped ? Cm + 4 : Cm;
    const size_t esz = f32 ? 4 : 8, nrow = (size_t)ns * npol * C;
    std::vector<unsigned char> ports(nrow * B * esz);
    for (size_t j = 0; j < nrow * B; ++j) {
        const double v = 0.5 + (j % 13) * 0.01;
        if (f32) ((float*)ports.data())[j] = (float)v; else ((double*)ports.data())[j] = v;
    }
    void* dports = dev ? dev_copy(ports.data(), ports.size()) : nullptr;
    const void* src = dev ? dports : (const void*)ports.data();
    std::vector<double> freqs(C), P(ns, 0.003), par3((size_t)ns * 3, 0.0), w((size_t)ns * C, 1.5);
    for (int j = 0; j < C; ++j) freqs[j] = 1100.0 + 800.0 * (j + 0.5) / C;
    for (int i = 0; i < ns; ++i) { par3[(size_t)i * 3] = 0.01 * i; par3[(size_t)i * 3 + 1] = i % 2 ? 1e-3 : 0.0; par3[(size_t)i * 3 + 2] = i % 3 ? 1500.0 : INFINITY; }
    w[1] = 0.0; w[w.size() - 1] = NAN; w[C] = -0.5;
    std::vector<int32_t> cmap((size_t)ns * C);
    for (int i = 0; i < ns; ++i)
        for (int n = 0; n < C; ++n) cmap[(size_t)i * C + n] = (n * (Cm - 1)) / C;        // the last row gets nothing
    const int32_t* cm = mapped ? cmap.data() : nullptr;
    char nm[200];
    auto name = [&](const char* fn) {
        snprintf(nm, sizeof nm, "%s %s %dx%dx%dx%d -> %d %s %s %s", fn, tag, ns, npol, C, B, Cm, f32 ? "f32" : "f64", dev ? "device" : "host", mapped ? "mapped" : "identity");
        return nm;
    };
    const int dt = f32 ? PP_F32 : PP_F64;
    { Outs o; int32_t* off = (int32_t*)o.raw((size_t)Cm + 1, 4); std::vector<int32_t> pairs((size_t)2 * ns * C);
      mark("case aux %s", name("pp_align_lists")); ++g_ncase;
      const int np_ = pp_align_lists(ns, C, Cm, w.data(), cm, off, pairs.data());
      mark("pairs %d", np_);
      if (np_ != ns * C - 2) { fprintf(stderr, "pp_align_lists: %d pairs of %d rows with two skipped\n", np_, ns * C); exit(1); }
      o.require_filled("pp_align_lists"); }
    { Outs o; AUX(o, name("pp_align_begin"), pp_align_begin(c, npol, Cm, B)); }
    { Outs o; AUX(o, name("pp_align_add"), pp_align_add(c, src, dt, dev, ns, npol, C, B, freqs.data(), 0, P.data(), par3.data(), w.data(), cm)); }
    { Outs o; double* al = o.d((size_t)npol * Cm * B); double* tw = o.d(Cm);
      AUX(o, name("pp_align_finish"), pp_align_finish(c, 0.0, al, tw, -1)); }
    { Outs o; AUX(o, name("pp_align_add again"), pp_align_add(c, src, dt, dev, 1, npol, C, B, freqs.data(), 0, P.data(), par3.data(), w.data(), cm)); }
    { Outs o; double* al = o.d((size_t)npol * Cm * B); double* tw = o.d(Cm);
      AUX(o, name("pp_align_finish into a slot"), pp_align_finish(c, 0.37, al, tw, 2)); }
    if (dports) dev_free(dports);
}

static void aux_align_refusals(int Cm, int B) {
    mark("case aux context %dx%d for the accumulator's refusals", Cm, B);
    pp_ctx* c = make_ctx(Cm, B);
    const int ns = 3, C = Cm + 4;
    const Outs o;
    std::vector<double> ports((size_t)ns * 4 * C * B, 0.5), freqs(C, 1400.0), P(ns, 0.003), par3((size_t)ns * 3, 0.0), w((size_t)ns * C, 1.0);
    std::vector<double> outv((size_t)4 * Cm * B);
    std::vector<int32_t> cmap((size_t)ns * C, 0);
    const void* src = ports.data();
    const double *f = freqs.data(), *Pp = P.data(), *p3 = par3.data(), *wp = w.data();
    double* out = outv.data();
#define REF(what, call) AUX(o, "refused: " what, call)
    REF("pp_align_add before pp_align_begin", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_finish before pp_align_begin", pp_align_finish(c, 0.0, out, out, -1));
    for (int B2 : {B + 1, 6, 4098}) REF("pp_align_begin nbin", pp_align_begin(c, 1, Cm, B2));
    REF("pp_align_begin npol", pp_align_begin(c, 0, Cm, B));
    REF("pp_align_begin npol", pp_align_begin(c, 5, Cm, B));
    REF("pp_align_begin nchan", pp_align_begin(c, 1, 0, B));
    REF("pp_align_begin null", pp_align_begin(nullptr, 1, Cm, B));
    { Outs g; AUX(g, "pp_align_begin for the refusals", pp_align_begin(c, 1, Cm, B)); }
    REF("pp_align_add nbin", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B == 64 ? 128 : 64, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_add npol", pp_align_add(c, src, PP_F64, 0, ns, 4, C, B, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_add npol 0", pp_align_add(c, src, PP_F64, 0, ns, 0, C, B, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_add identity with other channels", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B, f, 0, Pp, p3, wp, nullptr));
    for (int bad : {Cm, -1, INT32_MAX}) {
        cmap[(size_t)ns * C - 1] = bad;
        REF("pp_align_add chan_map out of range", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B, f, 0, Pp, p3, wp, cmap.data()));
    }
    cmap[(size_t)ns * C - 1] = 0;
    REF("pp_align_add shape", pp_align_add(c, src, PP_F64, 0, 0, 1, C, B, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_add dtype", pp_align_add(c, src, 7, 0, ns, 1, C, B, f, 0, Pp, p3, wp, cmap.data()));
    REF("pp_align_add freqs_stride", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B, f, 5, Pp, p3, wp, cmap.data()));
    for (int z = 0; z < 6; ++z) {
#define NZ(i, p) (z == (i) ? nullptr : (p))
        REF("pp_align_add null", pp_align_add(NZ(5, c), NZ(0, src), PP_F64, 0, ns, 1, C, B, NZ(1, f), 0, NZ(2, Pp), NZ(3, p3), NZ(4, wp), cmap.data()));
#undef NZ
    }
    REF("pp_align_finish null", pp_align_finish(c, 0.0, nullptr, out, -1));
    REF("pp_align_finish null", pp_align_finish(c, 0.0, out, nullptr, -1));
    REF("pp_align_finish null", pp_align_finish(nullptr, 0.0, out, out, -1));
    REF("pp_align_finish slot", pp_align_finish(c, 0.0, out, out, PP_MAX_SLOTS));
    REF("pp_align_finish rot_phase", pp_align_finish(c, NAN, out, out, -1));
    {
        Spec s; s.C = Cm; s.B = B;
        Batch b(s);
        mark("case aux refused: a batch is pending (accumulator)");
        ++g_ncase;
        mark("enqueue rc %d", pp_fit_enqueue(c, &b.in, &b.out));
        REF("pending pp_align_begin", pp_align_begin(c, 1, Cm, B));
        REF("pending pp_align_add", pp_align_add(c, src, PP_F64, 0, ns, 1, C, B, f, 0, Pp, p3, wp, cmap.data()));
        REF("pending pp_align_finish", pp_align_finish(c, 0.0, out, out, -1));
        mark("collect rc %d", pp_fit_collect(c));
    }
#undef REF
    MUST(pp_destroy(c));
}

static void aux_align_cases() {
    char tag[64];
    for (int B : {64, 2048, 1000})
        for (int small : {0, 1}) {
            const int Cm = 8, ns = small ? 7 : 3;
            mark("case aux context %dx%d accumulator budget=%s", Cm, B, small ? "small" : "large");
            pp_ctx* c = make_ctx(Cm, B);
            snprintf(tag, sizeof tag, "budget=%s", small ? "small" : "large");
            for (int f32 : {0, 1})
                for (int dev : {0, 1})
                    for (int npol : {1, 4})
                        for (int mapped : {0, 1}) {
                            // the budget: 2.4 subints' portraits of this shape
                            if (small) MUST(pp_set_option(c, "max_work_bytes", 2.4 * npol * (mapped ? Cm + 4 : Cm) * B * (f32 ? 4 : 8)));
                            aux_align_calls(c, B, Cm, ns, f32, dev, npol, mapped, tag);
                        }
            MUST(pp_destroy(c));
        }
    aux_align_refusals(8, 64);
    aux_align_refusals(8, 1000);
}

// ---- the Gaussian-component fit: pp_gauss_fit_begin / pp_gauss_residuals / pp_gauss_normal / pp_gauss_fit_end ------
// (after aux_align_cases(), so that everything in front keeps its place in the trace)  Every array exactly as long as
// the entry points read or write: the portrait f64 / f32, host / device; one, two and nine parameter sets with sets that
// differ in tau; the reduction on the resident rows, on host rows and on device rows; then the same fit joined
// (pp_gauss_fit_join: a band map of exactly C entries with a channel in no band, a join table of exactly nsets x njoin x 2)
static void aux_gauss_calls(pp_ctx* c, int B, int C, int f32, int dev, const char* tag) {
    const size_t esz = f32 ? 4 : 8, nrow = (size_t)C * B;
    std::vector<unsigned char> port(nrow * esz);
    for (size_t j = 0; j < nrow; ++j) {
        const double v = 0.5 + (j % 13) * 0.01;
        if (f32) ((float*)port.data())[j] = (float)v; else ((double*)port.data())[j] = v;
    }
    void* dport = dev ? dev_copy(port.data(), port.size()) : nullptr;
    std::vector<double> freqs(C), errs(C, 0.05);
    for (int j = 0; j < C; ++j) freqs[j] = 1100.0 + 800.0 * (j + 0.5) / C;
    char nm[200];
    auto name = [&](const char* fn, int nsets) {
        snprintf(nm, sizeof nm, "%s %s %dx%d %s %s nsets=%d", fn, tag, C, B, f32 ? "f32" : "f64", dev ? "device" : "host", nsets);
        return nm;
    };
    { Outs o; AUX(o, name("pp_gauss_fit_begin", 0), pp_gauss_fit_begin(c, dev ? dport : (const void*)port.data(), f32 ? PP_F32 : PP_F64, dev, C, B, freqs.data(), errs.data())); }
    const int ng = 2;
    for (int nsets : {1, 2, 9}) {
        std::vector<double> dc(nsets, 0.1), tau(nsets, 0.0), alpha(nsets, -4.0), comps((size_t)nsets * ng * 6), h(nsets > 1 ? nsets - 1 : 0, 1e-6);
        const double comp0[12] = {0.3, 0.0, 0.02, 0.0, 1.0, 0.0, 0.6, 0.0, 0.05, 0.0, 0.5, -1.0};
        for (int s = 0; s < nsets; ++s) {
            for (int q = 0; q < 12; ++q) comps[(size_t)s * 12 + q] = comp0[q] + 1e-6 * s;
            if (s % 2) tau[s] = 1e-3;
        }
        { Outs o; double* R = o.d((size_t)nsets * nrow);
          AUX(o, name("pp_gauss_residuals", nsets), pp_gauss_residuals(c, "010", 1500.0, nsets, dc.data(), tau.data(), alpha.data(), ng, comps.data(), R, nullptr)); }
        { Outs o; AUX(o, name("pp_gauss_residuals resident only", nsets), pp_gauss_residuals(c, "000", 1500.0, nsets, dc.data(), tau.data(), alpha.data(), ng, comps.data(), nullptr, nullptr)); }
        const int K = nsets - 1;
        { Outs o; double* chi2 = o.d(1); double* g = K ? o.d(K) : nullptr; double* G = K ? o.d((size_t)K * K) : nullptr;
          AUX(o, name("pp_gauss_normal resident", nsets), pp_gauss_normal(c, nullptr, 0, nsets, (int)nrow, K ? h.data() : nullptr, chi2, g, G)); }
        std::vector<double> rows((size_t)nsets * 77, 0.25);
        { Outs o; double* chi2 = o.d(1); double* g = K ? o.d(K) : nullptr; double* G = K ? o.d((size_t)K * K) : nullptr;
          AUX(o, name("pp_gauss_normal host rows", nsets), pp_gauss_normal(c, rows.data(), 0, nsets, 77, K ? h.data() : nullptr, chi2, g, G)); }
        { Outs o; double* chi2 = o.d(1); double* g = K ? o.d(K) : nullptr; double* G = K ? o.d((size_t)K * K) : nullptr;
          void* drows = dev_copy(rows.data(), rows.size() * 8);
          AUX(o, name("pp_gauss_normal device rows", nsets), pp_gauss_normal(c, (const double*)drows, 1, nsets, 77, K ? h.data() : nullptr, chi2, g, G));
          dev_free(drows); }
    }
    {
        const int njoin = 2;
        std::vector<int> band(C);
        for (int j = 0; j < C; ++j) band[j] = (j == C - 1) ? -1 : j % njoin;
        { Outs o; AUX(o, name("pp_gauss_fit_join", 0), pp_gauss_fit_join(c, njoin, band.data(), 0.003)); }
        for (int nsets : {1, 5}) {
            std::vector<double> dc(nsets, 0.1), tau(nsets, 0.0), alpha(nsets, -4.0), comps((size_t)nsets * ng * 6, 0.0), join((size_t)nsets * njoin * 2, 0.0);
            const double comp0[12] = {0.3, 0.0, 0.02, 0.0, 1.0, 0.0, 0.6, 0.0, 0.05, 0.0, 0.5, -1.0};
            for (int s = 0; s < nsets; ++s) {
                for (int q = 0; q < 12; ++q) comps[(size_t)s * 12 + q] = comp0[q];
                if (s % 2) tau[s] = 1e-3;
                // (set 0 and set 1 carry no rotation -- with and without tau --, the later ones a phase or a DM)
                if (s >= 2) join[((size_t)s * njoin + s % njoin) * 2 + s / 2 % 2] = (s / 2 % 2) ? 1e-3 : 0.1;
            }
            { Outs o; double* R = o.d((size_t)nsets * nrow);
              AUX(o, name("pp_gauss_residuals joined", nsets), pp_gauss_residuals(c, "010", 1500.0, nsets, dc.data(), tau.data(), alpha.data(), ng, comps.data(), R, join.data())); }
            { Outs o; AUX(o, name("pp_gauss_residuals joined, no table", nsets), pp_gauss_residuals(c, "000", 1500.0, nsets, dc.data(), tau.data(), alpha.data(), ng, comps.data(), nullptr, nullptr)); }
        }
    }
    { Outs o; AUX(o, name("pp_gauss_fit_end", 0), pp_gauss_fit_end(c)); }
    if (dport) dev_free(dport);
}

static void aux_gauss_refusals(int C, int B) {
    mark("case aux context %dx%d for the Gaussian fit's refusals", C, B);
    pp_ctx* c = make_ctx(C, B);
    const Outs o;
    const int big = 101;
    std::vector<double> port((size_t)C * B, 0.5), freqs(C, 1400.0), errs(C, 0.05), bad(C, 0.05), sc(big, 0.0), comps((size_t)big * 17 * 6, 0.1), h(big, 1e-6);
    std::vector<double> outv((size_t)big * big + (size_t)2 * C * B);
    bad[C - 1] = 0.0;
    const double *f = freqs.data(), *e = errs.data(), *z = sc.data(), *cp = comps.data();
    double* out = outv.data();
#define REF(what, call) AUX(o, "refused: " what, call)
    REF("pp_gauss_residuals before pp_gauss_fit_begin", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, nullptr));
    REF("pp_gauss_normal without resident rows", pp_gauss_normal(c, nullptr, 0, 1, C * B, nullptr, out, nullptr, nullptr));
    for (int B2 : {B + 1, 6, 8194}) REF("pp_gauss_fit_begin nbin", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B2, f, e));
    REF("pp_gauss_fit_begin nchan", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, 0, B, f, e));
    REF("pp_gauss_fit_begin dtype", pp_gauss_fit_begin(c, port.data(), 7, 0, C, B, f, e));
    REF("pp_gauss_fit_begin errs", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, f, bad.data()));
    REF("pp_gauss_fit_begin freqs", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, bad.data(), e));
    REF("pp_gauss_fit_begin null", pp_gauss_fit_begin(nullptr, port.data(), PP_F64, 0, C, B, f, e));
    REF("pp_gauss_fit_begin null", pp_gauss_fit_begin(c, nullptr, PP_F64, 0, C, B, f, e));
    REF("pp_gauss_fit_begin null", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, nullptr, e));
    REF("pp_gauss_fit_begin null", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, f, nullptr));
    REF("pp_gauss_residuals after a refused begin", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, nullptr));
    { Outs g; AUX(g, "pp_gauss_fit_begin for the refusals", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, f, e)); }
    REF("pp_gauss_normal before pp_gauss_residuals", pp_gauss_normal(c, nullptr, 0, 1, C * B, nullptr, out, nullptr, nullptr));
    REF("pp_gauss_residuals ngauss 17", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 17, cp, nullptr, nullptr));
    REF("pp_gauss_residuals ngauss 0", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 0, cp, nullptr, nullptr));
    REF("pp_gauss_residuals nsets 101", pp_gauss_residuals(c, "000", 1500.0, 101, z, z, z, 1, cp, nullptr, nullptr));
    REF("pp_gauss_residuals nsets 0", pp_gauss_residuals(c, "000", 1500.0, 0, z, z, z, 1, cp, nullptr, nullptr));
    REF("pp_gauss_residuals code", pp_gauss_residuals(c, "020", 1500.0, 1, z, z, z, 1, cp, nullptr, nullptr));
    for (int k = 0; k < 6; ++k) {
#define NZ(i, p) (k == (i) ? nullptr : (p))
        REF("pp_gauss_residuals null", pp_gauss_residuals(NZ(0, c), NZ(1, "000"), 1500.0, 1, NZ(2, z), NZ(3, z), NZ(4, z), 1, NZ(5, cp), nullptr, nullptr));
#undef NZ
    }
    { Outs g; AUX(g, "pp_gauss_residuals for the refusals", pp_gauss_residuals(c, "000", 1500.0, 2, z, z, z, 1, cp, nullptr, nullptr)); }
    {
        std::vector<int> band(C, 0), low(C, 0), high(C, 0);
        low[0] = -2; high[C - 1] = 2;
        REF("pp_gauss_residuals join table without a band map", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, z));
        REF("pp_gauss_fit_join njoin 0", pp_gauss_fit_join(c, 0, band.data(), 0.003));
        REF("pp_gauss_fit_join njoin 17", pp_gauss_fit_join(c, 17, band.data(), 0.003));
        REF("pp_gauss_fit_join index below -1", pp_gauss_fit_join(c, 2, low.data(), 0.003));
        REF("pp_gauss_fit_join index njoin", pp_gauss_fit_join(c, 2, high.data(), 0.003));
        REF("pp_gauss_fit_join P 0", pp_gauss_fit_join(c, 2, band.data(), 0.0));
        REF("pp_gauss_fit_join P negative", pp_gauss_fit_join(c, 2, band.data(), -1.0));
        REF("pp_gauss_fit_join P infinite", pp_gauss_fit_join(c, 2, band.data(), HUGE_VAL));
        REF("pp_gauss_fit_join P nan", pp_gauss_fit_join(c, 2, band.data(), NAN));
        REF("pp_gauss_fit_join null", pp_gauss_fit_join(nullptr, 2, band.data(), 0.003));
        REF("pp_gauss_fit_join null", pp_gauss_fit_join(c, 2, nullptr, 0.003));
        REF("pp_gauss_residuals join table after refused joins", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, z));
        { Outs g; AUX(g, "pp_gauss_fit_join for the refusals", pp_gauss_fit_join(c, 2, band.data(), 0.003)); }
        { Outs g; AUX(g, "pp_gauss_residuals joined for the refusals", pp_gauss_residuals(c, "000", 1500.0, 2, z, z, z, 1, cp, nullptr, z)); }
        // (a second begin clears the band map)
        { Outs g; AUX(g, "pp_gauss_fit_begin again", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, f, e)); }
        REF("pp_gauss_residuals join table after a second begin", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, z));
        { Outs g; AUX(g, "pp_gauss_residuals for the refusals, again", pp_gauss_residuals(c, "000", 1500.0, 2, z, z, z, 1, cp, nullptr, nullptr)); }
    }
    REF("pp_gauss_normal other nsets than resident", pp_gauss_normal(c, nullptr, 0, 3, C * B, h.data(), out, out, out));
    REF("pp_gauss_normal other nrow than resident", pp_gauss_normal(c, nullptr, 0, 2, C * B - 1, h.data(), out, out, out));
    REF("pp_gauss_normal nsets 101", pp_gauss_normal(c, port.data(), 0, 101, 2, h.data(), out, out, out));
    REF("pp_gauss_normal nsets 0", pp_gauss_normal(c, port.data(), 0, 0, 2, h.data(), out, out, out));
    REF("pp_gauss_normal nrow", pp_gauss_normal(c, port.data(), 0, 2, 0, h.data(), out, out, out));
    h[0] = 0.0;
    REF("pp_gauss_normal zero step", pp_gauss_normal(c, nullptr, 0, 2, C * B, h.data(), out, out, out));
    h[0] = 1e-6;
    REF("pp_gauss_normal null", pp_gauss_normal(nullptr, nullptr, 0, 2, C * B, h.data(), out, out, out));
    REF("pp_gauss_normal null", pp_gauss_normal(c, nullptr, 0, 2, C * B, nullptr, out, out, out));
    REF("pp_gauss_normal null", pp_gauss_normal(c, nullptr, 0, 2, C * B, h.data(), nullptr, out, out));
    REF("pp_gauss_normal null", pp_gauss_normal(c, nullptr, 0, 2, C * B, h.data(), out, nullptr, out));
    REF("pp_gauss_normal null", pp_gauss_normal(c, nullptr, 0, 2, C * B, h.data(), out, out, nullptr));
    REF("pp_gauss_fit_end null", pp_gauss_fit_end(nullptr));
    {
        Spec s; s.C = C; s.B = B;
        Batch b(s);
        mark("case aux refused: a batch is pending (Gaussian fit)");
        ++g_ncase;
        mark("enqueue rc %d", pp_fit_enqueue(c, &b.in, &b.out));
        REF("pending pp_gauss_fit_begin", pp_gauss_fit_begin(c, port.data(), PP_F64, 0, C, B, f, e));
        REF("pending pp_gauss_residuals", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, nullptr));
        { std::vector<int> band(C, 0); REF("pending pp_gauss_fit_join", pp_gauss_fit_join(c, 1, band.data(), 0.003)); }
        REF("pending pp_gauss_normal", pp_gauss_normal(c, nullptr, 0, 2, C * B, h.data(), out, out, out));
        REF("pending pp_gauss_fit_end", pp_gauss_fit_end(c));
        mark("collect rc %d", pp_fit_collect(c));
    }
    { Outs g; AUX(g, "pp_gauss_fit_end", pp_gauss_fit_end(c)); }
    REF("pp_gauss_residuals after pp_gauss_fit_end", pp_gauss_residuals(c, "000", 1500.0, 1, z, z, z, 1, cp, nullptr, nullptr));
    { std::vector<int> band(C, 0); REF("pp_gauss_fit_join after pp_gauss_fit_end", pp_gauss_fit_join(c, 1, band.data(), 0.003)); }
#undef REF
    MUST(pp_destroy(c));
}

static void aux_gauss_cases() {
    char tag[64];
    for (int B : {64, 2048, 1000})
        for (int profile : {0, 1}) {
            const int C = 3;
            mark("case aux context %dx%d Gaussian fit profile=%d", C, B, profile);
            pp_ctx* c = make_ctx(C, B);
            MUST(pp_set_option(c, "profile", profile));
            snprintf(tag, sizeof tag, "profile=%d", profile);
            for (int f32 : {0, 1})
                for (int dev : {0, 1}) aux_gauss_calls(c, B, C, f32, dev, tag);
            MUST(pp_destroy(c));
        }
    aux_gauss_refusals(8, 64);
    aux_gauss_refusals(8, 1000);
}

int main() {
    g_mark = (void (*)(const char*))dlsym(RTLD_DEFAULT, "hip_stub_mark");
    if (!g_mark) fprintf(stderr, "trace_driver: no hip_stub_mark (LD_PRELOAD libhip_stub.so): cases go unnamed\n");
    for (int B : {64, 1024, 2048, 1000})
        for (int C : {48, 256, 640, 2304}) shape_cases(B, C);
    entry_cases();
    chain("chain");
    option_cases();
    aux_cases();
    aux_align_cases();
    aux_gauss_cases();
    printf("trace_driver: done\n");
    return 0;
}
