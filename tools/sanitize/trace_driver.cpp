// Walks the HOST driver of libpptoas_hip.so through a matrix of small batches against the no-op HIP stub
// (hip_stub.cpp with PP_STUB_TRACE set): every flow, entry point and option once, so that the stub's trace -- every
// launch, copy, memset, event and wait in the order the library queues them -- can be compared between two builds of
// the library (make trace-run; a refactor of the driver must leave the trace byte-identical).  Single-threaded, C ABI
// only: the same source builds against any commit's library.  Kernels do not run and the stub's device memory is all
// zeros, so every host decision that reads a device count sees "all done": the weak-pilot re-seed, the recentre loop,
// the re-transform of listed subints and the re-fit on collect are NOT reached here (the GPU suite asserts those).
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

int main() {
    g_mark = (void (*)(const char*))dlsym(RTLD_DEFAULT, "hip_stub_mark");
    if (!g_mark) fprintf(stderr, "trace_driver: no hip_stub_mark (LD_PRELOAD libhip_stub.so): cases go unnamed\n");
    for (int B : {64, 1024, 2048, 1000})
        for (int C : {48, 256, 640, 2304}) shape_cases(B, C);
    entry_cases();
    chain("chain");
    option_cases();
    printf("trace_driver: done\n");
    return 0;
}
