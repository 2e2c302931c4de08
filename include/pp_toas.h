/*
 * pp_toas.h -- C ABI of the MI355X wideband-TOA fit engine (libpptoas_hip.so).
 *
 * The reference (pennucci/PulsePortraiture) is pure Python with no FFI of its
 * own; the drop-in boundary is therefore the Python call signature, and this
 * header is what the Python shims in pulseportraiture_amd/ bind with ctypes
 * (INTEGRATION.md shows the stub a maintainer would add to the reference).
 * Each entry point names the reference interface it replaces (file:line under
 * the reference tree).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types;
 *   - every function returns an int status: PP_OK (0) or a negative PP_E*
 *     code, with a human-readable message available from pp_last_error();
 *     no exception crosses the boundary;
 *   - per-subint numerical status goes in return_code[] (PP_RC_*), the fit
 *     itself never fails the call (reference: pptoaslib.py:1016-1033);
 *   - the caller owns every host buffer; the library copies what it needs and
 *     keeps no host pointer after return.  Device scratch lives in the opaque
 *     context.  One context per (host thread, GPU); calls on one context are
 *     serialised by the caller.
 *   - portraits are C-contiguous [nsub][nchan][nbin]; nbin is a power of two
 *     in [32, 8192] (tuned plans) or any even number in [8, 4096] (every entry
 *     point, by the chirp-z route: the reference's numpy.fft takes every nbin).
 *   - a subint's outputs are a function of that subint's inputs alone: whatever
 *     else is in the batch, however it is cut into sub-batches, shards or ranks,
 *     the same bits come back (the reference fits subints in a plain loop,
 *     pptoas.py:344-489).
 */
#ifndef PP_TOAS_H
#define PP_TOAS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 11

/* status codes */
#define PP_OK 0
#define PP_EINVAL (-1)   /* bad argument */
#define PP_EHIP (-2)     /* HIP runtime error */
#define PP_ENOMEM (-3)   /* device memory */
#define PP_ESTATE (-4)   /* call order / missing model */
#define PP_ENOTSUP (-5)  /* the request is valid but this shape / option set has no device path
                            (pp_fit_in.ref_seed: the caller then forms the guess with
                            pp_reference_phase_seed and fits in a second call) */

/* sample types of portraits */
#define PP_F64 0
#define PP_F32 1

/* per-subint return codes (return_code[]); 2 is what the reference's
 * trust-ncg normally reports with gtol=-1 (pptoaslib.py:1002) */
#define PP_RC_GRAD 0      /* gradient below tolerance */
#define PP_RC_MAXITER 1   /* iteration limit */
#define PP_RC_STALL 2     /* no predicted reduction left: converged to rounding */
#define PP_RC_NAN 3       /* NaN / singular objective */

/* minimiser (pp_fit_in.method; the reference's `method` argument,
 * pptoaslib.py:932, 993-1010).  The reference's answer for GM and scattering
 * fits is where SciPy's trust-ncg stops with gtol = -1 ("no predicted
 * reduction" in floating point, after truncated conjugate-gradient steps), up
 * to ~1.5e-9 rot short of the optimum: PP_METHOD_TRUST_NCG walks that very
 * iteration (scipy/optimize/_trustregion.py, _trustregion_ncg.py) on the device
 * and stops where it stops; PP_METHOD_NEWTON converges to the rounding of the
 * objective in fewer evaluations (what 'Newton-CG' and 'TNC' also aim at). */
#define PP_METHOD_TRUST_NCG 0
#define PP_METHOD_NEWTON 1

/* normalisation of pp_channel_noise: normalize_portrait's methods (pplib.py:2462-2507) */
#define PP_NORM_NONE 0
#define PP_NORM_MEAN 1
#define PP_NORM_MAX 2
#define PP_NORM_PROF 3    /* the caller's divisor per row */
#define PP_NORM_RMS 4
#define PP_NORM_ABS 5

/* pp_channel_noise_fit: what the rows are, and find_kc's model function (pplib.py:1448-1463) */
#define PP_NOISEFIT_ROWS 0    /* profiles [nrows][nbin] */
#define PP_NOISEFIT_POWS 1    /* power spectra [nrows][nbin / 2 + 1], f64 */
#define PP_KC_EXP_DC 0        /* b exp(-a k) + dc */
#define PP_KC_HALF_TRI 1      /* half_triangle_function (pplib.py:1436-1446) */

typedef struct pp_ctx pp_ctx;

/* Streams.  A context launches everything on its own non-blocking HIP stream
 * (pp_stream) and every entry point returns after synchronising it, so outputs --
 * host or device -- are complete on return.  Device pointers passed IN (portraits,
 * errs, masks, output tensors) must be complete as well: if they were produced on
 * another stream (e.g. an asynchronous copy or kernel of the caller's framework),
 * synchronise that stream, or make pp_stream wait on an event of it, before the
 * call.  The Python binding does the former for torch tensors. */

/* ---- context ---------------------------------------------------------- */
int pp_abi_version(void);
const char* pp_last_error(void);
int pp_create(int device_id, pp_ctx** out);
int pp_destroy(pp_ctx* ctx);
/* block until everything queued on the context's stream has finished.  A batch enqueued with pp_fit_enqueue whose
 * solve and post-fit stage were still waiting for a next batch to carry them (option "fuse_tail") gets them queued
 * first, by the stand-alone kernels: after pp_synchronize the DEVICE-resident outputs of every enqueued batch
 * (records_dev, per-channel arrays with chan_on_device) are written; host outputs are complete after pp_fit_collect. */
int pp_synchronize(pp_ctx* ctx);
/* the hipStream_t the context launches on (as void*) */
void* pp_stream(pp_ctx* ctx);

/* Options (name, value):
 *   "harm_eps"     relative |m_nk| threshold below which the model's trailing
 *                  harmonics are dropped from the cross-spectrum (0 = keep all;
 *                  default 2^-50, DESIGN.md "Harmonic truncation")
 *   "max_iter"     trust-region iteration limit (default 64; reference: 1000)
 *   "profile"      1 = record HIP events around every kernel (pp_kernel_times)
 *   "check_every"  iterations between host checks of the active count
 *   "lagged_check" 1 (default) = evaluation loops without the scattering model read that count
 *                  one iteration behind, so the GPU never waits for the host's look at it
 *                  (one extra, empty iteration is queued at the end); 0 = synchronous checks
 *   "x_pad"        pad (elements) of the rows of a stored cross-spectrum (default 0: measured
 *                  neutral)
 *   "max_work_bytes"  cap on device scratch per call (larger batches are split)
 *   "taylor"       1 (default) = fits without scattering first try the
 *                  per-channel Taylor-model solve; 0 = always iterate
 *   "taylor_recentre"  fits of phase / DM whose Taylor model fails its certificate (poor
 *                  guesses) are expanded again about the tentative answer -- one more pass
 *                  over those subints' data -- before falling back to evaluations over a
 *                  stored cross-spectrum: how many times (default 1, 0 = never)
 *   "seed_chan_stride"  device phase seed (seed_ns > 0) of fits without scattering:
 *                  the seed is formed in a pilot pass over every n-th channel (default
 *                  16; 1 = from all channels, with the cross-spectrum stored), then the
 *                  usual single pass runs at the seeded phase
 *   "seed_min_snr" pilot seeds whose correlation peak stands less than this many rms
 *                  above the mean of the grid (default 8) are redone from all channels
 *   "seed_ndm", "seed_dm_step"  the coarse seed grid is (phi, DM): seed_ns phases x
 *                  seed_ndm trial DMs spaced seed_dm_step [pc cm^-3] about the guessed DM
 *                  (centred; an odd count keeps the guess itself); the DM of the highest
 *                  correlation peak, refined by the parabola through it and its
 *                  neighbours, seeds the DM, and the phase is seeded at it.  Default 1 trial:
 *                  the reference's seed trusts the header DM (pptoas.py:421-457)
 *   "paired_split" 1 (default) = 2048-bin rows whose template keeps fewer than 512
 *                  harmonics take the transform kernel that does the last FFT stage
 *                  and the even/odd split in registers; 0 = the generic kernel
 *   "one_exchange" 1 (default) = 2048- and 1024-bin rows fitted without scattering (noise
 *                  given or measured) take the transform kernels whose FFT crosses the LDS
 *                  once (first exchange by lane swaps) and whose split reads only the partner
 *                  harmonics -- k_xspec_q1024 / k_xspec_qf<1024> / k_xspec_qf<512> --, and the
 *                  single-pass reference seed (pp_seed_ref) exists; 0 = the kernels above
 *   "cu_tables"    1 (default) = f64 2048-bin rows with the noise given, a template cut below 512
 *                  harmonics and neither a channel mask, an `act` list nor per-subint templates take
 *                  k_xspec_cu1024: k_xspec_q1024's row with the CU's eight waves in one workgroup
 *                  that shares LDS tables of the row-invariant twiddle powers (bitwise the same
 *                  results); 0 = k_xspec_q1024.  A device that does not grant the kernel its 161 792 B
 *                  of LDS keeps k_xspec_q1024 whatever the option says
 *   "cu_grid_cap"  k_xspec_cu1024: at most this many workgroups; 0 (default) = one per CU.  For tests
 *                  (with one workgroup every wave of a small batch has rows and works tickets between them)
 *   "scat_model"   scattering fits: 1 (default) = once the trust-ncg iteration is
 *                  predicted to stay within its range, ONE more pass over the
 *                  cross-spectrum leaves a degree-8 polynomial model of every channel's
 *                  sums in (phi_n, tau_n) and the remaining evaluations are made on it,
 *                  each with a truncation certificate (DESIGN.md "Scattering fits");
 *                  2 = also for method 'newton' (whose few closing iterations do not
 *                  repay the pass); 0 = every evaluation is a pass over the cross-spectrum
 *   "fuse_scat"    1 (default) = scattering fits of 2048-bin portraits (template cut below 512
 *                  harmonics, noise given) take the transform that stores the cross-spectrum AND
 *                  forms the first evaluation's sums while it is in registers (one pass over the
 *                  stored cross-spectrum fewer); 0 = the general transform + an evaluation pass
 *   "x_f32"        1 = scattering fits keep their stored cross-spectrum X_nk = d_nk m_nk* as
 *                  pairs of floats (half the bytes of every evaluation pass, all arithmetic f64;
 *                  without the closing model).  Off by default: it buys 8 % on configs[3] and
 *                  costs chi2 its 1e-10 agreement with the reference
 *   "scat_model_tol"  predicted relative truncation below which that pass is asked
 *                  for (default 1e-10; the certificate guards the result either way)
 *   "fps_finish"   pp_fit_phase_shift_batch after its brute grid: 0 (default) = Newton to
 *                  the exact local optimum; 1 = what scipy.optimize.brute does by default
 *                  and the reference therefore returns (pplib.py:2085): the Nelder-Mead
 *                  simplex to xtol = ftol = 1e-4, operation by operation
 *   "skip_masked"  1 (default) = channels a subint's chan_mask removes are not transformed at
 *                  all: the transform walks a compact list of the (subint, channel) rows in use,
 *                  as the reference slices the good channels away before its fit
 *                  (pptoas.py:384-397); 0 = every row is transformed and masked ones get weight 0
 *   "eager_flush"  1 (default) = the stream is queried once the transform has been queued, which makes the
 *                  runtime hand what is queued to the GPU at once instead of with the next blocking call
 *   "solve_threads"  one-pass flow: threads per subint of the solve on the Taylor model (0 = default: 64 for a
 *                  band of up to 512 channels, 128 up to 1024, 256 beyond; 64 / 128 / 256 / 512 force it).  The
 *                  channel sums are taken in a different order for each: results agree to rounding, not bitwise
 *   "solve_prefetch"  that solve at more than 2048 channels: 0 (default) = each Taylor row fetched when its turn comes
 *                  (the batch's rows exceed the Infinity Cache there: the less a CU keeps in flight, the less it evicts),
 *                  1 = rows prefetched two ahead as for narrower bands
 *   "solve_cache"  ... channels whose weight, phase geometry and template power that solve keeps in LDS
 *                  (-1 = default: all, up to 8 per thread; 0 = formed again on every evaluation)
 *   "finalize_regs"  post-fit stage of fits without scattering: 1 (default) = each thread holds its (up to 8)
 *                  channels' numbers in registers over the stage's passes, 64 ... 512 threads per subint by band
 *                  width; 0 = the pass-by-pass kernel every other fit uses; 64 / 128 / 256 / 512 force a width
 *   "copy_kernels"  1 (default) = the packed block of small inputs and the packed per-subint outputs cross PCIe by a
 *                  kernel that reads / writes the pinned staging block directly; 0 = by hipMemcpyAsync (a copy
 *                  command between two kernels hands the stream to the copy engine and back: ~0.05 ms per batch)
 *   "fuse_tail"    pp_fit_enqueue, one-pass fits of 2048-bin portraits: 1 (default) = the batch's solve on the Taylor model and
 *                  its post-fit stage are NOT queued behind its transform; the transform of the next enqueued batch works
 *                  them off, one subint per ticket, between its own rows (one wave per ticket walking the waves of the
 *                  stand-alone kernels in turn: bitwise their results), and the batch's outputs and event follow that
 *                  transform on the stream.  The reference-seed flow (pp_seed_ref, what get_TOAs runs by default) is part
 *                  of this since round 6: its pass (k_xspec_qr1024) carries tickets, and ITS tail -- the guess's spectrum
 *                  from the pass's chunk partials, fit_phase_shift with SciPy's simplex, the start points, then solve and
 *                  post-fit stage -- is a ticket of the next pass (+2.7 % fits/s, profiles/r06_refseed_tail_ab.txt).  If no
 *                  batch follows (pp_fit_collect or pp_synchronize comes first), the next batch cannot carry them (another
 *                  row length, scattering, a device seed) or is much smaller than the one it would carry (fewer than half
 *                  as many waves as tickets), the stand-alone kernels are queued then.  Keep THREE batches enqueued to hide
 *                  it all (a batch completes one transform later).  +0.6 ... 2.9 % fits/s (profiles/r05_fuse_tail_ab.txt);
 *                  0 = solve and post-fit stage queued at once
 *   "tail_virtual" experiments: 1 = the stand-alone solve / post-fit kernels themselves in their one-wave form
 *   "check_from"   evaluation loop: the first iteration after which the host looks at the count of unfinished subints
 *                  (default 2; trust-ncg scattering fits with the closing model: 5 at least -- none is done before)
 *   "refseed_stride"  pp_seed_ref: channel stride of the pilot pass on wide bands (0 = default 64; at least 32 pilot
 *                  channels are kept).  128 measured +0.4 % at 4096 channels: not taken, a thinner pilot is a weaker one
 *   "overlap_post"  pp_fit_enqueue: 1 = the solve and post-fit stage of a deferred batch are queued on a second,
 *                  higher-priority stream of the context behind an event of its transform, with a work-buffer set
 *                  of their own, so that they may run beside the NEXT batch's transform; 0 (default) = one stream.
 *                  Same results either way.  Measured neutral (profiles/r05_overlap_ab.txt): the persistent transform
 *                  holds every wave slot, the two kernels alternate instead of co-residing
 *   "coarse_newton"  1 (default) = scattering fits with PP_METHOD_NEWTON first iterate on every 16th channel
 *                  (each evaluation reads a sixteenth of the stored cross-spectrum) and start the
 *                  full-channel iteration from that answer -- the optimum does not depend on the path --;
 *                  0 = every evaluation over all channels.  nfeval includes the coarse evaluations, npass
 *                  counts full passes.  (PP_METHOD_TRUST_NCG retraces SciPy's iterates and is not affected.)
 *   "nfev_shadow"  one-pass flow, method trust-ncg: how SciPy's one-point cache is mirrored when nfeval is
 *                  counted.  0: proposals are compared as displacements from the expansion point
 *                  (resolution 1e-21: the closing proposal p = -H^-1 g is always a new point and counts);
 *                  1: on the absolute iterate fl(x + p) as SciPy forms it; 2: as 1, with the model evaluated
 *                  at the rounded point; -1 (default): 1 for one-parameter fits, 0 otherwise -- the rule
 *                  that agrees with the reference's count most often, family by family (3000 random fits,
 *                  profiles/r04_parity_sweep.txt; the closing p is rounding noise of whoever computes it, so
 *                  the last unit of nfeval is a coin toss of the reference's own arithmetic)
 *   "moments_in_xspec"  1 (default) = the Taylor moments are accumulated inside
 *                  the transform kernel and no cross-spectrum is stored; 0 = store
 *                  the cross-spectrum and take the moments in a second pass
 */
int pp_set_option(pp_ctx* ctx, const char* name, double value);
/* the current value of an option (a caller that changes one for a call -- max_iter = 0 to
 * evaluate only -- reads it first and puts it back) */
int pp_get_option(pp_ctx* ctx, const char* name, double* value);

/* ---- model portraits ---------------------------------------------------- */
/* Upload an nchan x nbin template into slot `slot` (0..PP_MAX_SLOTS-1), rFFT it
 * on the device, zero the DC harmonic and keep sum_k |m_nk|^2 per channel.
 * Replaces the model half of pptoaslib.py:978-979 (and pplib.py:2123-2124).
 * `on_device` != 0 means `portrait` is a device pointer on this GPU. */
#define PP_MAX_SLOTS 64
int pp_model_set(pp_ctx* ctx, int slot, const void* portrait, int dtype,
                 int on_device, int nchan, int nbin);
/* number of harmonics (of nbin/2) kept for this slot after truncation */
int pp_model_nharm(pp_ctx* ctx, int slot);
/* DC harmonic of every channel of the slot's template, dc[nchan] (host): nbin x the
 * profile mean the flux estimate of get_TOAs uses (pptoas.py:554-575) */
int pp_model_dc(pp_ctx* ctx, int slot, double* dc);
/* nchan and nbin of the slot's template (PP_ESTATE: the slot is not set): what a caller that hands a
 * destination to pp_fake_portraits sizes it by */
int pp_model_shape(pp_ctx* ctx, int slot, int* nchan, int* nbin);

/* Gaussian-component template portraits synthesised on the device (.gmodel
 * files: read_model / gen_gaussian_portrait / gaussian_profile / evolve_parameter,
 * pplib.py:2867-2953, 853-930, 770-825, 996-1046).  code[3]: '0' = power-law,
 * '1' = linear evolution of (loc, wid, amp); comps[ngauss][6] = loc, m_loc, wid,
 * m_wid, amp, m_amp at nu_ref; dc = baseline; tau_rot = scattering time at nu_ref
 * in rotations (TAU / P, 0 = none), scaled as (nu/nu_ref)^alpha and applied in the
 * Fourier domain (pplib.py:915-922).  pp_gaussian_portrait writes the
 * [nchan][nbin] f64 portrait (host or device pointer); pp_model_set_gaussian
 * loads it straight into a model slot (no host copy of the portrait at all). */
int pp_gaussian_portrait(pp_ctx* ctx, int nchan, int nbin, const double* freqs,
                         const char* code, double nu_ref, double dc, double tau_rot,
                         double alpha, int ngauss, const double* comps,
                         double* portrait, int out_on_device);
int pp_model_set_gaussian(pp_ctx* ctx, int slot, int nchan, int nbin,
                          const double* freqs, const char* code, double nu_ref,
                          double dc, double tau_rot, double alpha, int ngauss,
                          const double* comps);

/* Spline (PCA + B-spline) template portraits synthesised on the device (.spl files:
 * read_spline_model / gen_spline_portrait, pplib.py:2955-2987, 932-956): row n =
 * basis[0] + sum_c splev(freqs[n]; t, coefs[c], degree) * basis[1 + c], where basis
 * [ncomp + 1][nbin] holds the mean profile and the eigenvectors (resampled to nbin
 * on the host when the model's own resolution differs), t[nknots] the knots and
 * coefs[ncomp][nknots] the B-spline coefficients of scipy's `tck` (FITPACK layout).
 * The curve is evaluated like scipy.interpolate.splev(..., ext=0).  pp_spline_portrait
 * writes the [nchan][nbin] f64 portrait (host or device pointer);
 * pp_model_set_spline loads it straight into a model slot. */
int pp_spline_portrait(pp_ctx* ctx, int nchan, int nbin, const double* freqs, int ncomp,
                       const double* basis, int nknots, const double* t,
                       const double* coefs, int degree, double* portrait,
                       int out_on_device);
int pp_model_set_spline(pp_ctx* ctx, int slot, int nchan, int nbin, const double* freqs,
                        int ncomp, const double* basis, int nknots, const double* t,
                        const double* coefs, int degree);

/* Instrumental response applied to the template resident in `slot`, in the Fourier
 * domain on the device (instrumental_response_port_FT, pptoaslib.py:145-179, as
 * get_TOAs(add_instrumental_response=True) uses it, pptoas.py:388-394):
 * m_nk <- m_nk * rconst[k] * sinc(k smear_wid[n]).  rconst: host [nbin/2 + 1]
 * interleaved (re, im), the product of the constant responses, or NULL; smear_wid:
 * host [nchan], the dispersive smearing width of every channel in rotations
 * (8.3e-6 chan_bw / nu_GHz^3 / P as the reference forms it; 0 = none), or NULL.  The
 * harmonic truncation of the slot is re-derived. */
int pp_model_apply_response(pp_ctx* ctx, int slot, const double* rconst,
                            const double* smear_wid);

/* ---- the batched fit ----------------------------------------------------- */
/* The reference's own initial phase guess formed INSIDE the fit, from the same single pass over
 * the portraits (pp_fit_in.ref_seed; pptoas.py:421-457):
 *   rot_prof_i = np.average(rotate_data(port_i, 0.0, DM_i, P_i, freqs_i, nu_mean_i), axis=0,
 *                           weights=weights_i)                    (DM_i = init_params[i][1])
 *   phi_i      = fit_phase_shift(rot_prof_i, model_prof_i, Ns=Ns, bounds=(lo, hi)).phase
 *   init_params[i][0] <- phase_transform(phi_i, DM_i, nu_mean_i, nu_fits[i][0], P_i, mod=True)
 * and the fit then starts from there (init_params[.][0] as given is ignored).  The transform
 * kernel takes the per-channel Taylor model about a provisional phase (a pilot pass over every
 * 16th channel) together with the rotated channel sums; the iteration starts off-centre, at the
 * reference's guess.  A scattering fit iterates over the stored cross-spectrum instead: the
 * transform that stores it takes the rotated channel sums as well (rotation by the DM guess
 * alone, no pilot) and the iteration starts AT the reference's guess.  Available for 2048-bin
 * portraits whose template keeps fewer than 512 harmonics, nchan a multiple of 32 (and >= 256
 * without scattering), errs given, GM guesses 0: otherwise pp_fit_portrait_batch returns
 * PP_ENOTSUP and nothing has been done. */
typedef struct {
    const double* weights;       /* [nsub][nchan] weights of the channel mean (0 = channel not used);
                                    host, or device when pp_fit_in.aux_on_device; NULL = all 1 */
    const double* model_profs;   /* host: [nsub][nbin], or [nbin] when model_prof_stride == 0 */
    int64_t model_prof_stride;   /* 0 or nbin */
    const double* nu_mean;       /* host [nsub]: mean frequency of the channels used */
    double lo, hi;               /* bounds of the brute grid (-0.5, 0.5) */
    int32_t Ns;                  /* its size (100) */
    int32_t finish;              /* 1 = SciPy brute's simplex finish (what the reference returns), 0 = Newton */
    double* seed_phase;          /* host [nsub] out, or NULL: the phase guesses formed (at nu_fit) */
} pp_seed_ref;

typedef struct {
    int32_t nsub, nchan, nbin;
    const void* data;          /* [nsub][nchan][nbin] */
    int32_t data_dtype;        /* PP_F64 | PP_F32 */
    int32_t data_on_device;    /* data is a device pointer */
    const int32_t* model_slot; /* [nsub] or NULL (= slot 0 for all) */
    const double* freqs;       /* [nsub][nchan] or [nchan] if freqs_stride==0 */
    int64_t freqs_stride;      /* 0 or nchan */
    const double* errs;        /* [nsub][nchan] time-domain sigma, or NULL:
                                  measured per channel as get_noise_PS
                                  (pplib.py:2227-2247) */
    const uint8_t* chan_mask;  /* [nsub][nchan], 1 = fit this channel, or NULL */
    int32_t aux_on_device;     /* errs and chan_mask are device pointers */
    const double* P;           /* [nsub] spin period [s] */
    const double* init_params; /* [nsub][5] phi, DM, GM, tau|log10 tau, alpha */
    const double* nu_fits;     /* [nsub][3] or NULL; NaN = mean(freqs) */
    const double* nu_outs;     /* [nsub][3] or NULL; NaN = zero-covariance */
    int32_t fit_flags[5];
    int32_t log10_tau;
    int32_t option;            /* get_nu_zeros option (pptoaslib.py:734) */
    int32_t is_toa;
    int32_t method;            /* PP_METHOD_* */
    int32_t seed_ns;           /* > 0: ignore init_params[.][0] and seed the phase on
                                  the device: seed_ns-point grid over [-0.5, 0.5] of
                                  the channel-summed cross-correlation at the guessed
                                  DM/GM/tau, polished to its maximum (the role of
                                  pptoas.py:421-457, fit_phase_shift with Ns=100) */
    const pp_seed_ref* ref_seed; /* NULL, or: form the reference's own phase guess in the pass (above) */
} pp_fit_in;

typedef struct {
    double* params;       /* [nsub][5]  phi(nu_out), DM, GM, tau(nu_out), alpha */
    double* param_errs;   /* [nsub][5]  0 where not fitted */
    double* nu_refs;      /* [nsub][3]  nu_DM, nu_GM, nu_tau of the outputs */
    double* cov;          /* [nsub][5][5] covariance, zero rows/cols if unfit */
    double* chi2;         /* [nsub] */
    double* red_chi2;     /* [nsub] */
    double* snr;          /* [nsub] */
    int32_t* nfeval;      /* [nsub] objective evaluations as the reference reports them: SciPy's
                             `nfev` (pptoaslib.py:1017 `nfeval = results.nfev`) -- the initial point,
                             every proposal that is not the point evaluated last (SciPy's one-point
                             cache), and the proposal SciPy evaluates before it tests the predicted
                             reduction and stops.  Most of them cost no pass over the data here. */
    int32_t* return_code; /* [nsub] PP_RC_* */
    int32_t chan_on_device; /* the three per-channel outputs are device pointers */
    double* scales;       /* [nsub][nchan] or NULL */
    double* scale_errs;   /* [nsub][nchan] or NULL */
    double* channel_snrs; /* [nsub][nchan] or NULL */
    double* obj_f;        /* [nsub]      objective at init_params, or NULL */
    double* obj_grad;     /* [nsub][5]   its gradient, or NULL */
    double* obj_hess;     /* [nsub][25]  its Hessian, or NULL */
    double* duration;     /* [1] seconds of device time for the whole call */
    int32_t* npass;       /* [nsub] or NULL: how many of those evaluations were passes over the
                             portraits or the stored cross-spectrum (1 for a fit solved on the
                             Taylor model of its single pass) */
    double* records_dev;  /* DEVICE pointer [nsub][PP_RECORD_WIDTH] or NULL: one fixed-size
                             TOA record per subint left in HBM -- phi, DM, GM, tau, alpha,
                             their five errors, nu_DM, nu_GM, nu_tau, chi2, red_chi2, snr,
                             nfeval, return_code -- what the ranks of a multi-GPU job
                             gather (one RCCL gather at the end of the job) */
} pp_fit_out;
#define PP_RECORD_WIDTH 18

/* Fit every subint of the batch: rFFT, cross-spectrum, trust-region Newton
 * solve, zero-covariance frequencies, errors, S/N, chi2.  One call replaces
 * nsub calls of fit_portrait_full (pptoaslib.py:928-1096), i.e. the body of
 * the per-subint loop of GetTOAs.get_TOAs (pptoas.py:344-489).
 * max_iter == 0 only evaluates the objective at init_params (obj_* outputs). */
int pp_fit_portrait_batch(pp_ctx* ctx, const pp_fit_in* in, pp_fit_out* out);

/* Asynchronous form.  pp_fit_submit copies the two argument blocks, starts
 * the batch on a worker thread of the context and returns at once; pp_fit_wait blocks
 * until it has finished and returns what pp_fit_portrait_batch would have returned (the
 * message of a failure is then available from pp_last_error on the waiting thread);
 * pp_fit_poll returns 1 once the batch is complete, 0 while it runs.  Every buffer the
 * argument blocks point to must stay valid and untouched until pp_fit_wait returns; one
 * batch per context may be in flight, and no other call may be made on that context
 * meanwhile (PP_ESTATE on a second submit).  Batches submitted on two contexts of one
 * GPU overlap: one context's host-to-device copies run beside the other's kernels.
 * The reference has no counterpart: its loop over subints is serial
 * (pptoas.py:344-489). */
int pp_fit_submit(pp_ctx* ctx, const pp_fit_in* in, pp_fit_out* out);
int pp_fit_poll(pp_ctx* ctx);
int pp_fit_wait(pp_ctx* ctx);

/* Stream-ordered batches (one context, one stream, no extra thread).  pp_fit_enqueue copies the two
 * argument blocks and queues the WHOLE batch on the context's stream -- small inputs, every kernel,
 * the outputs on their way to a pinned staging block -- and returns without waiting; pp_fit_collect
 * completes the OLDEST enqueued batch (waits for it, fills the caller's output arrays) and returns what
 * pp_fit_portrait_batch would have returned.  Up to THREE batches may be pending (each has its own
 * staging blocks and its own set of the device work buffers its solve and post-fit stage use), so a
 * caller that enqueues batches k + 1, k + 2 before it collects batch k keeps the GPU busy while the host
 * marshals.  One-pass fits of 2048-bin portraits leave their solve and post-fit stage to the transform of
 * the NEXT enqueued batch (option "fuse_tail", default on): batch k is then complete one transform later,
 * or when pp_fit_collect finds it the youngest and queues them itself.  Same results either way, to the
 * bit, as pp_fit_portrait_batch.  Batches whose flow needs a host decision in its middle (scattering fits,
 * device seeds, sub-batching) simply run to their end inside pp_fit_enqueue; the one-pass flow, with
 * the caller's guesses or with the reference's own (pp_seed_ref; phase / DM / GM fits), is deferred whole; a one-pass
 * batch in which some subint fails its certificate (poor guesses) is fitted again by the general
 * flow inside pp_fit_collect.  Every buffer the argument blocks point to (pp_seed_ref included) must
 * stay valid and untouched until the batch has been collected; no other fit call may be made on the
 * context while batches are pending (PP_ESTATE).  pp_fit_pending returns how many are.
 * The reference has no counterpart: its loop over subints is serial (pptoas.py:344-489). */
int pp_fit_enqueue(pp_ctx* ctx, const pp_fit_in* in, pp_fit_out* out);
int pp_fit_collect(pp_ctx* ctx);
int pp_fit_pending(pp_ctx* ctx);

/* ---- building blocks exported for parity tests --------------------------- */
/* rFFT of nrows real rows of length nbin (host pointers); out holds
 * nrows*(nbin/2+1) interleaved (re,im) doubles.  numpy.fft.rfft of
 * pptoaslib.py:976-978. */
int pp_rfft_rows(pp_ctx* ctx, const void* rows, int dtype, int nrows, int nbin,
                 double* out);

/* 1-D FFTFIT of nprof (data, model) profile pairs: 7 doubles per pair
 * (phase, phase_err, scale, scale_err, snr, red_chi2, duration).
 * fit_phase_shift (pplib.py:2054-2100).  noise[i] < 0 or NaN = measure it. */
int pp_fit_phase_shift_batch(pp_ctx* ctx, const double* data,
                             const double* model, const double* noise,
                             int nprof, int nbin, double lo, double hi, int Ns,
                             double* out7);

/* Narrowband scattering fit of nprof (data, model) profile pairs: a phase and a scattering time each,
 * fitted jointly.  The reference planned it as fit_phase_shift_scat (pptoas.py:988-991) and never wrote
 * it; it is fit_portrait_full (pptoaslib.py:928-1096) on a one-channel portrait with fit_flags
 * [1,0,0,1,0].  With B_k = 1 / (1 + 2 pi i k tau), tau in rotations, over the harmonics k = 1 .. nbin/2:
 *   C = Re sum_k d_k conj(m_k) conj(B_k) e^{2 pi i k phi} / sigma_F^2,  S = sum_k |B_k|^2 |m_k|^2 / sigma_F^2,
 *   f = -C^2 / S is minimised over (phi, tau) or, with log10_tau != 0, over (phi, log10 tau).
 * guess [nprof][2]: phi (NaN = an Ns-point grid over [lo, hi] at the guessed tau, fit_phase_shift against
 * the scattered model) and tau or log10 tau.  noise [nprof] or null: time-domain sigma, NaN / < 0 =
 * measured from the top quarter of the power spectrum.  Any even nbin from 8 to 4096.
 * out [nprof][PP_NBS_NOUT]:
 *   0 phi [rot, in [-0.5, 0.5)]   1 phi_err     2 tau or log10 tau [rot]   3 its error
 *   4 scale                       5 scale_err   6 snr = scale sqrt(S)      7 red_chi2 = (Sd + f) / (nbin - 3)
 *   8 covariance of (phi, tau)    9 nfeval      10 return_code (PP_RC_*)
 * The errors and the covariance come from the Hessian that includes the amplitude
 * (fit_portrait_full_function_2deriv_with_scales).  return_code: PP_RC_STALL converged to rounding;
 * PP_RC_MAXITER 64 evaluations spent; PP_RC_NAN for NaN / Inf input, an all-zero data or model row, a
 * Hessian that is not positive definite, a linear tau more than 3 tau_err below zero, or a fitted S/N
 * below 6 (no detection: the tail would be fitted to the noise) -- phi, tau, their errors and the
 * covariance are NaN then.  PP_RC_NAN also marks a numerically singular (phi, tau) Hessian, which is what
 * unscattered data give (at tau = 0 a scattering time and a delay are the same thing to second order in
 * chi^2): the covariance is NaN, the error of tau is +infinity, and phi, phi_err, scale_err are the values
 * at that fixed tau -- fit_phase_shift's.  A pair's outputs depend on that pair alone, bit for bit. */
#define PP_NBS_NOUT 11
int pp_fit_phase_tau_batch(pp_ctx* ctx, const double* data, const double* model, const double* noise,
                           const double* guess, int nprof, int nbin, double lo, double hi, int Ns,
                           int log10_tau, double* out);

/* The reference's initial phase guess of nsub subints (pptoas.py:421-457), data side
 * fused into one read of the portraits:
 *   rot_prof_i = np.average(rotate_data(port_i, phi_i, DM_i, P_i, freqs_i, nu_DM),
 *                           axis=0, weights=weights_i)      (par3 = phi, DM, GM per subint)
 *   out7[i]    = fit_phase_shift(rot_prof_i, model_profs_i, Ns=Ns, bounds=(lo, hi))
 * with the finish selected by option "fps_finish".  Channels of zero weight are not
 * read.  weights [nsub][nchan] and model_profs [nsub][nbin] are host arrays; `src` is
 * a host or device pointer (`on_device`), dtype PP_F64 / PP_F32. */
int pp_reference_phase_seed(pp_ctx* ctx, const void* src, int dtype, int on_device,
                            int nsub, int nchan, int nbin, const double* freqs,
                            int64_t freqs_stride, const double* P, const double* par3,
                            double nu_DM, double nu_GM, const double* weights,
                            const double* model_profs, double lo, double hi, int Ns,
                            double* out7);

/* Fourier rotation / (de)dispersion of portraits: dst[i][n] = irfft(rfft(src[i][n])
 * e^{2 pi i k phi_in}), phi_in = par[i][0] + Dconst par[i][1] (nu_n^-2 - nu_DM^-2)/P_i
 * + Dconst^2 par[i][2] (nu_n^-4 - nu_GM^-4)/P_i.  rotate_data (pplib.py:2338-2426),
 * rotate_portrait (:2428-2460), rotate_portrait_full (pptoaslib.py:52-81).
 * src/dst: [nsub][nchan][nbin] of `dtype`, both host or both device pointers
 * (dst may equal src on the device); nu_DM / nu_GM may be INFINITY. */
int pp_rotate_portraits(pp_ctx* ctx, const void* src, void* dst, int dtype,
                        int on_device, int nsub, int nchan, int nbin,
                        const double* freqs, int64_t freqs_stride, const double* P,
                        const double* par3, double nu_DM, double nu_GM);

/* ---- synthetic portraits generated on the device ------------------------- */
/* ppalign's accumulation (ppalign.py:199-206): aligned[n][:] = sum_i w[i][n] *
 * rotate_data(src[i][n], phase_i, DM_i, P_i, freqs, nu_ref_i) and total_weights[n] =
 * sum_i w[i][n]; rows with w = 0 (or NaN) are skipped.  par3[i] = {phase, DM, nu_ref}
 * (nu_ref may be INFINITY).  src: [nsub][nchan][nbin] of `dtype`, host or device;
 * aligned [nchan][nbin] and total_weights [nchan] are host arrays, overwritten. */
int pp_align_accumulate(pp_ctx* ctx, const void* src, int dtype, int on_device,
                        int nsub, int nchan, int nbin, const double* freqs,
                        int64_t freqs_stride, const double* P, const double* par3,
                        const double* weights, double* aligned, double* total_weights);

/* ---- ppalign: an accumulator that stays on the device between calls --------- */
/* align_archives' sum over archives and subints (ppalign.py:116-117, :202-212): the context keeps
 * aligned_port as packed half-spectra [npol][nchan_model][nbin/2] and total_weights [nchan_model].
 * pp_align_begin allocates (or reuses) and zeroes them; a second begin starts over. */
int pp_align_begin(pp_ctx* ctx, int npol, int nchan_model, int nbin);

/* ppalign.py:202-208 for every subint of src[nsub][npol][nchan][nbin] (`dtype`, host or device):
 *   aligned_port[ipol, chan_map[i][n]] += weights[i][n] * rotate_data(src[i][ipol][n], phase_i,
 *                                          DM_i, P_i, freqs, nu_ref_i)       for every ipol
 *   total_weights[chan_map[i][n]]      += weights[i][n]                      once
 * par3[i] = {phase, DM, nu_ref} (nu_ref may be INFINITY).  weights [nsub][nchan] (host): 0 or NaN
 * skips the row, a negative weight counts.  chan_map [nsub][nchan] (host) names the accumulator row
 * of every data channel -- the reference's model_ichans (:161-172); several channels may share a row
 * and a row may get nothing; NULL is the identity and needs nchan == nchan_model.  A row's
 * contributions are added in the order (subint, data channel) by the one workgroup that owns the
 * row: the accumulator's bits depend on the sequence of rows only, not on how the subints are cut
 * into calls.  PP_EINVAL before pp_align_begin, for npol / nbin other than begin's, and for a
 * chan_map entry outside [0, nchan_model) -- checked on the host before anything is launched. */
int pp_align_add(pp_ctx* ctx, const void* src, int dtype, int on_device, int nsub, int npol,
                 int nchan, int nbin, const double* freqs, int64_t freqs_stride,
                 const double* P, const double* par3, const double* weights,
                 const int32_t* chan_map);

/* The contribution lists pp_align_add builds from weights and chan_map, for inspection (host only, no context):
 * off[nchan_model + 1] and pairs[2 x live rows] = (subint, data channel) of accumulator row m at off[m] .. off[m+1],
 * by subint, then data channel; rows of weight 0 or NaN are left out.  pairs must hold 2 nsub nchan ints.  Returns
 * the number of pairs, or PP_EINVAL (a chan_map entry outside [0, nchan_model), or no map with nchan != nchan_model). */
int pp_align_lists(int nsub, int nchan, int nchan_model, const double* weights,
                   const int32_t* chan_map, int32_t* off, int32_t* pairs);

/* ppalign.py:210-212 and :220-226: rows of positive total weight divided by it, the overall
 * rotation rotate_data(aligned_port, rot_phase) applied in the spectrum (0: the rows are not
 * touched), ONE inverse transform per row; aligned [npol][nchan_model][nbin] and total_weights
 * [nchan_model] are host arrays, overwritten.  to_slot >= 0 also installs polarisation 0 as the
 * template of that model slot from the device copy (the next iteration's model_port, :213) --
 * the same bits as pp_model_set of `aligned`.  The accumulator stays valid: finish may be called
 * again with another rot_phase, and pp_align_add may go on. */
int pp_align_finish(pp_ctx* ctx, double rot_phase, double* aligned, double* total_weights,
                    int to_slot);

/* Per-channel reduced chi^2 of fitted subints in the time domain, as
 * get_channels_to_zap forms it (pptoas.py:1239-1245 via show_fit :1394-1404 and
 * get_red_chi2 pplib.py:727-750): sum over bins of (data rotated by the fitted
 * phi, DM, GM  -  scales[n] x template, scattered by tau, alpha when tau != 0)^2
 * / errs[n]^2 / (nbin - 2).  params5[i] = {phi, DM, GM, tau [rot, linear], alpha}
 * at nu_refs3[i]; the template is the model slot of each subint (null: slot 0);
 * red_chi2: [nsub][nchan] host array. */
int pp_channel_red_chi2(pp_ctx* ctx, const void* src, int dtype, int on_device,
                        int nsub, int nchan, int nbin, const int32_t* model_slot,
                        const double* freqs, int64_t freqs_stride, const double* P,
                        const double* params5, const double* nu_refs3,
                        const double* scales, const double* errs, double* red_chi2);

/* The fit's residual portrait: what GetTOAs.show_fit(..., return_fit=True) returns
 * (pptoas.py:1317-1419) and their difference.  With phi_in and tau_in as for
 * pp_channel_red_chi2, B_k = 1 / (1 + 2 pi i k tau_in), d = rfft(src[i][n]), m the
 * template of the subint's model slot (null: slot 0) and a = scales[i][n]:
 *   frame 0 ("model"): D_k = d_k e^{2 pi i k phi_in},  Mo_k = a B_k m_k
 *   frame 1 ("data"):  D_k = d_k,                      Mo_k = a B_k m_k e^{-2 pi i k phi_in}
 * (DC is not rotated; the Nyquist harmonic keeps its real part, as irfft does) and
 *   port = irfft(D), model = irfft(Mo), resid = irfft(D - Mo)   [nsub][nchan][nbin] of `dtype`
 *   red_chi2[nsub][nchan] = sum_bins resid^2 / errs^2 / (nbin - 2), by Parseval, the same
 *   figure in both frames and bit for bit pp_channel_red_chi2's.
 * Every output may be null (not formed, not stored), at least one must be given; errs may be
 * null unless red_chi2 is asked for.  mask[nsub][nchan] (host, may be null): rows of weight 0
 * or NaN are not read, their port / model / resid rows are zeros and their red_chi2 NaN.
 * Host input gives host outputs; a device input (`on_device`) gives device outputs, red_chi2
 * included, with no copy to the host.  The per-subint arrays are host arrays either way. */
int pp_fit_residuals(pp_ctx* ctx, const void* src, int dtype, int on_device, int nsub,
                     int nchan, int nbin, const int32_t* model_slot, const double* freqs,
                     int64_t freqs_stride, const double* P, const double* params5,
                     const double* nu_refs3, const double* scales, const double* errs,
                     const double* mask, int frame, void* port, void* model, void* resid,
                     double* red_chi2);

/* ---- ppzap ---------------------------------------------------------------- */
/* The channel noise of ppzap's noise method (ppzap.py:200-241): for every row of src
 * [nrows][nbin] (`dtype`, host or device) the norm of normalize_portrait (pplib.py:2462-2507)
 * by `norm_method` (PP_NORM_*; PP_NORM_PROF takes divisor[nrows], the fit_phase_shift scale
 * of each row against its subint's mean profile) and get_noise_PS(row / norm, frac=4)
 * (pplib.py:2227-2253), formed as noise(row) / |norm|.  Rows with no non-zero sample keep
 * norm 1 and noise 0.  norms and noise: [nrows] host arrays.  nbin: even, 8 ... 4096. */
int pp_channel_noise(pp_ctx* ctx, const void* src, int dtype, int on_device, int nrows,
                     int nbin, int norm_method, const double* divisor, double* norms,
                     double* noise);

/* get_zap_channels (ppzap.py:18-47) of nsub subints at once: over the channels with
 * good[i][n] != 0, drop every channel whose noise exceeds median + nstd * std (NumPy's
 * median and population std) and repeat until a round drops none or none is left.
 * noise, good, zap: [nsub][nchan] host arrays (nchan <= 4096); zap[i][n] = 1 for every
 * dropped channel, 0 elsewhere. */
int pp_zap_median(pp_ctx* ctx, const double* noise, const unsigned char* good, int nsub,
                  int nchan, double nstd, unsigned char* zap);

/* ---- ppspline --------------------------------------------------------------- */
/* pplib.get_SNR(row, fudge) (pplib.py:2289-2308) of every row of src [nrows][nbin] (`dtype`, host or
 * device): sum / (noise sqrt(Weq)) / fudge with Weq = sum / max (1, and a zero result, where that is not
 * positive) and the get_noise_PS noise of pp_channel_noise; sum, maximum and noise come from one pass over
 * the row.  snrs: [nrows] host array. */
int pp_channel_snrs(pp_ctx* ctx, const void* src, int dtype, int on_device, int nrows,
                    int nbin, double fudge, double* snrs);

/* ---- the 'fit' noise method -------------------------------------------------- */
/* pplib.get_noise_fit(row, fact) (pplib.py:2255-2287) of every row of src [nrows][nbin] (`dtype`, host or
 * device), with pplib.find_kc(pows, fn=fn) (pplib.py:1465-1495) inside it: pows = |rfft(row)|^2 / nbin, the
 * 20 x 20 x 20 opt.brute grid over (a, b, dc) of b f_a(k) + dc against log10(pows) in closed form, NumPy's
 * argmin (a slowest, dc fastest, the first minimum), kc of the winning a, then sqrt(mean(pows[int(k):])) with
 * k = fact kc, clipped to int(0.99 H) from H = nbin / 2 + 1 on.  A row with a harmonic of exactly zero power
 * (log10 = -inf: the reference's grid is all NaN) takes cell 0 and kc = H - 1; an all-zero row has noise 0.
 * input_kind PP_NOISEFIT_POWS: src holds H f64 powers per row, find_kc's own input (PP_F64, PP_NORM_NONE).
 * norm_method, divisor, norms, noise: as pp_channel_noise, noise(row) / |norm| (PP_NORM_RMS: the fitted noise);
 * scaling a row shifts log10(pows) and the grid alike, so the cell does not move.  kc: int32 [nrows] or NULL;
 * cell: int32 [nrows][3] = (ia, ib, idc) or NULL.  A row's bits do not depend on the rest of the call.
 * nbin: even, 8 ... 4096; fact >= 0. */
int pp_channel_noise_fit(pp_ctx* ctx, const void* src, int dtype, int on_device, int nrows, int nbin,
                         int input_kind, int fn, double fact, int norm_method, const double* divisor,
                         double* norms, double* noise, int32_t* kc, int32_t* cell);

/* pplib.get_SNR(row, fudge) (pplib.py:2289-2308) of every row with get_noise(row, method='fit')
 * (pplib.py:2221-2222) as its noise: pp_channel_snrs with pp_channel_noise_fit's estimator, one pass. */
int pp_channel_snrs_fit(pp_ctx* ctx, const void* src, int dtype, int on_device, int nrows, int nbin,
                        int fn, double fact, double fudge, double* snrs);

/* find_kc's width axis for H harmonics (host only, no context): the 20 values np.mgrid[lo:hi:20j] gives
 * opt.brute (pplib.py:1476-1485; i * ((hi - lo) / 19) + lo, (lo, hi) = (1 / H, 1) for PP_KC_EXP_DC and (1, H)
 * for PP_KC_HALF_TRI) and the kc find_kc returns for each (pplib.py:1487-1493): the smallest k < H with
 * exp(-a k) < 0.005, H - 1 where there is none; floor(a) for the half triangle. */
int pp_noise_fit_grid(int H, int fn, double* a20, int32_t* kc20);

/* The device side of pplib.pca (pplib.py:1497-1534) up to the eigen-solve, for the portrait src
 * [nchan][nbin] (`dtype`, host or device) and the weights w[nchan] (host; sumw = sum w, fact = sumw -
 * sum w^2 / sumw, np.cov's normalisation with aweights and ddof = 1):
 *   mean_prof = sum_n w_n src_n / sumw                                      (ppspline.py:70)
 *   delta = src - mean_prof, re-centred by its weighted average as np.cov does (pplib.py:1528)
 *   gram  = the nbin x nbin covariance when nchan >= nbin, else the nchan x nchan dual
 *           sqrt(w_i) sqrt(w_j) delta_i . delta_j / fact, which has the covariance's non-zero spectrum
 * on v_mfma_f64_16x16x4_f64 in a fixed summation order (the same bits on every run).  mean_prof [nbin] and
 * gram [n][n], n = min-side as above, are host arrays.  The centred rows stay resident for pp_pca_basis
 * and pp_pca_project.  nbin: even, 8 ... 4096. */
int pp_pca_gram(pp_ctx* ctx, const void* src, int dtype, int on_device, int nchan, int nbin,
                const double* w, double sumw, double fact, double* mean_prof, double* gram);

/* The leading eigenvectors of the covariance and what find_significant_eigvec (pplib.py:1555-1619) measures
 * of them without smoothing.  vecs [nvec][n] are the host's leading eigenvectors of gram (one per row,
 * eigenvalues lam[nvec], descending; nvec <= 16); on the dual side each is mapped back to a profile,
 * delta^T sqrt(w) u / sqrt(lam fact), scaled to unit length.  basis [nvec][nbin]; stats [nvec][4] = { sum_{k>=1} |rfft(ev)_k|^2,
 * get_noise_PS(ev) (pplib.py:2249-2253), max |ev|, count_crossings(|ev|, 0.1 max |ev|) (pplib.py:686-694) }.
 * The basis stays resident. */
int pp_pca_basis(pp_ctx* ctx, const double* vecs, const double* lam, int nvec, double* basis,
                 double* stats);

/* proj [nchan][ncomp] = delta . basis[ieig] and reconst [nchan][nbin] = proj . basis[ieig]^T + mean_prof
 * (ppspline.py:119-129; reconstruct_portrait, pplib.py:1536-1553) from the resident rows and basis. */
int pp_pca_project(pp_ctx* ctx, const int32_t* ieig, int ncomp, double* proj, double* reconst);

/* ---- wavelet smoothing (ppspline's smoothed templates) ----------------------- */
/* wavelet_smooth (pplib.py:1621-1666) of rows[nrows][nbin] (`dtype`, host or device) with the db8 wavelet: the
 * stationary wavelet transform with periodic boundary to nlevel levels, the threshold
 *   lopt = fact * median(|cA_L u cD_L|) / 0.6745 * sqrt(2 ln nbin)
 * applied to the coarsest approximation and every level's details (threshtype 0: hard, 0 where |c| < lopt;
 * 1: soft, c max(1 - lopt / |c|, 0)), and the inverse transform.  filt[16]: the orthonormal low-pass taps in
 * PyWavelets' rec_lo order (checked: sum sqrt 2, orthonormal to 1e-12).  nlevel and fact are host arrays read with
 * their strides: 0 = one value for every row, 1 = one per row; 2^nlevel must divide nbin.  out[nrows][nbin] is f64,
 * on the device when the rows are.  nbin: even, 16 ... 4096.  Every row's result depends on that row alone. */
int pp_wavelet_smooth(pp_ctx* ctx, const void* rows, int dtype, int on_device, int nrows, int nbin,
                      const double* filt, int threshtype, const int32_t* nlevel, int64_t nlevel_stride,
                      const double* fact, int64_t fact_stride, void* out);

/* smart_smooth (pplib.py:1668-1735) of the same rows: for every level 1 ... try_nlevels, scipy.optimize.brute of
 * fit_wavelet_smooth_function (:1737-1761) over 30 factors in [0, 3] with its Nelder-Mead finish; the level of the
 * smallest value; the final smooth, zeroed when its reduced chi^2 against the row is further than rchi2_tol from 1.
 * A row of zeros stays zero (level 0).  Host arrays: info5[nrows][5] = { level, fact, -fun, reduced chi^2 of the
 * final smooth, objective evaluations }, stats4[nrows][4] = pp_pca_basis's statistics of the smoothed row,
 * raw_noise[nrows] (or NULL) = get_noise_PS of the row itself, find_significant_eigvec's noise. */
int pp_smart_smooth(pp_ctx* ctx, const void* rows, int dtype, int on_device, int nrows, int nbin,
                    const double* filt, int threshtype, int try_nlevels, double rchi2_tol, void* out,
                    double* info5, double* stats4, double* raw_noise);

/* ---- ppgauss --------------------------------------------------------------- */
/* The device side of fit_gaussian_portrait (pplib.py:1924-2052), a Levenberg-Marquardt fit whose Jacobian is taken by
 * forward differences: every column is a whole model portrait (gen_gaussian_portrait, pplib.py:853-930).
 * pp_gauss_fit_begin makes the data portrait data[nchan][nbin] (`dtype`, host or device; the caller hands over the
 * good channels only), its channel frequencies freqs[nchan] and 1 / errs[n] (errs[nchan] > 0, the noise level of every
 * channel; host arrays) resident for the whole fit: no later call uploads the portrait again.  A second begin starts
 * over; pp_gauss_fit_end releases everything the fit holds.  nbin: even, 8 ... 4096, or a power of two up to 8192. */
int pp_gauss_fit_begin(pp_ctx* ctx, const void* data, int dtype, int on_device, int nchan,
                       int nbin, const double* freqs, const double* errs);
int pp_gauss_fit_end(pp_ctx* ctx);

/* A joined fit (gen_gaussian_portrait's join_ichans, pplib.py:923-929): one model fitted to njoin bands at once, every
 * band with a phase offset and a Delta-DM of its own.  band_of_chan[nchan] (host) names the band of every resident
 * channel, 0 .. njoin - 1, or -1 for a channel in none; P [s] turns the Delta-DMs into rotations.  Valid only while a
 * fit is open; the map stays resident until pp_gauss_fit_begin or pp_gauss_fit_end clears it.  Refused: no open fit
 * (PP_ESTATE); njoin outside 1..16, an index outside [-1, njoin), P not positive and finite (PP_EINVAL). */
int pp_gauss_fit_join(pp_ctx* ctx, int njoin, const int* band_of_chan, double P);

/* The weighted residual rows of nsets parameter vectors at once (fit_gaussian_portrait_function, pplib.py:1230-1242):
 *   R[s][n][:] = (data_n - model_n(dc[s], tau_rot[s], alpha[s], comps[s])) / errs[n]
 * with model = gen_gaussian_portrait of model code `code` ("000" ... "111") about nu_ref; tau_rot[s] is the scattering
 * time at nu_ref in rotations (0: unscattered), alpha[s] the scattering index, comps[s][ngauss][6] = loc, m_loc, wid,
 * m_wid, amp, m_amp.  One workgroup per (channel, set); the model rows are formed by the code of
 * pp_gaussian_portrait, operation for operation.  R stays on the device for pp_gauss_normal; out_or_null
 * [nsets][nchan][nbin] (host) receives a copy.  Refused, never truncated: ngauss > 16, nsets > 100, nsets nchan nbin 8
 * bytes above 2 GiB (PP_EINVAL); no resident portrait (PP_ESTATE).
 * join_or_null [nsets][njoin][2] = (phase [rot], Delta-DM [cm^-3 pc]) of every set and band of a joined fit: the model
 * row of channel n in band j is rotated by phi_n = phase_sj + Dconst DM_sj (nu_n^-2 - nu_ref^-2) / P after it has been
 * scattered (rotate_data's sign: positive to earlier phase), within the row's one pass through its harmonics; a row
 * with phi_n == 0 is computed exactly as without a join.  NULL with a resident band map means all zeros; a pointer
 * without one is refused (PP_ESTATE). */
int pp_gauss_residuals(pp_ctx* ctx, const char* code, double nu_ref, int nsets, const double* dc,
                       const double* tau_rot, const double* alpha, int ngauss,
                       const double* comps, double* out_or_null, const double* join_or_null);

/* Normal equations of a forward-difference Levenberg-Marquardt step from nsets residual rows of nrow samples: with
 * D_a = (R_{a+1} - R_0) / h[a], a = 0 .. nsets - 2,
 *   *chi2 = sum R_0^2,   g[a] = sum D_a R_0,   G[a][b] = sum D_a D_b          (over all nrow samples)
 * R_or_null == NULL takes the rows the last pp_gauss_residuals left (nsets and nrow = nchan nbin must be its; else
 * PP_ESTATE); a pointer (host, or device with on_device) hands in R[nsets][nrow] -- host rows take the resident rows'
 * place.  With nsets == 1 only chi2 is written (h, g, G may be NULL).  f64 throughout, a two-stage slab sum without
 * floating-point atomics: stage one writes the partial sums of runs of samples whose length depends on nrow alone,
 * stage two adds them in run order, so the same call gives the same bits on every run and every device.  Every
 * product and every sum is rounded on its own: an entry's error is below nrow 2^-53 sum |terms|. */
int pp_gauss_normal(pp_ctx* ctx, const double* R_or_null, int on_device, int nsets, int nrow,
                    const double* h, double* chi2, double* g, double* G);

/* Fill dst[nsub][nchan][nbin] (device pointer, dtype) with
 *   gains[i][n] * rotate(model slot, -phi_i, -DM_i, -GM_i) + N(0, sigma)
 * using a counter-based RNG keyed on (seed, first_subint + i, channel, bin).
 * inj is host [nsub][3] (phi, DM, GM injected, reference frequency infinity); gains is host
 * [nsub][nchan] -- per-channel amplitudes, e.g. the scintillation pattern of add_scintillation
 * (pplib.py:1146-1174) -- or NULL (= 1 everywhere).  The synthetic inputs of SURVEY 8(d). */
int pp_synth_portraits(pp_ctx* ctx, int slot, void* dst, int dtype, int nsub,
                       const double* freqs, const double* P, const double* inj,
                       const double* gains, double sigma, uint64_t seed, int64_t first_subint);

/* Simulated observations (make_fake_pulsar, pplib.py:3183-3378): fill dst[nsub][npol][nchan][nbin] (device pointer,
 * dtype; nchan and nbin are the model slot's) with
 *   amps[i][p][n] * irfft_k(m[n][k] e^{-2 pi i k delays[i][n]}) + sigmas[n] * z(seed, first_subint + i, p, n, bin)
 * m being the slot's spectrum and z unit normal deviates of a counter-based RNG.  delays is host [nsub][nchan] in
 * rotations, positive = later -- any delay law the caller can write down (dispersion about a centre frequency, the
 * DM(nu) power laws of add_DM_nu, ...); amps is host [nsub][npol][nchan] (scales times the scintillation pattern of
 * add_scintillation, pplib.py:1146-1174) or NULL (= 1); sigmas is host [nchan] or NULL (= 0).  The model is the same
 * in every polarisation: a row's inverse transform is taken once and its npol copies differ in amplitude and noise.
 * Values are formed in f64 and cast on the store: the f32 output is the rounded f64 output.  sigmas[n] == 0 gives the
 * noise-free row exactly and amps == 0 gives sigmas z exactly.  A subint's bits depend on (seed, first_subint + i) and
 * its own arguments only, not on nsub or on how a long observation is cut into calls.  Refused: an unset slot
 * (PP_ESTATE); nsub or npol < 1, npol > 65536, a delay that is not finite, a sigma that is negative, NaN or infinite
 * (PP_EINVAL) -- checked on the host before anything is launched. */
int pp_fake_portraits(pp_ctx* ctx, int slot, void* dst, int dtype, int nsub, int npol,
                      const double* delays, const double* amps, const double* sigmas,
                      uint64_t seed, int64_t first_subint);

/* ---- time, frequency and polarisation scrunching ---------------------------- */
#define PP_POL_KEEP  0   /* every polarisation is kept */
#define PP_POL_SUM01 1   /* Coherence -> Intensity: src[s][0] + src[s][1], one output polarisation */
#define PP_POL_FIRST 2   /* Stokes -> Intensity: polarisation 0 only; the others are not read */

/* What load_data hands to PSRCHIVE -- tscrunch, fscrunch, pscrunch (pplib.py:2650-2814, the calls at :2692, :2709 and :2713) -- as
 * one pass over src[nsub][npol][nchan][nbin] (`dtype`, host or device):
 *   dst [gt][p'][gf][b] = sum_{s in T_gt} sum_{c in F_gf} weights[s][c] * src[s][p][c][b]  /  wout[gt][gf]
 *   wout[gt][gf]        = sum_{s in T_gt} sum_{c in F_gf} weights[s][c]
 * The groups are contiguous runs given by offsets: T_gt = [t_off[gt], t_off[gt+1]) over subints, F_gf = [f_off[gf],
 * f_off[gf+1]) over channels; t_off[ngt+1] and f_off[ngf+1] ascend strictly from 0 to nsub / nchan.  Singleton
 * groups leave an axis alone.  pol_mode is one of PP_POL_*; p' = p for PP_POL_KEEP, otherwise there is one output
 * polarisation.  weights [nsub][nchan] (host): a row of weight 0 or NaN is skipped and its samples are not read (a
 * zapped channel may hold anything), a negative weight counts; a cell whose total weight is not positive is all
 * zeros and has wout = 0.  Of a host input only the polarisations the mode reads are copied to the device.
 * dst [ngt][npol'][ngf][nbin] is f64, on the host or the device like src; wout [ngt][ngf]
 * is a host array.
 * The order of summation is part of the interface: every output element is the f64 sum of its members in ascending
 * (s, c) order -- fma(w, x, sum), for PP_POL_SUM01 fma(w, x0 + x1, sum) -- divided once at the end.  Its bits do not
 * depend on the launch, on how a host input is cut into runs (option max_work_bytes: a time group that straddles
 * two runs carries its partial sums on the device), on whether src was on the device or on the other groups of the
 * call.  No atomics.
 * PP_EINVAL -- checked on the host before anything is launched -- for null pointers, offsets that are not as above,
 * PP_POL_SUM01 with fewer than two polarisations, an unknown pol_mode or dtype, and nbin that is not even in
 * [8, 4096] or a power of two. */
int pp_scrunch(pp_ctx* ctx, const void* src, int dtype, int on_device, int nsub, int npol, int nchan,
               int nbin, const double* weights, int ngt, const int32_t* t_off, int ngf,
               const int32_t* f_off, int pol_mode, double* dst, double* wout);

/* ---- measurement --------------------------------------------------------- */
/* Accumulated HIP-event time per kernel family since the last reset (only
 * while option "profile" = 1): names[i] points to a static string.
 * Returns the number of families written (<= cap). */
int pp_kernel_times(pp_ctx* ctx, int cap, const char** names, double* seconds,
                    int64_t* launches);
int pp_kernel_times_reset(pp_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PP_TOAS_H */
