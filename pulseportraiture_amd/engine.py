"""Thin Python wrapper of the C ABI: one Engine = one device context.

The batch entry point `Engine.fit_batch` is what reaches 10^4 fits/s; the
reference-shaped single-subint functions in pptoaslib.py / pplib.py marshal
into it.
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from ._lib import (FitIn, FitOut, PP_ENOTSUP, PP_F32, PP_F64, PP_METHOD_NEWTON, PP_METHOD_TRUST_NCG,
                   SeedRef, c_double_p, c_int32_p, c_uint8_p)

# the reference's minimiser names (pptoaslib.py:993-1010) -> device solver
METHODS = {'trust-ncg': PP_METHOD_TRUST_NCG, 'Newton-CG': PP_METHOD_NEWTON,
           'TNC': PP_METHOD_NEWTON, 'newton': PP_METHOD_NEWTON}


class EngineError(RuntimeError):
    pass


class EngineNotSupported(EngineError):
    """The library has no device path for this request in this shape (PP_ENOTSUP): nothing
    was done; the caller takes its general route."""


def _check(rc, what):
    if rc == PP_ENOTSUP:
        raise EngineNotSupported("%s: %s" % (what, _lib.last_error()))
    if rc != 0:
        raise EngineError("%s failed (%d): %s" % (what, rc, _lib.last_error()))


def _is_device_array(x):
    """A device-resident array (torch tensor).  The engine launches on its OWN HIP
    stream, the array's contents were produced on the caller's (torch's current
    stream, asynchronously): wait for the producer before the engine may touch it --
    otherwise a kernel of ours can read a tensor whose `clone()` / `to()` / fill has
    not finished (seen as rare, run-dependent garbage in a few rows).  The engine's
    calls end with a synchronise of its own stream, so the other direction is safe."""
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda):
        _wait_for_producer(x)
        return True
    return False


# Devices whose producer stream the engine call running on THIS thread has already waited for.
# Per thread: engines are one per host thread, and a set shared between threads would let one
# thread's call clear -- or pre-fill -- the record of another's while that one sits in
# synchronize() with the GIL released.
_TLS = threading.local()


def _new_call():
    """Start of an engine call: every device array handed over was produced before it, so
    one wait per device and call covers them all (seven waits per fit cost ~50 us)."""
    _TLS.waited = set()


def _wait_for_producer(x):
    waited = getattr(_TLS, "waited", None)
    if waited is None:
        waited = _TLS.waited = set()
    key = str(x.device)
    if key in waited:
        return
    try:
        import torch
        torch.cuda.current_stream(x.device).synchronize()
    except ImportError:      # (another array library: its arrays must be complete when handed over)
        pass
    waited.add(key)


def _array_arg(x, what):
    """(pointer, dtype code, on_device, shape, keep-alive) of an array argument: NumPy (anything
    that is not f32 is converted to f64, and made contiguous) or a device tensor, f64 or f32.  A
    device tensor must be contiguous -- the library reads (rotate_portraits: writes) it as dense
    memory, so a strided view is refused: "<what> must be contiguous"."""
    if _is_device_array(x):
        if not x.is_contiguous():
            raise EngineError("%s must be contiguous" % what)
        return (C.c_void_p(x.data_ptr()), PP_F64 if x.element_size() == 8 else PP_F32, 1,
                tuple(int(v) for v in x.shape), x)
    a = np.asarray(x)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    a = np.ascontiguousarray(a)
    return C.c_void_p(a.ctypes.data), PP_F64 if a.dtype == np.float64 else PP_F32, 0, a.shape, a


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


NOISE_METHODS = _lib.NOISE_METHODS
_RESID_OUTPUTS = ("port", "model", "resid", "red_chi2")     # what fit_residuals can return
_RESID_FRAMES = {"model": 0, "data": 1}


def _noise_method(method, fn='exp_dc'):
    if method not in NOISE_METHODS:
        raise ValueError("noise method must be 'PS' or 'fit', not %r" % (method,))
    if fn not in _lib.PP_KC_FNS:
        raise ValueError("fn must be 'exp_dc' or 'half_tri', not %r" % (fn,))


def _f64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = np.ascontiguousarray(np.broadcast_to(a, shape))
    return a


def _nu_array(nus, nsub):
    """[nsub,3] float64 reference frequencies; None entries become NaN (= let
    the engine choose: mean frequency for the fit, zero-covariance for output)."""
    if nus is None:
        return np.full((nsub, 3), np.nan)
    a = np.asarray(nus)
    if a.dtype == object:
        a = np.where(np.equal(a, None), np.nan, a).astype(np.float64)
    return np.ascontiguousarray(np.broadcast_to(a.astype(np.float64, copy=False),
                                                (nsub, 3)))


class _Batch(object):
    """One prepared fit: the result dict, the two argument blocks, and everything those point
    to.  Whoever holds it keeps all of that alive -- until the synchronous call returns, or
    until collect() / wait() has returned for an enqueued / submitted batch."""

    def __init__(self, res, fin, fout, keep):
        self.res, self.fin, self.fout, self.keep = res, fin, fout, keep

    def finish(self):
        """The result dict of the completed batch (`duration` becomes a Python float)."""
        self.res["duration"] = float(self.res["duration"][0])
        return self.res


class Engine(object):
    """Device context + scratch; not thread-safe (one per host thread and GPU)."""

    def __init__(self, device=0):
        self._ctx = None
        self._digests = {}      # slot -> content digest of the resident template
        self._queue = []        # enqueued batches (_Batch), oldest first, until collect()
        self._pending = None    # the submitted batch (_Batch) until wait()
        self._pca_shape = None  # (nchan, nbin) of the centred portrait pca_gram left on the device
        self._align_shape = None  # (npol, nchan_model, nbin) of the resident accumulator (align_begin)
        self._gauss_shape = None  # (nchan, nbin) of the portrait gauss_fit_begin made resident
        self._gauss_njoin = 0     # bands of the map gauss_fit_join made resident
        self._lib = _lib.load()
        ctx = C.c_void_p()
        _check(self._lib.pp_create(int(device), C.byref(ctx)), "pp_create")
        self._ctx = ctx
        self.device = int(device)
        if os.environ.get("PP_DEBUG_POISON"):
            # work buffers start every batch filled with NaN bit patterns: a kernel that reads
            # what no kernel of the batch wrote shows up in the results (a poor man's
            # sanitizer; run the GPU tests once with PP_DEBUG_POISON=255)
            self.set_option("debug_poison", int(os.environ["PP_DEBUG_POISON"]))
        if os.environ.get("PP_OVERLAP_POST"):
            # (run the GPU suite once with the solve / post-fit stage of enqueued batches on the context's second
            # stream: PP_OVERLAP_POST=1)
            self.set_option("overlap_post", int(os.environ["PP_OVERLAP_POST"]))

    def close(self):
        if self._ctx:
            self._lib.pp_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration --------------------------------------------------
    def set_option(self, name, value):
        _check(self._lib.pp_set_option(self._ctx, name.encode(), float(value)),
               "pp_set_option(%s)" % name)
        if name == "harm_eps":
            self._digests.clear()      # truncation is decided when a template is set

    def get_option(self, name):
        """Current value of an engine option (pp_get_option)."""
        v = C.c_double()
        _check(self._lib.pp_get_option(self._ctx, name.encode(), C.byref(v)), "pp_get_option(%s)" % name)
        return v.value

    @contextlib.contextmanager
    def options(self, **values):
        """The named engine options set to `values` for the calls made inside the block, and back
        to what get_option reported on entry after it -- also when the block raises.  An unknown
        name raises before anything is changed; blocks nest."""
        saved = [(name, self.get_option(name)) for name in values]
        try:
            for name, _ in saved:
                self.set_option(name, values[name])
            yield
        finally:
            for name, was in reversed(saved):
                self.set_option(name, was)

    @contextlib.contextmanager
    def profiled(self):
        """Kernel timing (option `profile`) switched on and the counters cleared for the calls made
        inside the block; yields a dict that holds kernel_times() of those calls after the block."""
        times = {}
        with self.options(profile=1):
            self.kernel_times(reset=True)
            try:
                yield times
            finally:
                times.update(self.kernel_times(reset=True))

    def synchronize(self):
        _check(self._lib.pp_synchronize(self._ctx), "pp_synchronize")

    # -- model ------------------------------------------------------------
    def set_model(self, model, slot=0, digest=None):
        """Upload an nchan x nbin template (numpy array or CUDA tensor).
        `digest` (optional) tags the slot's content for set_model_cached."""
        self._digests[int(slot)] = digest
        ptr, dtype, on_dev, shape, keep = _array_arg(model, "set_model: the device template")
        nchan, nbin = shape[-2:] if on_dev else shape
        _check(self._lib.pp_model_set(self._ctx, int(slot), ptr, dtype, on_dev, nchan, nbin),
               "pp_model_set")
        del keep
        return self._lib.pp_model_nharm(self._ctx, int(slot))

    def set_model_cached(self, model, slot=0):
        """Upload the template unless the same bytes are already resident in the
        slot (the reference re-reads and re-transforms it for every subint,
        pptoas.py:352-379)."""
        m = np.ascontiguousarray(model)
        try:
            import xxhash
            digest = (m.shape, m.dtype.str,
                      xxhash.xxh3_128_digest(m.view(np.uint8).reshape(-1)))
        except ImportError:
            digest = None
        if digest is None or self._digests.get(int(slot)) != digest:
            self.set_model(m, slot=slot, digest=digest)
        return self.model_nharm(slot)

    def model_nharm(self, slot=0):
        return self._lib.pp_model_nharm(self._ctx, int(slot))

    def _slot_changed(self, slot):
        """The library rewrote the slot's template: forget what set_model_cached knew of it;
        returns the number of harmonics kept."""
        self._digests.pop(int(slot), None)
        return int(self._lib.pp_model_nharm(self._ctx, int(slot)))

    # -- the fit ------------------------------------------------------------
    def fit_batch(self, data, freqs, P, init_params, errs=None, nu_fits=None,
                  nu_outs=None, fit_flags=(1, 1, 0, 0, 0), log10_tau=False,
                  option=0, is_toa=True, model_slot=None, chan_mask=None,
                  per_channel=True, objective=False, seed_ns=0, method='trust-ncg',
                  records=None, ref_seed=None):
        """Fit nsub subints.  data: [nsub,nchan,nbin] numpy array (f64/f32) or
        CUDA tensor.  freqs: [nchan] or [nsub,nchan].  Returns a dict of arrays
        (see include/pp_toas.h pp_fit_out).  errs / chan_mask may be CUDA
        tensors [nsub,nchan]; per_channel="device" leaves scales, scale_errs and
        channel_snrs in HBM as CUDA tensors instead of copying them out;
        records (a float64 CUDA tensor [nsub, 18]) receives one TOA record per
        subint on the device (dist.RECORD_FIELDS).
        seed_ns > 0 replaces init_params[:, 0] by a phase seeded on the device.
        method: 'trust-ncg' follows SciPy's trust-ncg iteration to the very point
        where the reference stops; 'newton' ('Newton-CG', 'TNC') converges to the
        rounding of the objective in fewer evaluations.
        ref_seed: dict(weights=[nsub,nchan] (array, CUDA tensor or None), model_profs=[nsub,nbin]
        or [nbin], nu_mean=[nsub], Ns=100, bounds=(-0.5, 0.5), finish='simplex') -- the
        reference's own phase guess (pptoas.py:421-457) is formed inside the fit, from the same
        single pass over the portraits, and replaces init_params[:, 0]; the result gains
        "seed_phase".  Raises EngineNotSupported when the batch has no single-pass path
        (include/pp_toas.h pp_seed_ref): form the guess with reference_phase_seed then."""
        b = self._prepare(data, freqs, P, init_params, errs, nu_fits, nu_outs, fit_flags, log10_tau, option,
                          is_toa, model_slot, chan_mask, per_channel, objective, seed_ns, method, records,
                          ref_seed)
        _check(self._lib.pp_fit_portrait_batch(self._ctx, C.byref(b.fin), C.byref(b.fout)),
               "pp_fit_portrait_batch")
        return b.finish()

    def _prepare(self, data, freqs, P, init_params, errs=None, nu_fits=None, nu_outs=None,
                 fit_flags=(1, 1, 0, 0, 0), log10_tau=False, option=0, is_toa=True, model_slot=None,
                 chan_mask=None, per_channel=True, objective=False, seed_ns=0, method='trust-ncg',
                 records=None, ref_seed=None):
        """fit_batch's arguments (and defaults: submit and enqueue hand theirs straight through)
        as a _Batch ready for one of the three C calls."""
        if method not in METHODS:
            raise EngineError("unknown method %r" % (method,))
        if records is not None and not (
                _is_device_array(records) and records.is_contiguous() and
                records.element_size() == 8 and tuple(records.shape)[-1] == _lib.PP_RECORD_WIDTH):
            raise EngineError("records must be a contiguous float64 CUDA tensor [nsub, %d]"
                              % _lib.PP_RECORD_WIDTH)
        fin, in_keep, aux_given = self._fit_in(data, freqs, P, init_params, errs, nu_fits, nu_outs, fit_flags,
                                               log10_tau, option, is_toa, model_slot, chan_mask, seed_ns, method)
        seed_keep = None if ref_seed is None else self._seed_ref(fin, ref_seed, aux_given)
        fout, res = self._fit_out(fin, data.device if fin.data_on_device else None, per_channel, objective,
                                  records, fit_flags)
        if seed_keep is not None:
            res["seed_phase"] = seed_keep[-1]
        return _Batch(res, fin, fout, (in_keep, seed_keep, records))

    def _fit_in(self, data, freqs, P, init_params, errs, nu_fits, nu_outs, fit_flags, log10_tau, option,
                is_toa, model_slot, chan_mask, seed_ns, method):
        """The inputs as a FitIn: (fin, what it points to, whether errs / chan_mask were given)."""
        dptr, dtype, on_dev, shape, keep = _array_arg(data, "device data")
        if not on_dev and len(shape) == 2:      # (one host portrait: a batch of one subint)
            shape = (1,) + shape
        nsub, nchan, nbin = shape
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        if freqs.ndim == 1:
            if freqs.shape[0] != nchan:
                raise EngineError("freqs has %d entries for %d channels" %
                                  (freqs.shape[0], nchan))
            fstride = 0
        else:
            if freqs.shape != (nsub, nchan):
                raise EngineError("freqs shape %s != (%d, %d)" %
                                  (freqs.shape, nsub, nchan))
            fstride = nchan
        P = _f64(P, (nsub,))
        x0 = _f64(init_params, (nsub, 5))
        aux_dev = _is_device_array(errs) or _is_device_array(chan_mask)
        if aux_dev:
            for t, nm in ((errs, "errs"), (chan_mask, "chan_mask")):
                if t is not None and not (_is_device_array(t) and t.is_contiguous()
                                          and tuple(t.shape) == (nsub, nchan)):
                    raise EngineError("%s must be a contiguous CUDA tensor "
                                      "[nsub,nchan] when either aux input is" % nm)
            if errs is not None and errs.element_size() != 8:
                raise EngineError("device errs must be float64")
            if chan_mask is not None and chan_mask.element_size() != 1:
                raise EngineError("device chan_mask must be uint8")
        else:
            errs = _f64(errs, (nsub, nchan))
        nu_fits = _nu_array(nu_fits, nsub)
        nu_outs = _nu_array(nu_outs, nsub)
        slot = None if model_slot is None else np.ascontiguousarray(
            np.broadcast_to(model_slot, (nsub,)), dtype=np.int32)
        mask = None
        if chan_mask is not None and not aux_dev:
            mask = np.ascontiguousarray(np.broadcast_to(chan_mask, (nsub, nchan)),
                                        dtype=np.uint8)

        fin = FitIn()
        fin.nsub, fin.nchan, fin.nbin = nsub, nchan, nbin
        fin.data = dptr
        fin.data_dtype, fin.data_on_device = dtype, on_dev
        fin.model_slot = None if slot is None else slot.ctypes.data_as(c_int32_p)
        fin.freqs, fin.freqs_stride = _dp(freqs), fstride
        fin.aux_on_device = int(aux_dev)
        if aux_dev:
            fin.errs = None if errs is None else C.cast(errs.data_ptr(), c_double_p)
            fin.chan_mask = None if chan_mask is None else C.cast(
                chan_mask.data_ptr(), c_uint8_p)
        else:
            fin.errs = _dp(errs)
            fin.chan_mask = None if mask is None else mask.ctypes.data_as(c_uint8_p)
        fin.P, fin.init_params = _dp(P), _dp(x0)
        fin.nu_fits, fin.nu_outs = _dp(nu_fits), _dp(nu_outs)
        for j in range(5):
            fin.fit_flags[j] = 1 if fit_flags[j] else 0
        fin.log10_tau = int(bool(log10_tau))
        fin.option, fin.is_toa = int(option), int(bool(is_toa))
        fin.seed_ns = int(seed_ns)
        fin.method = METHODS[method]
        return fin, (keep, freqs, P, x0, errs, nu_fits, nu_outs, slot, mask, chan_mask), \
            errs is not None or chan_mask is not None

    def _seed_ref(self, fin, ref_seed, aux_given):
        """fit_batch's ref_seed dict as a SeedRef hung into `fin`; returns what must stay alive:
        (the SeedRef, what it points to ..., the seed_phase output array)."""
        nsub, nchan, nbin = fin.nsub, fin.nchan, fin.nbin
        aux_dev = bool(fin.aux_on_device)
        sr = SeedRef()
        w = ref_seed.get("weights")
        if w is not None and _is_device_array(w):
            if not aux_dev and aux_given:
                raise EngineError("ref_seed weights on the device need errs / chan_mask there too")
            if not (w.is_contiguous() and w.element_size() == 8 and tuple(w.shape) == (nsub, nchan)):
                raise EngineError("device ref_seed weights must be a contiguous float64 tensor [nsub,nchan]")
            fin.aux_on_device = 1
            sr.weights = C.cast(w.data_ptr(), c_double_p)
        elif w is not None:
            if aux_dev:
                raise EngineError("ref_seed weights must be a CUDA tensor when errs / chan_mask are")
            w = _f64(w, (nsub, nchan))
            sr.weights = _dp(w)
        mp = np.ascontiguousarray(ref_seed["model_profs"], dtype=np.float64)
        if mp.ndim == 1:
            sr.model_prof_stride = 0
        elif mp.shape == (nsub, nbin):
            sr.model_prof_stride = nbin
        else:
            raise EngineError("ref_seed model_profs must be [nbin] or [nsub,nbin]")
        if mp.shape[-1] != nbin:
            raise EngineError("ref_seed model_profs has %d bins, the data %d" % (mp.shape[-1], nbin))
        sr.model_profs = _dp(mp)
        numean = _f64(ref_seed["nu_mean"], (nsub,))
        sr.nu_mean = _dp(numean)
        lo_hi = ref_seed.get("bounds", (-0.5, 0.5))
        sr.lo, sr.hi = float(lo_hi[0]), float(lo_hi[1])
        sr.Ns = int(ref_seed.get("Ns", 100))
        sr.finish = 1 if ref_seed.get("finish", "simplex") == "simplex" else 0
        sphase = np.empty(nsub)
        sr.seed_phase = _dp(sphase)
        fin.ref_seed = C.pointer(sr)
        return sr, w, mp, numean, sphase

    def _fit_out(self, fin, data_device, per_channel, objective, records, fit_flags):
        """The result dict (arrays the library fills in place) and the FitOut that points into
        it.  `data_device`: the device of device-resident portraits, None for host portraits."""
        nsub, nchan = fin.nsub, fin.nchan
        res = dict(params=np.empty((nsub, 5)), param_errs=np.empty((nsub, 5)),
                   nu_refs=np.empty((nsub, 3)), cov=np.empty((nsub, 5, 5)),
                   chi2=np.empty(nsub), red_chi2=np.empty(nsub), snr=np.empty(nsub),
                   nfeval=np.empty(nsub, dtype=np.int32),
                   return_code=np.empty(nsub, dtype=np.int32),
                   npass=np.empty(nsub, dtype=np.int32),
                   duration=np.zeros(1))
        chan_dev = (per_channel == "device")
        if chan_dev:
            import torch
            dev = data_device if data_device is not None else torch.device("cuda", self.device)
            res.update({k: torch.empty((nsub, nchan), dtype=torch.float64, device=dev)
                        for k in ("scales", "scale_errs", "channel_snrs")})
        elif per_channel:
            res.update(scales=np.empty((nsub, nchan)),
                       scale_errs=np.empty((nsub, nchan)),
                       channel_snrs=np.empty((nsub, nchan)))
        if objective:
            res.update(obj_f=np.empty(nsub), obj_grad=np.empty((nsub, 5)),
                       obj_hess=np.empty((nsub, 5, 5)))
        fout = FitOut()
        fout.chan_on_device = int(chan_dev)
        if records is not None:
            if int(records.shape[0]) != nsub:
                raise EngineError("records has %d rows for %d subints" % (records.shape[0], nsub))
            fout.records_dev = C.cast(records.data_ptr(), c_double_p)
        for name, _ in FitOut._fields_:
            if name in ("chan_on_device", "records_dev"):
                continue
            arr = res.get(name)
            if arr is None:
                setattr(fout, name, None)
            elif _is_device_array(arr):
                setattr(fout, name, C.cast(arr.data_ptr(), c_double_p))
            elif arr.dtype == np.int32:
                setattr(fout, name, arr.ctypes.data_as(c_int32_p))
            else:
                setattr(fout, name, arr.ctypes.data_as(c_double_p))
        res["fit_flags"] = [1 if f else 0 for f in fit_flags]
        return fout, res

    def submit(self, *args, **kwargs):
        """fit_batch started on a worker thread of the context (pp_fit_submit): returns at
        once; wait() returns the result dict.  The caller's arrays must not be modified
        until then.  Two engines on one GPU overlap their copies and kernels."""
        b = self._prepare(*args, **kwargs)
        _check(self._lib.pp_fit_submit(self._ctx, C.byref(b.fin), C.byref(b.fout)), "pp_fit_submit")
        self._pending = b       # (everything the argument blocks point to stays alive until wait())

    def enqueue(self, *args, **kwargs):
        """fit_batch queued on the engine's stream (pp_fit_enqueue): returns without waiting for the
        GPU; collect() returns the result dict of the OLDEST enqueued batch.  Up to three batches may be
        pending: enqueue batch k + 1, then collect batch k, and the GPU never waits for the host
        between batches.  The caller's arrays must not be modified until the batch is collected."""
        b = self._prepare(*args, **kwargs)
        _check(self._lib.pp_fit_enqueue(self._ctx, C.byref(b.fin), C.byref(b.fout)), "pp_fit_enqueue")
        self._queue.append(b)   # (everything the argument blocks point to stays alive until collect())

    def collect(self):
        """Complete the oldest enqueued batch; returns what fit_batch returns."""
        if not self._queue:
            raise EngineError("nothing enqueued")
        # the batch (result arrays + everything the argument blocks point to) leaves the queue only once the C
        # call is through with it; if that call fails, the Python queue is brought back in step with the
        # library's (pp_fit_pending): the failed batch is gone there, younger ones may still be queued
        b = self._queue[0]
        try:
            _check(self._lib.pp_fit_collect(self._ctx), "pp_fit_collect")
        finally:
            left = self._lib.pp_fit_pending(self._ctx)
            left = left if left >= 0 else 0
            while len(self._queue) > left:
                self._queue.pop(0)
        return b.finish()

    def poll(self):
        """True once the submitted batch is complete."""
        rc = self._lib.pp_fit_poll(self._ctx)
        if rc < 0:
            _check(rc, "pp_fit_poll")
        return bool(rc)

    def wait(self):
        """Block until the submitted batch is complete; returns what fit_batch returns."""
        if self._pending is None:
            raise EngineError("nothing submitted")
        b, self._pending = self._pending, None
        _check(self._lib.pp_fit_wait(self._ctx), "pp_fit_wait")
        return b.finish()

    # -- parity hooks / measurement ---------------------------------------
    def rfft_rows(self, rows):
        src, dtype, on_dev, (nrows, nbin), keep = _array_arg(rows, "rfft_rows: rows")
        if on_dev:
            raise EngineError("rfft_rows takes host rows")
        out = np.empty((nrows, nbin // 2 + 1), dtype=np.complex128)
        _check(self._lib.pp_rfft_rows(self._ctx, src, dtype, nrows, nbin, out.ctypes.data_as(c_double_p)),
               "pp_rfft_rows")
        return out

    def fit_phase_shift_batch(self, data, model, noise=None, bounds=(-0.5, 0.5),
                              Ns=100, finish='newton'):
        """1-D FFTFIT of nprof profile pairs: Ns-point brute grid over `bounds` (both
        ends included), then finish = 'newton': the exact local optimum; 'simplex':
        what scipy.optimize.brute does by default and the reference returns
        (pplib.py:2085) -- Nelder-Mead to xtol = ftol = 1e-4, step for step.
        Returns [nprof, 7]: phase, phase_err, scale, scale_err, snr, red_chi2, duration."""
        if finish not in ('newton', 'simplex'):
            raise ValueError("finish must be 'newton' or 'simplex'")
        d = _f64(np.atleast_2d(data))
        nprof, nbin = d.shape
        m = _f64(np.atleast_2d(model), (nprof, nbin))
        nz = self._noise_arg(noise, nprof)
        out = np.empty((nprof, 7))
        with self.options(fps_finish=1 if finish == 'simplex' else 0):
            _check(self._lib.pp_fit_phase_shift_batch(
                self._ctx, _dp(d), _dp(m), _dp(nz), nprof, nbin, float(bounds[0]),
                float(bounds[1]), int(Ns), _dp(out)), "pp_fit_phase_shift_batch")
        return out

    @staticmethod
    def _noise_arg(noise, nprof):
        if noise is None:
            return np.full(nprof, np.nan)
        if isinstance(noise, np.ndarray) and noise.dtype.kind == "f":
            return _f64(noise, (nprof,))
        return _f64([np.nan if v is None else v for v in
                     np.broadcast_to(np.asarray(noise, dtype=object), (nprof,))])

    def fit_phase_tau_batch(self, data, model, noise=None, tau_guess=0.0, phi_guess=None,
                            log10_tau=True, bounds=(-0.5, 0.5), Ns=100):
        """Narrowband scattering fit of nprof profile pairs: a phase and a scattering time
        [rot] each, fitted jointly -- fit_portrait_full on a one-channel portrait with
        fit_flags [1,0,0,1,0].  tau_guess (scalar or [nprof]) is tau, or log10 tau under
        log10_tau; phi_guess None / NaN asks for an Ns-point grid over `bounds` at the
        guessed tau.  Returns [nprof, 11]: phi, phi_err, tau (or log10 tau), tau_err,
        scale, scale_err, snr, red_chi2, cov_phi_tau, nfeval, return_code
        (include/pp_toas.h, pp_fit_phase_tau_batch)."""
        d = _f64(np.atleast_2d(data))
        nprof, nbin = d.shape
        m = _f64(np.atleast_2d(model), (nprof, nbin))
        nz = self._noise_arg(noise, nprof)
        guess = np.empty((nprof, 2))
        guess[:, 0] = np.nan if phi_guess is None else np.asarray(phi_guess, dtype=np.float64)
        guess[:, 1] = np.asarray(tau_guess, dtype=np.float64)
        out = np.empty((nprof, 11))
        _check(self._lib.pp_fit_phase_tau_batch(
            self._ctx, _dp(d), _dp(m), _dp(nz), _dp(guess), nprof, nbin, float(bounds[0]),
            float(bounds[1]), int(Ns), int(bool(log10_tau)), _dp(out)), "pp_fit_phase_tau_batch")
        return out

    def reference_phase_seed(self, ports, freqs, P, weights, model_profs, phi=0.0, DM=0.0, GM=0.0,
                             nu_DM=np.inf, nu_GM=np.inf, bounds=(-0.5, 0.5), Ns=100, finish='simplex'):
        """fit_phase_shift(np.average(rotate_data(port_i, phi_i, DM_i, P_i, freqs_i, nu_DM),
        axis=0, weights=weights_i), model_profs_i, Ns) for every subint, the rotation
        and the channel mean fused into one read of the portraits (pptoas.py:421-457).
        Returns [nsub, 7] like fit_phase_shift_batch."""
        src, dtype, on_dev, (nsub, nchan, nbin), keep = _array_arg(ports, "reference_phase_seed: device ports")
        freqs, fstride, P, par = self._subint_args(freqs, P, (phi, DM, GM), nsub, nchan)
        w = _f64(weights, (nsub, nchan))
        mp = _f64(np.broadcast_to(np.asarray(model_profs, dtype=np.float64), (nsub, nbin)))
        out = np.empty((nsub, 7))
        with self.options(fps_finish=1 if finish == 'simplex' else 0):
            _check(self._lib.pp_reference_phase_seed(
                self._ctx, src, dtype, on_dev, nsub, nchan, nbin, _dp(freqs), fstride, _dp(P), _dp(par),
                float(nu_DM), float(nu_GM), _dp(w), _dp(mp), float(bounds[0]), float(bounds[1]), int(Ns),
                _dp(out)), "pp_reference_phase_seed")
        return out

    def rotate_portraits(self, ports, freqs, P, phi=0.0, DM=0.0, GM=0.0, nu_DM=np.inf,
                         nu_GM=np.inf):
        """Fourier-rotate ports[nsub,nchan,nbin] (numpy -> new numpy array; CUDA
        tensor -> rotated in place) by per-subint (phi, DM, GM)."""
        src, dtype, on_dev, (nsub, nchan, nbin), keep = _array_arg(ports, "rotate_portraits: device ports")
        out, dst = keep, src
        if not on_dev:
            out = np.empty_like(keep)
            dst = C.c_void_p(out.ctypes.data)
        freqs, fstride, P, par = self._subint_args(freqs, P, (phi, DM, GM), nsub, nchan)
        _check(self._lib.pp_rotate_portraits(self._ctx, src, dst, dtype, on_dev, nsub, nchan,
                                             nbin, _dp(freqs), fstride, _dp(P), _dp(par),
                                             float(nu_DM), float(nu_GM)),
               "pp_rotate_portraits")
        return out

    @staticmethod
    def _gauss_args(model, P):
        p = np.asarray(model["params"], dtype=np.float64)
        ng = int(model["ngauss"])
        comps = np.ascontiguousarray(p[2:2 + 6 * ng].reshape(ng, 6))
        tau_rot = 0.0
        if p[1] != 0.0:
            if P is None:
                raise ValueError("need the period P for a model with TAU != 0")
            tau_rot = float(p[1]) / float(P)
        return (str(model["code"]).encode(), float(model["nu_ref"]), float(p[0]), tau_rot,
                float(model["alpha"]), ng, comps)

    def gaussian_portrait(self, model, freqs, nbin, P=None, out=None):
        """nchan x nbin portrait of a parsed .gmodel (gmodel.parse_gmodel) built
        on the device; `out` may be a CUDA float64 tensor [nchan,nbin] (filled in
        place), else a NumPy array is returned."""
        freqs = _f64(freqs)
        nchan = len(freqs)
        code, nu_ref, dc, tau_rot, alpha, ng, comps = self._gauss_args(model, P)
        if out is not None and _is_device_array(out):
            dst, on_dev, ret = C.c_void_p(out.data_ptr()), 1, out
        else:
            ret = np.empty((nchan, int(nbin)))
            dst, on_dev = C.c_void_p(ret.ctypes.data), 0
        _check(self._lib.pp_gaussian_portrait(self._ctx, nchan, int(nbin), _dp(freqs), code, nu_ref,
                                              dc, tau_rot, alpha, ng, _dp(comps), dst, on_dev),
               "pp_gaussian_portrait")
        return ret

    def set_model_gaussian(self, model, freqs, nbin, P=None, slot=0):
        """Synthesise a .gmodel template on the device straight into a model slot;
        returns the number of harmonics kept."""
        freqs = _f64(freqs)
        code, nu_ref, dc, tau_rot, alpha, ng, comps = self._gauss_args(model, P)
        _check(self._lib.pp_model_set_gaussian(self._ctx, int(slot), len(freqs), int(nbin),
                                               _dp(freqs), code, nu_ref, dc, tau_rot, alpha, ng,
                                               _dp(comps)), "pp_model_set_gaussian")
        return self._slot_changed(slot)

    def _spline_args(self, mean_prof, eigvec, tck, nbin):
        from .splmodel import spline_device_args
        basis, t, coefs, k = spline_device_args(mean_prof, eigvec, tck, nbin)
        ncomp = basis.shape[0] - 1
        return basis, t, coefs, k, ncomp

    def spline_portrait(self, mean_prof, eigvec, tck, freqs, nbin=None):
        """nchan x nbin portrait of a spline model (gen_spline_portrait, pplib.py:932-956)
        built on the device; returns a NumPy array."""
        freqs = _f64(freqs)
        basis, t, coefs, k, ncomp = self._spline_args(mean_prof, eigvec, tck, nbin)
        out = np.empty((len(freqs), basis.shape[1]))
        _check(self._lib.pp_spline_portrait(self._ctx, len(freqs), basis.shape[1], _dp(freqs), ncomp,
                                            _dp(basis), len(t), _dp(t), _dp(coefs), k,
                                            C.c_void_p(out.ctypes.data), 0), "pp_spline_portrait")
        return out

    def set_model_spline(self, mean_prof, eigvec, tck, freqs, nbin=None, slot=0):
        """Synthesise a spline (.spl) template on the device straight into a model
        slot (no host portrait); returns the number of harmonics kept."""
        freqs = _f64(freqs)
        basis, t, coefs, k, ncomp = self._spline_args(mean_prof, eigvec, tck, nbin)
        _check(self._lib.pp_model_set_spline(self._ctx, int(slot), len(freqs), basis.shape[1], _dp(freqs),
                                             ncomp, _dp(basis), len(t), _dp(t), _dp(coefs), k),
               "pp_model_set_spline")
        return self._slot_changed(slot)

    def apply_response(self, slot, rconst=None, smear_wid=None):
        """Multiply the template resident in `slot` by an instrumental response in the
        Fourier domain, on the device: rconst[nbin/2 + 1] (complex, the product of the
        constant responses) and/or smear_wid[nchan] (dispersive smearing width of each
        channel in rotations).  pptoaslib.py:145-179."""
        rc = None if rconst is None else np.ascontiguousarray(
            np.asarray(rconst, dtype=np.complex128)).view(np.float64)
        wd = None if smear_wid is None else _f64(smear_wid)
        _check(self._lib.pp_model_apply_response(self._ctx, int(slot), _dp(rc), _dp(wd)),
               "pp_model_apply_response")
        return self._slot_changed(slot)

    def model_means(self, slot, nchan, nbin):
        """Mean over phase of every channel of the template in `slot` (its DC
        harmonic / nbin)."""
        dc = np.empty(int(nchan))
        _check(self._lib.pp_model_dc(self._ctx, int(slot), _dp(dc)), "pp_model_dc")
        return dc / float(nbin)

    @staticmethod
    def _subint_args(freqs, P, triple, nsub, nchan):
        """(freqs, freqs_stride, P, par3) as the entry points that take portraits plus
        per-subint arrays want them: freqs[nchan] shared (stride 0) or [nsub,nchan];
        `triple`: three scalars or per-subint arrays stacked into par3[nsub,3] (None:
        the call has no such triple)."""
        freqs = np.ascontiguousarray(freqs, dtype=np.float64)
        par = None if triple is None else np.ascontiguousarray(np.stack([
            np.broadcast_to(np.asarray(v, dtype=np.float64), (nsub,)) for v in triple], axis=1))
        return freqs, 0 if freqs.ndim == 1 else nchan, _f64(P, (nsub,)), par

    def align_accumulate(self, ports, freqs, P, phase, DM, nu_ref, weights):
        """ppalign's accumulation (ppalign.py:199-206): returns
        (sum_i w[i,n] * rotate_data(ports[i,n], phase_i, DM_i, P_i, freqs, nu_ref_i)
        as [nchan,nbin], sum_i w[i,n] as [nchan]); rows with w = 0 are skipped."""
        src, dtype, on_dev, (nsub, nchan, nbin), keep = _array_arg(ports, "align_accumulate: device ports")
        freqs, fstride, P, par = self._subint_args(freqs, P, (phase, DM, nu_ref), nsub, nchan)
        w = _f64(weights, (nsub, nchan))
        aligned = np.empty((nchan, nbin))
        totw = np.empty(nchan)
        _check(self._lib.pp_align_accumulate(self._ctx, src, dtype, on_dev, nsub, nchan, nbin,
                                             _dp(freqs), fstride, _dp(P), _dp(par), _dp(w),
                                             _dp(aligned), _dp(totw)), "pp_align_accumulate")
        return aligned, totw

    def align_begin(self, npol, nchan_model, nbin):
        """Start (or start over) the device-resident accumulator of align_archives
        (ppalign.py:116-117): aligned_port[npol,nchan_model,nbin] and total_weights, zeroed."""
        self._align_shape = None
        _check(self._lib.pp_align_begin(self._ctx, int(npol), int(nchan_model), int(nbin)), "pp_align_begin")
        self._align_shape = (int(npol), int(nchan_model), int(nbin))

    def align_add(self, ports, freqs, P, phase, DM, nu_ref, weights, chan_map=None):
        """ppalign.py:202-208 for every subint of ports[nsub,npol,nchan,nbin] (or
        [nsub,nchan,nbin]: one polarisation; NumPy or a device tensor): row (i, ipol, n),
        rotated by (phase_i, DM_i, nu_ref_i) and weighted by weights[i,n] -- 0 or NaN skips
        it --, is added to accumulator row (ipol, chan_map[i,n]); chan_map None is the
        identity.  The accumulator's bits do not depend on how the subints are cut into calls."""
        src, dtype, on_dev, shape, keep = _array_arg(ports, "align_add: device ports")
        if len(shape) == 3:
            shape = (shape[0], 1) + tuple(shape[1:])
        if len(shape) != 4:
            raise ValueError("ports must be [nsub,npol,nchan,nbin] or [nsub,nchan,nbin]")
        nsub, npol, nchan, nbin = shape
        freqs, fstride, P, par = self._subint_args(freqs, P, (phase, DM, nu_ref), nsub, nchan)
        w = _f64(weights, (nsub, nchan))
        cm = None
        if chan_map is not None:
            cm = np.ascontiguousarray(np.broadcast_to(np.asarray(chan_map, dtype=np.int32), (nsub, nchan)))
        _check(self._lib.pp_align_add(self._ctx, src, dtype, on_dev, nsub, npol, nchan, nbin, _dp(freqs),
                                      fstride, _dp(P), _dp(par), _dp(w),
                                      None if cm is None else cm.ctypes.data_as(c_int32_p)), "pp_align_add")
        del keep

    def align_finish(self, rot_phase=0.0, to_slot=-1):
        """ppalign.py:210-212 (and the overall rotation of :220-226) of the resident
        accumulator: returns (aligned_port[npol,nchan_model,nbin], total_weights[nchan_model]);
        rows of positive total weight are divided by it.  to_slot >= 0 also makes polarisation
        0 the template of that model slot, from the device copy (the bits set_model of the
        returned array would give).  May be called again, e.g. with another rot_phase."""
        if self._align_shape is None:
            raise EngineError("align_finish: no accumulator (align_begin first)")
        npol, nchan, nbin = self._align_shape
        aligned, totw = np.empty((npol, nchan, nbin)), np.empty(nchan)
        _check(self._lib.pp_align_finish(self._ctx, float(rot_phase), _dp(aligned), _dp(totw), int(to_slot)),
               "pp_align_finish")
        if int(to_slot) >= 0:
            self._slot_changed(to_slot)
        return aligned, totw

    def channel_red_chi2(self, ports, freqs, P, params, nu_refs, scales, errs, slots=None):
        """Per-channel reduced chi^2 of fitted subints, time domain, dof = nbin-2
        (get_channels_to_zap, pptoas.py:1239-1245).  params[nsub,5] = phi, DM, GM,
        tau [rot, linear], alpha at nu_refs[nsub,3]; the template is the resident
        model slot of each subint."""
        src, dtype, on_dev, (nsub, nchan, nbin), keep = _array_arg(ports, "channel_red_chi2: device ports")
        freqs, fstride, P, _ = self._subint_args(freqs, P, None, nsub, nchan)
        params = _f64(params, (nsub, 5))
        nu_refs = _f64(nu_refs, (nsub, 3))
        scales = _f64(scales, (nsub, nchan))
        errs = _f64(errs, (nsub, nchan))
        sl = None
        if slots is not None:
            sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots, dtype=np.int32), (nsub,)))
        out = np.empty((nsub, nchan))
        _check(self._lib.pp_channel_red_chi2(
            self._ctx, src, dtype, on_dev, nsub, nchan, nbin,
            None if sl is None else sl.ctypes.data_as(c_int32_p), _dp(freqs), fstride, _dp(P),
            _dp(params), _dp(nu_refs), _dp(scales), _dp(errs), _dp(out)), "pp_channel_red_chi2")
        return out

    def fit_residuals(self, ports, freqs, P, params, nu_refs, scales, errs=None, mask=None, slots=None,
                      frame="model", want=("resid",)):
        """The fit's residual portrait (show_fit(..., return_fit=True), pptoas.py:1317-1419).
        params[nsub,5] = phi, DM, GM, tau [rot, linear], alpha at nu_refs[nsub,3]; scales[nsub,nchan]
        the fitted amplitudes; the template is the resident model slot of each subint.  frame
        "model": `port` is the data rotated onto the template and `model` the scattered, scaled
        template (the reference's pair); frame "data": `port` is the data as it is and `model` the
        template rotated back onto it.  `resid` = port - model from ONE inverse transform;
        `red_chi2`[nsub,nchan] (needs errs) is channel_red_chi2's figure, the same in both frames.
        mask[nsub,nchan]: rows of weight 0 or NaN are not read and come back as zeros (red_chi2 NaN).
        Returns a dict of the arrays named in `want`: NumPy for NumPy input, device tensors (new
        ones, of the input's type; red_chi2 float64) for a device tensor."""
        want = tuple(want)
        if not want or any(w not in _RESID_OUTPUTS for w in want):
            raise ValueError("want must name some of %s" % (_RESID_OUTPUTS,))
        if frame not in _RESID_FRAMES:
            raise ValueError("frame must be 'model' or 'data', not %r" % (frame,))
        if "red_chi2" in want and errs is None:
            raise ValueError("fit_residuals: red_chi2 needs errs")
        src, dtype, on_dev, (nsub, nchan, nbin), keep = _array_arg(ports, "fit_residuals: device ports")
        freqs, fstride, P, _ = self._subint_args(freqs, P, None, nsub, nchan)
        params = _f64(params, (nsub, 5))
        nu_refs = _f64(nu_refs, (nsub, 3))
        scales = _f64(scales, (nsub, nchan))
        errs = _f64(errs, (nsub, nchan))
        mask = _f64(mask, (nsub, nchan))
        sl = None
        if slots is not None:
            sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots, dtype=np.int32), (nsub,)))
        out, ptr = {}, {}
        for name in _RESID_OUTPUTS:
            if name not in want:
                ptr[name] = None
            elif on_dev:
                import torch
                out[name] = (torch.empty((nsub, nchan), dtype=torch.float64, device=keep.device)
                             if name == "red_chi2" else torch.empty_like(keep))
                ptr[name] = C.c_void_p(out[name].data_ptr())
            else:
                out[name] = np.empty((nsub, nchan)) if name == "red_chi2" else np.empty_like(keep)
                ptr[name] = C.c_void_p(out[name].ctypes.data)
        _check(self._lib.pp_fit_residuals(
            self._ctx, src, dtype, on_dev, nsub, nchan, nbin,
            None if sl is None else sl.ctypes.data_as(c_int32_p), _dp(freqs), fstride, _dp(P),
            _dp(params), _dp(nu_refs), _dp(scales), _dp(errs), _dp(mask), _RESID_FRAMES[frame],
            ptr["port"], ptr["model"], ptr["resid"], ptr["red_chi2"]), "pp_fit_residuals")
        return out

    def channel_noise(self, ports, norm=None, weights=None, method='PS', fact=1.1, fn='exp_dc'):
        """ppzap's channel noise (ppzap.py:222-230): every row normalised as
        normalize_portrait(port, method=norm, weights) does (pplib.py:2462-2507), then
        get_noise(row, method).  method 'PS' is get_noise_PS(row, frac=4); 'fit' is
        get_noise_fit(row, fact) (pplib.py:2255-2287) with find_kc(pows, fn=fn) inside it,
        all of it on the device (norm 'rms' then divides by the fitted noise).  ports:
        [nsub,nchan,nbin] or [nrows,nbin] (one portrait), NumPy or a device tensor;
        weights: [nsub,nchan] (norm 'prof').  Returns (noise, norms) shaped like ports
        without the bin axis; rows with no non-zero sample keep norm 1 and noise 0."""
        if norm not in _lib.PP_NORMS:
            raise ValueError("norm must be one of None, 'mean', 'max', 'prof', 'rms', 'abs'")
        _noise_method(method, fn)
        shape = tuple(int(v) for v in ports.shape)
        if len(shape) not in (2, 3):
            raise ValueError("ports must be [nsub,nchan,nbin] or [nrows,nbin]")
        nbin = shape[-1]
        nrows = int(np.prod(shape[:-1]))
        src, dtype, on_dev, _, keep = _array_arg(ports, "channel_noise: device ports")
        div = None
        if norm == 'prof':
            div = self._prof_norms(ports, weights)
        norms, noise = np.empty(nrows), np.empty(nrows)
        if method == 'PS':
            _check(self._lib.pp_channel_noise(self._ctx, src, dtype, on_dev, nrows, nbin, _lib.PP_NORMS[norm],
                                              _dp(div), _dp(norms), _dp(noise)), "pp_channel_noise")
        else:
            _check(self._lib.pp_channel_noise_fit(self._ctx, src, dtype, on_dev, nrows, nbin, _lib.PP_NOISEFIT_ROWS,
                                                  _lib.PP_KC_FNS[fn], float(fact), _lib.PP_NORMS[norm], _dp(div),
                                                  _dp(norms), _dp(noise), None, None), "pp_channel_noise_fit")
        return noise.reshape(shape[:-1]), norms.reshape(shape[:-1])

    def find_kc(self, pows, fn='exp_dc', return_cell=False, fact=1.1, return_noise=False):
        """pplib.find_kc (pplib.py:1465-1495) of every row of pows [..., H] (power spectra, NumPy
        or an f64 device tensor; 5 <= H <= 2049): the cut-off harmonic where the noise floor of
        log10(pows) starts, from the 20 x 20 x 20 opt.brute grid of fn ('exp_dc' or 'half_tri')
        evaluated in closed form on the device.  Returns kc (int32, shaped like pows without its
        last axis); return_cell adds the winning grid cell [..., 3] = (ia, ib, idc), and
        return_noise adds sqrt(mean(pows[int(k):])) of get_noise_fit (pplib.py:2273-2277) for
        k = fact kc."""
        _noise_method('fit', fn)
        if not _is_device_array(pows):
            pows = np.ascontiguousarray(pows, dtype=np.float64)
        src, dtype, on_dev, shape, keep = _array_arg(pows, "find_kc: device power spectra")
        if dtype != PP_F64:
            raise ValueError("find_kc: power spectra must be float64")
        if len(shape) < 1 or not 5 <= shape[-1] <= 2049:
            raise ValueError("find_kc: pows must be [..., H] with 5 <= H <= 2049")
        H = int(shape[-1])
        nrows = int(np.prod(shape[:-1]))
        norms, noise = np.empty(nrows), np.empty(nrows)
        kc, cell = np.empty(nrows, dtype=np.int32), np.empty((nrows, 3), dtype=np.int32)
        _check(self._lib.pp_channel_noise_fit(self._ctx, src, dtype, on_dev, nrows, 2 * (H - 1), _lib.PP_NOISEFIT_POWS,
                                              _lib.PP_KC_FNS[fn], float(fact), _lib.PP_NORMS[None], None, _dp(norms),
                                              _dp(noise), kc.ctypes.data_as(c_int32_p), cell.ctypes.data_as(c_int32_p)),
               "pp_channel_noise_fit")
        out = (kc.reshape(shape[:-1]),)
        if return_cell:
            out += (cell.reshape(shape[:-1] + (3,)),)
        if return_noise:
            out += (noise.reshape(shape[:-1]),)
        return out[0] if len(out) == 1 else out

    def noise_fit(self, ports, fact=1.1, fn='exp_dc'):
        """Everything pp_channel_noise_fit measures of the rows of ports [..., nbin] (NumPy or a
        device tensor, f64 or f32): (noise, kc, cell) = get_noise_fit(row, fact), find_kc's cut-off
        and its winning grid cell (ia, ib, idc), shaped like ports without the bin axis."""
        _noise_method('fit', fn)
        src, dtype, on_dev, shape, keep = _array_arg(ports, "noise_fit: device rows")
        if len(shape) < 2:
            raise ValueError("ports must be [..., nbin]")
        nrows = int(np.prod(shape[:-1]))
        norms, noise = np.empty(nrows), np.empty(nrows)
        kc, cell = np.empty(nrows, dtype=np.int32), np.empty((nrows, 3), dtype=np.int32)
        _check(self._lib.pp_channel_noise_fit(self._ctx, src, dtype, on_dev, nrows, int(shape[-1]), _lib.PP_NOISEFIT_ROWS,
                                              _lib.PP_KC_FNS[fn], float(fact), _lib.PP_NORMS[None], None, _dp(norms),
                                              _dp(noise), kc.ctypes.data_as(c_int32_p), cell.ctypes.data_as(c_int32_p)),
               "pp_channel_noise_fit")
        return noise.reshape(shape[:-1]), kc.reshape(shape[:-1]), cell.reshape(shape[:-1] + (3,))

    # host bytes of f64 rows _prof_norms holds at a time (and as many again for their mean profiles)
    PROF_RUN_BYTES = 256 << 20

    def _prof_norms(self, ports, weights):
        """normalize_portrait's 'prof' norms (pplib.py:2478-2495): each portrait's mean
        profile over its channels of non-zero sum, weighted, on the host as np.average
        forms it; then fit_phase_shift(row, mean_prof).scale of every non-zero row on the
        device (brute grid + the reference's simplex finish).  Zero rows get 1.  Runs of
        whole portraits of at most PROF_RUN_BYTES go through the host at a time (a device
        tensor's run is copied over); a row's norm does not depend on its run."""
        dev = _is_device_array(ports)
        shape = tuple(int(v) for v in ports.shape)
        nchan, nbin = (shape[1], shape[2]) if len(shape) == 3 else (shape[0], shape[1])
        nsub = shape[0] if len(shape) == 3 else 1
        view = ports.reshape(nsub, nchan, nbin)
        w = np.ones((nsub, nchan)) if weights is None else \
            np.asarray(weights, dtype=np.float64).reshape(nsub, nchan)
        div = np.ones((nsub, nchan))
        run = max(1, self.PROF_RUN_BYTES // (nchan * nbin * 8))
        for s0 in range(0, nsub, run):
            part = view[s0:s0 + run]
            a = np.asarray(part.detach().cpu().numpy() if dev else part, dtype=np.float64)
            n = len(a)
            rows = a.reshape(n * nchan, nbin)
            live = rows.any(axis=1)
            if not live.any():
                continue
            means = np.empty((n, nbin))
            for i in range(n):
                good = np.where(a[i].sum(axis=1) != 0.0)[0]
                means[i] = np.average(a[i][good], axis=0, weights=w[s0 + i][good])
            sub_of = np.repeat(np.arange(n), nchan)[live]
            div[s0:s0 + n].reshape(-1)[live] = \
                self.fit_phase_shift_batch(rows[live], means[sub_of], finish='simplex')[:, 2]
        return div.reshape(-1)

    def channel_snrs(self, ports, fudge=3.25, method='PS', fact=1.1, fn='exp_dc'):
        """pplib.get_SNR (pplib.py:2289-2308) of every row of ports [..., nbin] (NumPy or a
        device tensor, f64 or f32): the row's sum, maximum and noise come from one pass over
        it on the device.  method: the noise estimator, 'PS' (the power spectrum's top
        quarter) or 'fit' (get_noise_fit with find_kc(fn=fn), as channel_noise).  Returns an
        array shaped like ports without the bin axis."""
        _noise_method(method, fn)
        src, dtype, on_dev, shape, keep = _array_arg(ports, "channel_snrs: device rows")
        if len(shape) < 2:
            raise ValueError("ports must be [..., nbin]")
        nrows = int(np.prod(shape[:-1]))
        snrs = np.empty(nrows)
        if method == 'PS':
            _check(self._lib.pp_channel_snrs(self._ctx, src, dtype, on_dev, nrows, shape[-1], float(fudge),
                                             _dp(snrs)), "pp_channel_snrs")
        else:
            _check(self._lib.pp_channel_snrs_fit(self._ctx, src, dtype, on_dev, nrows, shape[-1], _lib.PP_KC_FNS[fn],
                                                 float(fact), float(fudge), _dp(snrs)), "pp_channel_snrs_fit")
        return snrs.reshape(shape[:-1])

    # eigenvectors find_significant_eigvec examines (check_max = 10, pplib.py:1584)
    PCA_NVEC = 10

    def pca_gram(self, port, weights):
        """First stage of pplib.pca (pplib.py:1497-1528) for port [nchan,nbin] (NumPy or a
        device tensor, f64 or f32) and the PCA weights [nchan]: returns (mean_prof [nbin],
        gram, fact).  gram is np.cov(delta.T, aweights=weights, ddof=1) itself when nchan >=
        nbin, else its nchan x nchan dual sqrt(w_i w_j) delta_i . delta_j / fact, which has the
        same non-zero eigenvalues; fact is np.cov's normalisation.  Formed on the f64 MFMA in a
        fixed order (the same bits on every run).  The centred rows stay on the device for
        pca_basis and pca_project."""
        src, dtype, on_dev, shape, keep = _array_arg(port, "pca_gram: device rows")
        if len(shape) != 2:
            raise ValueError("port must be [nchan,nbin]")
        nchan, nbin = shape
        w = _f64(weights, (nchan,))
        sumw = float(np.sum(w))
        fact = sumw - float(np.sum(w * w)) / sumw
        n = nchan if nchan < nbin else nbin
        mean_prof, gram = np.empty(nbin), np.empty((n, n))
        self._pca_shape = None
        _check(self._lib.pp_pca_gram(self._ctx, src, dtype, on_dev, nchan, nbin, _dp(w), sumw, fact,
                                     _dp(mean_prof), _dp(gram)), "pp_pca_gram")
        self._pca_shape = (nchan, nbin)
        return mean_prof, gram, fact

    def pca_basis(self, vecs, eigval):
        """The leading eigenvectors of pca_gram's matrix (vecs [n,nvec], columns, with their
        eigenvalues, descending) as profiles: returns (eigvec [nbin,nvec], stats [nvec,4]).
        On the dual side each is mapped back through the resident rows.  stats holds what
        find_significant_eigvec (pplib.py:1586-1595) measures of every vector without
        smoothing: sum_{k>=1} |rfft(ev)_k|^2, get_noise(ev), max |ev| and
        count_crossings(|ev|, 0.1 max |ev|)."""
        v = np.ascontiguousarray(np.asarray(vecs, dtype=np.float64).T)
        nvec = v.shape[0]
        lam = _f64(eigval, (nvec,))
        if self._pca_shape is None:
            raise EngineError("pca_basis: no centred portrait is resident (pca_gram first)")
        basis = np.empty((nvec, self._pca_shape[1]))
        stats = np.empty((nvec, 4))
        _check(self._lib.pp_pca_basis(self._ctx, _dp(v), _dp(lam), nvec, _dp(basis), _dp(stats)),
               "pp_pca_basis")
        return np.ascontiguousarray(basis.T), stats

    def pca_project(self, ieig):
        """proj_port [nchan,ncomp] = delta . eigvec[:, ieig] and reconst_port [nchan,nbin] =
        proj_port . eigvec[:, ieig].T + mean_prof (ppspline.py:126-129) of the resident rows
        and basis."""
        if self._pca_shape is None:
            raise EngineError("pca_project: no centred portrait is resident (pca_gram first)")
        nchan, nbin = self._pca_shape
        idx = np.ascontiguousarray(ieig, dtype=np.int32)
        proj, reconst = np.empty((nchan, len(idx))), np.empty((nchan, nbin))
        _check(self._lib.pp_pca_project(self._ctx, idx.ctypes.data_as(c_int32_p), len(idx), _dp(proj),
                                        _dp(reconst)), "pp_pca_project")
        return proj, reconst

    # ---- wavelet smoothing (pplib.wavelet_smooth / smart_smooth, pplib.py:1621-1761) ----
    THRESHTYPES = {"hard": 0, "soft": 1}

    def _smooth_args(self, rows, threshtype, what):
        if threshtype not in self.THRESHTYPES:
            raise ValueError("threshtype must be 'hard' or 'soft'")
        src, dtype, on_dev, shape, keep = _array_arg(rows, what + ": device rows")
        if len(shape) != 2:
            raise ValueError("rows must be [nrows,nbin]")
        if on_dev:
            import torch
            out = torch.empty(shape, dtype=torch.float64, device=rows.device)
            dst = C.c_void_p(out.data_ptr())
        else:
            out = np.empty(shape)
            dst = C.c_void_p(out.ctypes.data)
        return src, dtype, on_dev, shape, keep, out, dst

    def wavelet_smooth(self, rows, nlevel=5, threshtype="hard", fact=1.0):
        """pplib.wavelet_smooth (pplib.py:1621-1666) of every row of rows [nrows,nbin] (NumPy or a device
        tensor, f64 or f32) with the db8 wavelet: stationary wavelet transform to nlevel levels, the threshold
        fact * median(|cA_L u cD_L|) / 0.6745 * sqrt(2 ln nbin) on every coefficient, inverse transform.  nlevel
        and fact: one value, or one per row.  nbin even, 16 ... 4096, a multiple of 2^nlevel.  Returns f64 rows,
        on the device when the input is."""
        from . import wavelets
        src, dtype, on_dev, shape, keep, out, dst = self._smooth_args(rows, threshtype, "wavelet_smooth")
        nrows, nbin = shape
        lv = np.ascontiguousarray(np.atleast_1d(nlevel), dtype=np.int32)
        fc = np.ascontiguousarray(np.atleast_1d(fact), dtype=np.float64).reshape(-1)
        for name, a in (("nlevel", lv), ("fact", fc)):
            if a.size not in (1, nrows):
                raise ValueError("%s: one value or one per row" % name)
        h = wavelets.rec_lo()
        _check(self._lib.pp_wavelet_smooth(self._ctx, src, dtype, on_dev, nrows, nbin, _dp(h),
                                           self.THRESHTYPES[threshtype], lv.ctypes.data_as(c_int32_p),
                                           0 if lv.size == 1 else 1, _dp(fc), 0 if fc.size == 1 else 1, dst),
               "pp_wavelet_smooth")
        return out

    def smart_smooth(self, rows, try_nlevels, rchi2_tol=0.1, threshtype="hard"):
        """pplib.smart_smooth (pplib.py:1668-1735) of every row of rows [nrows,nbin] (even nbin, 16 ... 4096, a
        multiple of 2^try_nlevels): per level 1 ... try_nlevels the brute search over 30 factors with its simplex
        finish, the best level, the final smooth, zeroed when its reduced chi^2 is further than rchi2_tol from 1.
        Returns (smoothed rows, info) with info a dict of per-row arrays: level (0 for a row of zeros), fact,
        snr (-fun), red_chi2, nfev, stats [nrows,4] (pca_basis's statistics of the smoothed row) and raw_noise
        (get_noise of the row itself)."""
        from . import wavelets
        src, dtype, on_dev, shape, keep, out, dst = self._smooth_args(rows, threshtype, "smart_smooth")
        nrows, nbin = shape
        info, stats, noise = np.empty((nrows, 5)), np.empty((nrows, 4)), np.empty(nrows)
        h = wavelets.rec_lo()
        _check(self._lib.pp_smart_smooth(self._ctx, src, dtype, on_dev, nrows, nbin, _dp(h),
                                         self.THRESHTYPES[threshtype], int(try_nlevels), float(rchi2_tol), dst,
                                         _dp(info), _dp(stats), _dp(noise)), "pp_smart_smooth")
        return out, dict(level=info[:, 0].astype(int), fact=info[:, 1].copy(), snr=info[:, 2].copy(),
                         red_chi2=info[:, 3].copy(), nfev=info[:, 4].astype(int), stats=stats, raw_noise=noise)

    def zap_median(self, noise, good, nstd):
        """get_zap_channels' clip (ppzap.py:18-47) of every subint at once: noise and
        good [nsub,nchan] (good != 0: a channel in ok_ichans).  Returns the uint8
        [nsub,nchan] mask of the channels it zaps."""
        nz = _f64(np.atleast_2d(noise))
        nsub, nchan = nz.shape
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(good) != 0, (nsub, nchan)), dtype=np.uint8)
        zap = np.empty((nsub, nchan), dtype=np.uint8)
        _check(self._lib.pp_zap_median(self._ctx, _dp(nz), g.ctypes.data_as(c_uint8_p), nsub, nchan, float(nstd),
                                       zap.ctypes.data_as(c_uint8_p)), "pp_zap_median")
        return zap

    # limits of the Gaussian-component fit's entry points (pp_gaussfit.h)
    GAUSS_FIT_MAX_SETS = 100
    GAUSS_FIT_MAX_GAUSS = 16

    def gauss_fit_begin(self, data, freqs, errs):
        """Make the data portrait data[nchan,nbin] (NumPy or a device tensor, f64 or f32; the good
        channels only), its frequencies and 1 / errs[nchan] resident for a Gaussian-component fit
        (fit_gaussian_portrait, pplib.py:1924-2052); gauss_fit_end releases them."""
        self._gauss_shape = None
        self._gauss_njoin = 0
        src, dtype, on_dev, shape, keep = _array_arg(data, "gauss_fit_begin: device data")
        if len(shape) != 2:
            raise ValueError("data must be [nchan,nbin]")
        nchan, nbin = shape
        freqs, errs = _f64(freqs, (nchan,)), _f64(errs, (nchan,))
        _check(self._lib.pp_gauss_fit_begin(self._ctx, src, dtype, on_dev, nchan, nbin, _dp(freqs), _dp(errs)),
               "pp_gauss_fit_begin")
        self._gauss_shape = (nchan, nbin)
        del keep

    def gauss_fit_end(self):
        self._gauss_shape = None
        self._gauss_njoin = 0
        _check(self._lib.pp_gauss_fit_end(self._ctx), "pp_gauss_fit_end")

    GAUSS_FIT_MAX_JOIN = 16

    def gauss_fit_join(self, band_of_chan, P, njoin=None):
        """Make the open fit a joined one (gen_gaussian_portrait's join_ichans, pplib.py:923-929):
        band_of_chan[nchan] is the band of every resident channel, 0 .. njoin - 1 (njoin None: its
        largest entry + 1), or -1 for a channel in no band; P [s] turns the bands' Delta-DMs into
        rotations.  gauss_residuals then takes the bands' (phase, Delta-DM) as `join`."""
        if self._gauss_shape is None:
            raise EngineError("gauss_fit_join: no fit is open (gauss_fit_begin first)")
        band = np.ascontiguousarray(band_of_chan, dtype=np.intc).reshape(-1)
        if band.shape != (self._gauss_shape[0],):
            raise ValueError("band_of_chan must hold one entry per resident channel")
        njoin = (int(band.max()) + 1 if len(band) else 0) if njoin is None else int(njoin)
        _check(self._lib.pp_gauss_fit_join(self._ctx, njoin, band.ctypes.data_as(C.POINTER(C.c_int)), float(P)),
               "pp_gauss_fit_join")
        self._gauss_njoin = njoin

    def gauss_residuals(self, code, nu_ref, dc, tau_rot, alpha, comps, fetch=False, join=None):
        """The weighted residual rows (data - model(set s)) / errs of nsets parameter sets against
        the resident portrait, left on the device for gauss_normal: dc, tau_rot [rot at nu_ref],
        alpha [nsets] and comps [nsets,ngauss,6] = loc, m_loc, wid, m_wid, amp, m_amp
        (fit_gaussian_portrait_function, pplib.py:1230-1242).  fetch=True returns them as
        [nsets,nchan,nbin].  join [nsets,njoin,2] = (phase [rot], Delta-DM) of every set and band
        of a joined fit (gauss_fit_join first); None there means no rotation."""
        comps = np.ascontiguousarray(comps, dtype=np.float64)
        if comps.ndim != 3 or comps.shape[2] != 6:
            raise ValueError("comps must be [nsets,ngauss,6]")
        nsets, ngauss = comps.shape[:2]
        dc, tau_rot, alpha = (_f64(v, (nsets,)) for v in (dc, tau_rot, alpha))
        if join is not None:
            join = np.ascontiguousarray(join, dtype=np.float64)
            if join.ndim != 3 or join.shape[0] != nsets or join.shape[2] != 2:
                raise ValueError("join must be [nsets,njoin,2]")
            if self._gauss_njoin and join.shape[1] != self._gauss_njoin:
                raise ValueError("join holds %d bands, the resident band map %d" % (join.shape[1], self._gauss_njoin))
        out = None
        if fetch:
            if self._gauss_shape is None:
                raise EngineError("gauss_residuals: no data portrait is resident (gauss_fit_begin first)")
            out = np.empty((nsets,) + self._gauss_shape)
        _check(self._lib.pp_gauss_residuals(self._ctx, str(code).encode(), float(nu_ref), nsets, _dp(dc),
                                            _dp(tau_rot), _dp(alpha), ngauss, _dp(comps), _dp(out), _dp(join)),
               "pp_gauss_residuals")
        return out

    def gauss_normal(self, h, rows=None, nsets=None, nrow=None):
        """(chi2, g, G) of a forward-difference step from the residual rows R[nsets,nrow]: with
        D_a = (R_{a+1} - R_0) / h[a], chi2 = sum R_0^2, g = D R_0, G = D D^T.  rows None: the rows
        the last gauss_residuals left on the device (nsets = len(h) + 1 of the resident shape);
        else rows [nsets,nrow], NumPy or a device f64 tensor.  Summed in a fixed order: the same
        call returns the same bits."""
        h = np.zeros(0) if h is None else np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
        src, on_dev, keep = None, 0, None
        if rows is not None:
            src, dtype, on_dev, shape, keep = _array_arg(rows, "gauss_normal: device rows")
            if dtype != PP_F64 or len(shape) != 2:
                raise ValueError("rows must be float64 [nsets,nrow]")
            nsets, nrow = shape
        else:
            nsets = len(h) + 1 if nsets is None else int(nsets)
            if nrow is None:
                if self._gauss_shape is None:
                    raise EngineError("gauss_normal: no resident residual rows (gauss_residuals first)")
                nrow = self._gauss_shape[0] * self._gauss_shape[1]
        if len(h) != nsets - 1:
            raise ValueError("h must hold nsets - 1 steps")
        K = nsets - 1
        chi2, g, G = np.empty(1), np.empty(K), np.empty((K, K))
        _check(self._lib.pp_gauss_normal(self._ctx, src, on_dev, int(nsets), int(nrow), _dp(h) if K else None,
                                         _dp(chi2), _dp(g) if K else None, _dp(G) if K else None),
               "pp_gauss_normal")
        del keep
        return float(chi2[0]), g, G

    def synth_portraits(self, dst, freqs, P, inj, sigma, seed, first_subint=0,
                        slot=0, gains=None):
        """Fill a CUDA tensor dst[nsub,nchan,nbin] with synthetic subints; gains[nsub,nchan]
        (optional) scales the template in every channel (scintillation)."""
        if not _is_device_array(dst):
            raise EngineError("synth_portraits needs a CUDA tensor destination")
        nsub = int(dst.shape[0])
        freqs = _f64(freqs)
        P = _f64(P, (nsub,))
        inj = _f64(inj, (nsub, 3))
        gains = _f64(gains, (nsub, int(dst.shape[1])))
        _check(self._lib.pp_synth_portraits(
            self._ctx, int(slot), C.c_void_p(dst.data_ptr()),
            PP_F64 if dst.element_size() == 8 else PP_F32, nsub, _dp(freqs),
            _dp(P), _dp(inj), _dp(gains), float(sigma), C.c_uint64(int(seed)),
            C.c_int64(int(first_subint))), "pp_synth_portraits")

    def model_shape(self, slot=0):
        """(nchan, nbin) of the template in `slot`."""
        nchan, nbin = C.c_int(0), C.c_int(0)
        _check(self._lib.pp_model_shape(self._ctx, int(slot), C.byref(nchan), C.byref(nbin)), "pp_model_shape")
        return nchan.value, nbin.value

    def fake_portraits(self, dst, delays, amps=None, sigmas=None, seed=0, first_subint=0, slot=0):
        """Fill a CUDA tensor dst[nsub,npol,nchan,nbin] (or [nsub,nchan,nbin]: npol = 1), f32 or f64, with
        simulated subints of the template in `slot`: amps[i,p,n] x the template delayed by delays[i,n]
        rotations (positive = later) + sigmas[n] x unit normal noise keyed on (seed, first_subint + i, p, n,
        bin).  amps [nsub,npol,nchan] (None: 1) and sigmas [nchan] (None: 0) are host arrays."""
        if not _is_device_array(dst):
            raise EngineError("fake_portraits needs a CUDA tensor destination")
        shape = tuple(int(s) for s in dst.shape)
        if len(shape) == 3:
            shape = (shape[0], 1) + shape[1:]
        if len(shape) != 4 or min(shape) < 1:
            raise EngineError("fake_portraits: dst must be [nsub,npol,nchan,nbin] or [nsub,nchan,nbin], not %s" %
                              (tuple(dst.shape),))
        nsub, npol, nchan, nbin = shape
        if (nchan, nbin) != self.model_shape(slot):
            raise EngineError("fake_portraits: dst holds %d x %d rows, the template in slot %d is %d x %d" %
                              ((nchan, nbin, int(slot)) + self.model_shape(slot)))
        if dst.element_size() not in (4, 8) or not dst.is_floating_point() or not dst.is_contiguous():
            raise EngineError("fake_portraits: dst must be a contiguous float32 or float64 tensor")
        if delays is None:
            raise EngineError("fake_portraits: delays is None")
        delays = _f64(delays, (nsub, nchan))
        amps = _f64(amps, (nsub, npol, nchan))
        sigmas = _f64(sigmas, (nchan,))
        _check(self._lib.pp_fake_portraits(
            self._ctx, int(slot), C.c_void_p(dst.data_ptr()), PP_F64 if dst.element_size() == 8 else PP_F32,
            nsub, npol, _dp(delays), _dp(amps), _dp(sigmas), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
            C.c_int64(int(first_subint))), "pp_fake_portraits")

    def scrunch(self, ports, weights, t_off=None, f_off=None, pol_mode="keep"):
        """Weighted sums over contiguous groups of subints and channels (what load_data hands to
        PSRCHIVE's tscrunch / pscrunch / fscrunch, pplib.py:2692, :2709, :2713) of ports[nsub,npol,nchan,nbin]
        (or [nsub,nchan,nbin]: one polarisation; NumPy or a device tensor, f32 or f64):
        out[gt,p',gf] = sum of weights[s,c] * ports[s,p,c] over the group's members / wout[gt,gf],
        wout = the members' summed weight.  t_off / f_off: group offsets, ascending from 0 to nsub /
        nchan (None: every subint / channel on its own).  pol_mode: 'keep', 'sum01' (Coherence ->
        Intensity) or 'first' (Stokes -> Intensity).  A weight of 0 or NaN skips the row unread; a
        cell without positive total weight is zero.  Returns (out, wout): out is f64, a device tensor
        when ports was one, with the polarisation axis ports had; wout is a NumPy array.  The sum runs
        in ascending (s, c) order in f64: its bits do not depend on how the call is cut up."""
        if pol_mode not in _lib.PP_POL:
            raise ValueError("pol_mode must be one of 'keep', 'sum01', 'first'")
        src, dtype, on_dev, shape, keep = _array_arg(ports, "scrunch: device ports")
        three = len(shape) == 3
        if three:
            shape = (shape[0], 1) + tuple(shape[1:])
        if len(shape) != 4:
            raise ValueError("ports must be [nsub,npol,nchan,nbin] or [nsub,nchan,nbin]")
        nsub, npol, nchan, nbin = (int(v) for v in shape)
        w = _f64(weights, (nsub, nchan))
        t_off = np.ascontiguousarray(np.arange(nsub + 1) if t_off is None else t_off, dtype=np.int32)
        f_off = np.ascontiguousarray(np.arange(nchan + 1) if f_off is None else f_off, dtype=np.int32)
        if t_off.ndim != 1 or f_off.ndim != 1 or len(t_off) < 2 or len(f_off) < 2:
            raise ValueError("t_off and f_off must be 1-D offset arrays")
        ngt, ngf = len(t_off) - 1, len(f_off) - 1
        oshape = (ngt, npol if pol_mode == "keep" else 1, ngf, nbin)
        if three:
            oshape = (ngt, ngf, nbin)
        if on_dev:
            import torch
            out = torch.empty(oshape, dtype=torch.float64, device=ports.device)
            dst = C.c_void_p(out.data_ptr())
        else:
            out = np.empty(oshape)
            dst = C.c_void_p(out.ctypes.data)
        wout = np.empty((ngt, ngf))
        _check(self._lib.pp_scrunch(self._ctx, src, dtype, on_dev, nsub, npol, nchan, nbin, _dp(w), ngt,
                                    t_off.ctypes.data_as(c_int32_p), ngf, f_off.ctypes.data_as(c_int32_p),
                                    _lib.PP_POL[pol_mode], dst, _dp(wout)), "pp_scrunch")
        del keep
        return out, wout

    def kernel_times(self, reset=False):
        n = 32
        names = (C.c_char_p * n)()
        secs = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        k = self._lib.pp_kernel_times(self._ctx, n, names, secs, cnt)
        out = {names[i].decode(): (secs[i], cnt[i]) for i in range(k)}
        if reset:
            self._lib.pp_kernel_times_reset(self._ctx)
        return out


_default = {}


def default_engine(device=0):
    """Process-wide engine for the reference-shaped single-call API."""
    eng = _default.get(device)
    if eng is None:
        eng = _default[device] = Engine(device)
    return eng


_WHILE_PENDING = ("poll", "wait", "close")      # what may be called while a submitted batch runs
_WHILE_QUEUED = ("enqueue", "fit_batch", "collect", "close", "set_option", "get_option", "options", "profiled",
                 "kernel_times", "synchronize")


def _fresh_waits(fn):
    import functools

    @functools.wraps(fn)
    def call(self, *args, **kwargs):
        # a submitted batch owns the context (its buffers, stream and counters) until wait():
        # include/pp_toas.h forbids every other call meanwhile -- enforce it here
        if self._pending is not None and fn.__name__ not in _WHILE_PENDING:
            raise EngineError("a submitted batch is pending on this engine: wait() before %s()" % fn.__name__)
        if self._queue and fn.__name__ not in _WHILE_QUEUED:
            raise EngineError("enqueued batches are pending on this engine: collect() before %s()" % fn.__name__)
        _new_call()
        return fn(self, *args, **kwargs)
    return call


# every entry point that may be handed device arrays starts a new round of producer waits
for _name in [n for n, f in vars(Engine).items() if callable(f) and not n.startswith("_")]:
    setattr(Engine, _name, _fresh_waits(getattr(Engine, _name)))

