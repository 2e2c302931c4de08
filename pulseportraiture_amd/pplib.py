"""Reference-shaped entry points of pplib that sit on the wideband-TOA path.

Mirrors (same names, argument meaning, result fields) of the reference's
pplib.py for: module settings (:45-83), RCSTRINGS (:111-119), DataBunch
(:125-136), fit_phase_shift (:2054-2100), the legacy fit_portrait (:2102-2204),
and the small host-side helpers the callers use between fits
(get_bin_centers :671-684, DM_delay :2577-2590, phase_transform :2592-2616,
guess_fit_freq :2618-2632), and the two Gaussian-component fits of ppgauss
(fit_gaussian_profile :1842-1922, fit_gaussian_portrait :1924-2052; their driver
is pulseportraiture_amd.gaussfit).  All array arithmetic of the fits themselves
runs in HIP kernels through pulseportraiture_amd.engine.
"""
import sys

import numpy as np


def default_engine(device=0):
    """engine.default_engine.  The engine (and with it the HIP library) is loaded by the first call that needs a
    device, not by importing this module: DataBunch and the host helpers here stand below modules that never touch
    one."""
    from .engine import default_engine as engine_default
    return engine_default(device)


# ---- settings (pplib.py:45-83); Dconst must be bit-identical ---------------
Dconst_exact = 4.148808e3
Dconst_trad = 0.000241 ** -1
Dconst = Dconst_trad
scattering_alpha = -4.0
use_get_noise = True
default_noise_method = 'PS'
F0_fact = 0
wid_max = 0.25
default_model = '000'
binshift = 1.0

# return-code strings (pplib.py:111-119); the device solver reports
# 0 gradient-converged, 1 iteration limit, 2 stalled at rounding (the
# reference's usual trust-ncg exit), 3 NaN/singular
RCSTRINGS = {'-1': 'INFEASIBLE: Infeasible (low > up).',
             '0': 'LOCALMINIMUM: Local minima reach (|pg| ~= 0).',
             '1': 'FCONVERGED: Converged (|f_n-f_(n-1)| ~= 0.)',
             '2': 'XCONVERGED: Converged (|x_n-x_(n-1)| ~= 0.)',
             '3': 'MAXFUN: Max. number of function evaluations reach.',
             '4': 'LSFAIL: Linear search failed.',
             '5': 'CONSTANT: All lower bounds are equal to the upper bounds.',
             '6': 'NOPROGRESS: Unable to progress.',
             '7': 'USERABORT: User requested end of minimization.'}


class DataBunch(dict):
    """dict whose attributes are its keys; results stay mutable attribute-dicts
    because callers modify them after the fit (pplib.py:125-136)."""

    def __init__(self, **kwds):
        dict.__init__(self, kwds)
        self.__dict__ = self


class DataPortrait(object):
    """Holder of the data a model is fit to, built FROM ARRAYS.

    The reference's DataPortrait (pplib.py:138-650) loads PSRCHIVE archives and
    carries joining / normalising / plotting methods.  `data` is a DataBunch with the
    load_data fields (see pulseportraiture_amd.pptoas.data_from_arrays) and gives the
    reference's single-archive field layout (pplib.py:306-327): every key of the
    DataBunch as an attribute, plus port, portx, freqsxs, noise_stdsxs, SNRsxs.  A list
    of DataBunches, one per band, stands for the reference's metafile (pplib.py:163-299):
    the bands' first subints are concatenated and sorted by frequency, and the "join"
    attributes say which channels came from which band and how the bands are to be
    aligned -- a phase offset and a Delta-DM each, fitted along with a Gaussian model
    (ppgauss).  joinfile: a file like the one write_join_parameters writes, with
    parameters to start from; metafile=name: what such a list is called (datafile)."""

    def __init__(self, data=None, joinfile=None, quiet=False, **kwargs):
        self.init_params = []
        self.joinfile = joinfile
        if isinstance(data, (list, tuple)) and len(data) and all(isinstance(d, dict) for d in data):
            self._init_joined(list(data), kwargs.get("metafile"))
            return
        if data is None or not isinstance(data, dict):
            raise RuntimeError("DataPortrait needs a DataBunch built from arrays, or a list of them "
                               "(PSRFITS loading requires PSRCHIVE)")
        self.njoin = 0
        self.join_params = []
        self.join_ichans = []
        self.all_join_params = []
        self.datafile = data.get("filename", "arrays")
        self.datafiles = [self.datafile]
        self.data = data
        for key in data.keys():
            setattr(self, key, data[key])
        if getattr(self, "source", None) is None:
            self.source = "noname"
        self.port = (self.masks * self.subints)[0, 0]
        self.portx = self.port[self.ok_ichans[0]]
        self.freqsxs = [self.freqs[0, self.ok_ichans[0]]]
        if self.noise_stds is not None:
            self.noise_stdsxs = np.asarray(self.noise_stds)[0, 0, self.ok_ichans[0]]
        self.SNRsxs = np.asarray(self.SNRs)[0, 0, self.ok_ichans[0]]
        if data.get("flux_prof") is not None:
            self.flux_profx = data["flux_prof"][self.ok_ichans[0]]

    def _init_joined(self, bunches, metafile=None):
        """The metafile branch (pplib.py:163-299): band 1 is the phase reference (phase fixed
        at 0, Delta-DM free), every other band starts at minus its profile's shift against band
        1's and has both free.  metafile: the name the list of bands goes by (datafile)."""
        self.datafiles = [str(d.get("filename", "arrays")) for d in bunches]
        self.metafile = self.datafile = metafile or "metafile"
        self.njoin = len(bunches)
        join_params, join_fit_flags = [], []
        self.join_nchans, self.join_nchanxs = [0], [0]
        self.join_ichans, self.join_ichanxs = [], []
        self.nchan = self.nchanx = 0
        self.lofreq, self.hifreq = np.inf, 0.0
        Ps, refprof = 0.0, None
        cat = dict((k, []) for k in ("freqs", "freqsxs", "masks", "port", "portx", "flux_prof", "flux_profx", "noise_stds",
                                     "noise_stdsxs", "SNRs", "SNRsxs", "weights", "weightsxs"))
        for ifile, data in enumerate(bunches):
            name = self.datafiles[ifile]
            if data["nsub"] != 1:
                raise ValueError("%s: a band of a joined fit holds one subint, not %d" % (name, data["nsub"]))
            if data.get("noise_stds") is None:
                raise ValueError("%s: a band of a joined fit needs its noise_stds" % name)
            ok = np.asarray(data["ok_ichans"][0], dtype=int)
            sub = np.asarray(data["subints"], dtype=np.float64)[0, 0]
            mask = np.asarray(data["masks"], dtype=np.float64)[0, 0] * np.ones(sub.shape)
            weights = np.asarray(data["weights"], dtype=np.float64)[0]
            prof = data.get("prof")
            if prof is None:
                prof = np.average(sub[ok], axis=0, weights=weights[ok])
            if ifile == 0:
                self.nbin, self.phases = data["nbin"], data["phases"]
                refprof = prof
                self.source = data.get("source") or "noname"
                join_params += [0.0, 0.0]
                join_fit_flags += [0, 1]
            else:
                if data["nbin"] != self.nbin:
                    raise ValueError("%s: %d bins, %s has %d" % (name, data["nbin"], self.datafiles[0], self.nbin))
                join_params += [-fit_phase_shift(prof, refprof, Ns=self.nbin).phase, 0.0]
                join_fit_flags += [1, 1]
            self.nchan += data["nchan"]
            self.nchanx += len(ok)
            self.join_nchans.append(self.nchan)
            self.join_nchanxs.append(self.nchanx)
            freqs = np.asarray(data["freqs"], dtype=np.float64)
            Ps += np.mean(data["Ps"])
            self.lofreq = min(self.lofreq, freqs.min() - abs(data["bw"]) / (2 * data["nchan"]))
            self.hifreq = max(self.hifreq, freqs.max() + abs(data["bw"]) / (2 * data["nchan"]))
            flux_prof = data.get("flux_prof")
            if flux_prof is None or not len(flux_prof):
                flux_prof = sub.mean(axis=1)
            noise, snrs = np.asarray(data["noise_stds"])[0, 0], np.asarray(data["SNRs"])[0, 0]
            # (port is the masked data, portx the good channels' own)
            for key, keyx, full, good in (("freqs", "freqsxs", freqs[0], freqs[0]), ("port", "portx", sub * mask, sub),
                                          ("flux_prof", "flux_profx", flux_prof, flux_prof),
                                          ("noise_stds", "noise_stdsxs", noise, noise), ("SNRs", "SNRsxs", snrs, snrs),
                                          ("weights", "weightsxs", weights, weights)):
                cat[key].extend(np.asarray(full))
                cat[keyx].extend(np.asarray(good)[ok])
            cat["masks"].extend(mask)
        self.Ps = [Ps / len(bunches)]
        self.bw = self.hifreq - self.lofreq
        freqs, freqsxs = np.array(cat["freqs"]), np.array(cat["freqsxs"])
        self.nu0 = freqs.mean()
        self.isort, self.isortx = np.argsort(freqs), np.argsort(freqsxs)
        for ijoin in range(self.njoin):
            self.join_ichans.append(np.where((self.isort >= self.join_nchans[ijoin]) &
                                             (self.isort < self.join_nchans[ijoin + 1]))[0])
            self.join_ichanxs.append(np.where((self.isortx >= self.join_nchanxs[ijoin]) &
                                              (self.isortx < self.join_nchanxs[ijoin + 1]))[0])
        self.masks = np.array([[np.array(cat["masks"])[self.isort]]])
        self.port = np.array(cat["port"])[self.isort]
        self.portx = np.array(cat["portx"])[self.isortx]
        self.flux_prof = np.array(cat["flux_prof"])[self.isort]
        self.flux_profx = np.array(cat["flux_profx"])[self.isortx]
        self.noise_stds = np.array([[np.array(cat["noise_stds"])[self.isort]]])
        self.noise_stdsxs = np.array(cat["noise_stdsxs"])[self.isortx]
        self.SNRs = np.array([[np.array(cat["SNRs"])[self.isort]]])
        self.SNRsxs = np.array(cat["SNRsxs"])[self.isortx]
        self.weights = np.array([np.array(cat["weights"])[self.isort]])
        self.weightsxs = np.array([np.array(cat["weightsxs"])[self.isortx]])
        self.freqs = np.array([freqs[self.isort]])
        self.freqsxs = [freqsxs[self.isortx]]
        self.ok_ichans = [np.flatnonzero(self.weights[0] > 0)]
        self.join_params = np.array(join_params, dtype=np.float64)
        self.join_fit_flags = np.array(join_fit_flags)
        if self.joinfile:
            self.read_joinfile()
        self.all_join_params = [self.join_ichanxs, self.join_params, self.join_fit_flags]
        if len(bunches) == 1:
            self.data = bunches[0]

    def read_joinfile(self):
        """Take the phases and Delta-DMs of the joinfile's last njoin lines (pplib.py:282-297):
        archive name, phase [, its error], DM [, its error] -- the four-column layout
        write_join_parameters writes, and the older one without errors."""
        with open(self.joinfile, "r") as fh:
            lines = [line.split() for line in fh.readlines()[-len(self.datafiles):]]
        try:
            for tok in lines:
                ijoin = self.datafiles.index(tok[0])
                phi = np.double(tok[1])
                DM = float(tok[3]) if len(tok) > 3 else float(tok[2])
                self.join_params[ijoin * 2] = phi
                self.join_params[ijoin * 2 + 1] = DM
        except (ValueError, IndexError):
            print("Bad join file.")

    def apply_joinfile(self, nu_ref, undo=False):
        """Rotate every band of port and portx by minus its join parameters about nu_ref [MHz], the
        fitted model's reference frequency (pplib.py:329-348); undo=True rotates the other way."""
        sign = (-1) ** int(undo)
        params = -np.asarray(self.join_params, dtype=np.float64) * sign
        self.port = self._rotate_bands(self.port, self.join_ichans, self.freqs[0], params, nu_ref)
        self.portx = self._rotate_bands(self.portx, self.join_ichanxs, self.freqsxs[0], params, nu_ref)

    def _rotate_bands(self, port, ichans, freqs, params, nu_ref):
        """port with the channels ichans[i] of every band i rotated by (params[2 i], params[2 i + 1])
        = (phase, DM) about nu_ref, on the device."""
        eng = getattr(self, "engine", None) or default_engine()
        out = np.array(port, dtype=np.float64)
        for ii, ic in enumerate(ichans):
            if len(ic):
                out[ic] = eng.rotate_portraits(out[ic][None], np.asarray(freqs)[ic], self.Ps[0], phi=params[2 * ii],
                                               DM=params[2 * ii + 1], nu_DM=nu_ref)[0]
        return out

    def format_join_parameters(self):
        """The text write_join_parameters appends (pplib.py:509-520)."""
        text = "# archive name" + " " * 32 + "-phase offset & err [rot]" + " " * 2 + "-delta-DM & err [cm**-3 pc]\n"
        for ifile, datafile in enumerate(self.datafiles):
            text += (datafile + " " * abs(45 - len(datafile)) + "% .10f" % self.join_params[ifile * 2] + " " +
                     "%.10f" % self.join_param_errs[::2][ifile] + "  " + "% .6f" % self.join_params[ifile * 2 + 1] + " " +
                     "%.6f" % self.join_param_errs[1::2][ifile] + "\n")
        return text

    def write_join_parameters(self):
        """Append the join parameters to the joinfile, or to <model_name>.join (pplib.py:486-521).
        NB, as in the reference: they are the "opposite" of how they rotate the data with e.g.
        rotate_data (use a negative), and the Delta-DMs are offsets, not Doppler corrected."""
        joinfile = self.joinfile if self.joinfile is not None else self.model_name + ".join"
        with open(joinfile, "a") as jf:
            jf.write(self.format_join_parameters())

    def smooth_portrait(self, smart=False, **kwargs):
        """Smooth the portrait data with wavelet_smooth's defaults, or with smart_smooth (smart=True, at most 8
        levels) -- pplib.py:400-424, with the reference's side effects: port, noise_stds[0,0], flux_prof, and
        portx, noise_stdsxs, flux_profx.  **kwargs go to wavelet_smooth / smart_smooth."""
        eng = kwargs.get("engine") or default_engine()
        if smart:
            kwargs = dict(kwargs, try_nlevels=min(8, int(np.log2(self.nbin))))

        def smooth(port):
            return np.asarray((smart_smooth if smart else wavelet_smooth)(port, **kwargs))
        # full portrait
        self.port = smooth(self.port)
        self.noise_stds[0, 0] = eng.channel_noise(self.port)[0]
        self.flux_prof = self.port.mean(axis=1)
        # condensed portrait
        self.portx = smooth(self.portx)
        self.noise_stdsxs = np.asarray(eng.channel_noise(self.portx)[0], dtype=np.float64)
        self.flux_profx = self.portx.mean(axis=1)


# ---- small host helpers ------------------------------------------------------
def get_bin_centers(nbin, lo=0.0, hi=1.0):
    lo, hi = np.double(lo), np.double(hi)
    diff = hi - lo
    return np.double(np.linspace(lo + diff / (nbin * 2), hi - diff / (nbin * 2),
                                 nbin))


def DM_delay(DM, freq, freq_ref=np.inf, P=None):
    delay = Dconst * DM * ((freq ** -2.0) - (freq_ref ** -2.0))
    return delay / P if P else delay


def phase_transform(phi, DM, nu_ref1=np.inf, nu_ref2=np.inf, P=None, mod=False):
    if P is None:
        P, mod = 1.0, False
    phi_prime = phi + (Dconst * DM * P ** -1 * (nu_ref2 ** -2.0 - nu_ref1 ** -2.0))
    if mod:
        phi_prime = np.where(abs(phi_prime) >= 0.5, phi_prime % 1, phi_prime)
        phi_prime = np.where(phi_prime >= 0.5, phi_prime - 1.0, phi_prime)
        if not phi_prime.shape:
            phi_prime = np.float64(phi_prime)
    return phi_prime


def guess_fit_freq(freqs, SNRs=None):
    freqs = np.asarray(freqs, dtype=np.float64)
    nu0 = (freqs.min() + freqs.max()) * 0.5
    if SNRs is None:
        SNRs = np.ones(len(freqs))
    diff = np.sum((freqs - nu0) * SNRs * freqs ** -2) / np.sum(SNRs * freqs ** -2)
    return nu0 + diff


# ---- Fourier rotation (device) ---------------------------------------------------
def rotate_data(data, phase=0.0, DM=0.0, Ps=None, freqs=None, nu_ref=np.inf):
    """Rotate and/or dedisperse a profile [nbin], portrait [nchan,nbin] or
    subint cube [nsub,npol,nchan,nbin]; positive phase / DM rotate to earlier
    phase (pplib.py:2338-2426).  Runs on the GPU."""
    data = np.asarray(data, dtype=np.float64)
    shape = data.shape
    if data.ndim == 1:
        cube = data[None, None]
    elif data.ndim == 2:
        cube = data[None]
    elif data.ndim == 4:
        cube = data.reshape(shape[0], shape[1] * shape[2], shape[3])
    else:
        print("Wrong number of dimensions.")
        return 0
    nsub, nch = cube.shape[0], cube.shape[1]
    if DM == 0.0 or freqs is None:
        fr, P, DM = np.full(nch, np.inf), np.ones(nsub), 0.0
    else:
        P = np.ones(nsub) * Ps
        fr = np.asarray(freqs, dtype=np.float64)
        if fr.ndim == 0:
            fr = np.full(shape[-2] if data.ndim > 1 else 1, float(fr))
        if data.ndim == 4:
            fr = np.broadcast_to(fr, (nsub, shape[2]))[:, None, :].repeat(shape[1], axis=1)
            fr = fr.reshape(nsub, nch)
    with np.errstate(divide='ignore'):
        out = default_engine().rotate_portraits(cube, fr, P, phi=phase, DM=DM, nu_DM=nu_ref)
    return out.reshape(shape)


def rotate_portrait(port, phase=0.0, DM=None, P=None, freqs=None, nu_ref=np.inf):
    """pplib.py:2428-2460."""
    if DM is None and freqs is None:
        return rotate_data(port, phase)
    return rotate_data(port, phase, DM, P, freqs, nu_ref)


def rotate_profile(profile, phase=0.0):
    return rotate_data(profile, phase)


# ---- 1-D FFTFIT ----------------------------------------------------------------
def weighted_mean(data, errs=1.0):
    """Weighted mean and its standard error, weights errs**-2 over the entries
    with errs > 0 (pplib.py:696-709)."""
    data = np.asarray(data, dtype=np.float64)
    if hasattr(errs, 'is_integer'):
        errs = np.ones(len(data))
    errs = np.asarray(errs, dtype=np.float64)
    ii = np.where(errs > 0.0)[0]
    w = errs[ii] ** -2.0
    return (data[ii] * w).sum() / w.sum(), w.sum() ** -0.5


def get_noise(data, method=default_noise_method, **kwargs):
    """Off-pulse noise of data, 1- or 2-D (get_noise, pplib.py:2206-2225).  method "PS" is the mean of the
    top 1/frac of the power spectrum (get_noise_PS; frac=4, chans=False); "fit" finds the harmonic where the
    noise floor starts (get_noise_fit; fact=1.1, chans=False), on the device.  **kwargs go to the selected
    function.  An unknown method prints and returns 0, as the reference."""
    if method == "PS":
        return get_noise_PS(data, **kwargs)
    if method == "fit":
        return get_noise_fit(data, **kwargs)
    print("Unknown get_noise method.")
    return 0


def get_noise_PS(data, frac=4, chans=False):
    """Off-pulse noise from the mean of the top 1/frac of the power spectrum (get_noise_PS,
    pplib.py:2227-2253).  Host helper for normalisation; inside a fit the engine measures the same quantity
    itself when errs is None."""
    a = np.asarray(data, dtype=np.float64)
    rows = a if chans else a.reshape(1, -1)
    power = np.abs(np.fft.rfft(rows, axis=-1)) ** 2.0 / rows.shape[-1]
    kc = int((1 - frac ** -1) * power.shape[-1])
    noise = np.sqrt(power[:, kc:].mean(axis=-1))
    return noise if chans else noise[0]


# points of one transform on the device (Engine.channel_noise: nbin <= 4096)
NOISE_FIT_MAX_POINTS = 4096


def get_noise_fit(data, fact=1.1, chans=False):
    """Off-pulse noise from the mean of the power spectrum above fact * find_kc(pows) (get_noise_fit,
    pplib.py:2255-2287), on the device (Engine.channel_noise(method='fit')).  data: 1-D, or 2-D with chans=True
    for one value per row.  2-D data with chans=False is the reference's transform of the ravelled nchan x nbin
    points: NotImplementedError beyond NOISE_FIT_MAX_POINTS points (and for an odd number of them).

    One departure: a row whose power above DC is nothing but the transform's rounding residue (a constant row).  At
    row lengths that are a power of two the device, like the reference, finds exact zeros there and takes kc = H - 1;
    at other lengths the reference's transform leaves exact zeros in some harmonics and the device's in none, so the
    fitted kc can differ.  The noise is 0 to 1e-12 of the row either way."""
    a = np.asarray(data)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    if chans:
        return default_engine().channel_noise(a.reshape(len(a), -1), method='fit', fact=fact)[0]
    flat = a.reshape(1, -1)
    if flat.shape[1] > NOISE_FIT_MAX_POINTS or flat.shape[1] % 2 or flat.shape[1] < 8:
        raise NotImplementedError(
            "get_noise_fit(chans=False) transforms the ravelled data as one row: %d points, and the device takes an "
            "even number from 8 to %d (chans=True measures every row)" % (flat.shape[1], NOISE_FIT_MAX_POINTS))
    return default_engine().channel_noise(flat, method='fit', fact=fact)[0][0]


def half_triangle_function(a, b, dc, N):
    """A half triangle of base floor(a) and height b on the baseline dc, N points (half_triangle_function,
    pplib.py:1436-1446): find_kc's 'half_tri' model, as a definition."""
    fn = np.zeros(N) + dc
    a = int(np.floor(a))
    fn[:a] += -(np.float64(b) / a) * np.arange(a) + b
    return fn


def find_kc_function(params, data, errs=1.0, fn='exp_dc'):
    """The (weighted) chi-squared of find_kc's model (a, b, dc) against data (find_kc_function,
    pplib.py:1448-1463): b exp(-a k) + dc for fn 'exp_dc', half_triangle_function for 'half_tri'.  The
    definition of what Engine.find_kc minimises over its grid, not a route around it."""
    a, b, dc = params[0], params[1], params[2]
    if fn == 'exp_dc':
        model = b * np.exp(-a * np.arange(len(data))) + dc
    elif fn == 'half_tri':
        model = half_triangle_function(a, b, dc, len(data))
    else:
        return 0.0
    return np.sum(((data - model) / errs) ** 2.0)


def find_kc(pows, errs=1.0, fn='exp_dc'):
    """The critical cut-off harmonic where the noise floor of the power spectrum pows (1-D) starts
    (find_kc, pplib.py:1465-1495), from the reference's 20 x 20 x 20 brute grid, searched on the device
    (Engine.find_kc).  A scalar errs scales every chi-squared alike and does not move the minimum; an array
    of errs is not supported.  An unknown fn returns 0, as the reference.  (Spectra are taken as given: a harmonic
    of exactly zero power gives kc = len(pows) - 1, as in the reference; whether a transform leaves exact zeros in
    harmonics that hold only rounding residue is the transform's business -- see get_noise_fit.)"""
    if np.ndim(errs) != 0:
        raise NotImplementedError("find_kc: errs must be a scalar (per-harmonic uncertainties are not supported)")
    if fn not in ('exp_dc', 'half_tri'):
        return 0
    pows = np.asarray(pows, dtype=np.float64)
    if pows.ndim != 1:
        raise ValueError("find_kc: pows is a 1-D power spectrum (Engine.find_kc takes rows of them)")
    return int(default_engine().find_kc(pows[None], fn=fn)[0])


# ---- wavelet smoothing -----------------------------------------------------------
def _as_rows(port):
    a = port if hasattr(port, "data_ptr") else np.asarray(port)
    one_prof = len(a.shape) == 1
    return (a.reshape(1, -1) if one_prof else a), one_prof


def wavelet_smooth(port, wavelet='db8', nlevel=5, threshtype='hard', fact=1.0, engine=None):
    """The wavelet-denoised version of a portrait [nchan,nbin] or a profile [nbin] (pplib.py:1621-1666),
    on the device (Engine.wavelet_smooth).  Only the 'db8' wavelet is built."""
    if getattr(wavelet, "name", wavelet) != 'db8':
        raise NotImplementedError("wavelet_smooth: only the 'db8' wavelet is available")
    rows, one_prof = _as_rows(port)
    out = (engine or default_engine()).wavelet_smooth(rows, nlevel=int(nlevel), threshtype=threshtype,
                                                      fact=float(np.asarray(fact).reshape(-1)[0]))
    return out[0] if one_prof else out


def smart_smooth(port, try_nlevels=None, rchi2_tol=0.1, return_info=False, engine=None, **kwargs):
    """wavelet_smooth applied the reference's automated way (pplib.py:1668-1735): per profile the level and
    threshold factor of the highest pseudo-S/N whose reduced chi^2 against the profile stays within rchi2_tol of
    1, on the device (Engine.smart_smooth).  try_nlevels = 0 and odd nbin return port as it is (a single profile of
    odd length as a one-row portrait, the reference's quirk); an even nbin
    that is no power of two gets one level; the default is log2(nbin) levels.  **kwargs as the reference reads
    them: threshtype is used, nlevel and fact are dropped, and a 'wavelet' key fails as it does there (it looks
    up kwargs['wave']).  return_info=True also returns Engine.smart_smooth's per-row dictionary (None where
    nothing ran)."""
    if try_nlevels == 0:
        return (port, None) if return_info else port
    rows, one_prof = _as_rows(port)
    nbin = int(rows.shape[-1])
    if nbin % 2 != 0:
        # (the reference has rebound a single profile to a one-row portrait by now, and returns that)
        port = np.array([port]) if one_prof else port
        return (port, None) if return_info else port
    elif np.modf(np.log2(nbin))[0] != 0.0:
        try_nlevels = 1
    elif try_nlevels is None:
        try_nlevels = int(np.log2(nbin))
    if 'wavelet' in kwargs:
        kwargs['wave']
    threshtype = kwargs.get('threshtype', 'hard')
    out, info = (engine or default_engine()).smart_smooth(rows, int(try_nlevels), rchi2_tol=rchi2_tol,
                                                         threshtype=threshtype)
    out = out[0] if one_prof else out
    return (out, info) if return_info else out


def find_significant_eigvec(eigvec, check_max=10, return_max=10, snr_cutoff=150.0, check_crossings=True,
                            check_acorr=True, return_smooth=True, engine=None, **kwargs):
    """Which eigenvectors (the columns of eigvec [nbin,ncomp]) are significant, from their smoothed versions
    and S/N (pplib.py:1555-1619): the signal and the crossings come from the smoothed vector, the noise from the
    vector itself.  All examined vectors are smoothed in one device call; smoothed vectors are not renormalised
    and only those found significant are returned in smooth_eigvec.  Returns ieig, or (ieig, smooth_eigvec)
    with return_smooth.  check_acorr cannot take effect (the reference's branch is unreachable); **kwargs go to
    smart_smooth."""
    from .ppspline import significant_eigvec
    eigvec = np.asarray(eigvec, dtype=np.float64)
    nbin = eigvec.shape[0]
    ncheck = min(max(check_max, return_max), eigvec.shape[1])
    rows = np.ascontiguousarray(eigvec.T[:ncheck])
    sm, info = smart_smooth(rows, return_info=True, engine=engine, **kwargs)
    stats = smooth_stats(rows, sm, info)
    ieig, _ = significant_eigvec(stats, nbin, check_max=check_max, return_max=return_max, snr_cutoff=snr_cutoff,
                                 check_crossings=check_crossings)
    if not return_smooth:
        return ieig
    smooth_eigvec = np.zeros(eigvec.shape)
    if len(ieig):
        smooth_eigvec[:, ieig] = np.asarray(sm)[ieig].T
    return ieig, smooth_eigvec


def smooth_stats(rows, smoothed, info):
    """find_significant_eigvec's numbers of smoothed vectors, shaped like Engine.pca_basis's stats: the power
    sum_{k>=1} |rfft|^2, max |.| and crossings of the SMOOTHED vector, the noise of the vector ITSELF.  With
    info None (nothing was smoothed: odd nbin or try_nlevels 0) everything is measured here on the host."""
    if info is not None:
        stats = np.array(info["stats"], dtype=np.float64)
        stats[:, 1] = info["raw_noise"]
        return stats
    stats = np.zeros((len(rows), 4))
    for i, (raw, ev) in enumerate(zip(np.asarray(rows), np.asarray(smoothed))):
        a = np.abs(ev)
        sg = np.sign(a - 0.1 * a.max())
        stats[i] = [np.sum(np.abs(np.fft.rfft(ev)[1:]) ** 2), get_noise(raw), a.max(),
                    np.sum(sg[1:] != sg[:-1]) - np.sum(sg == 0)]
    return stats


def gaussian_profile(nbin, loc, wid):
    """A Gaussian pulse of FWHM wid [rot] centred on phase loc, sampled at the nbin bin
    centres nearest to loc (wrapped), scaled so that the underlying curve peaks at 1
    (pplib.py:770-825); zeros for wid <= 0 and beyond 20 sigma."""
    out = np.zeros(int(nbin))
    if not wid > 0.0:
        return out
    sigma = wid / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    mean = loc % 1.0
    x = get_bin_centers(nbin)
    x = np.where(x > mean + 0.5, x - 1.0, x) if mean < 0.5 else np.where(x < mean - 0.5, x + 1.0, x)
    z = (x - mean) / sigma
    near = np.fabs(z) < 20.0
    out[near] = np.exp(-0.5 * z[near] ** 2.0) / (sigma * np.sqrt(2.0 * np.pi))
    if not out.any():
        return out
    ipk = out.argmax()
    return np.exp(-0.5 * ((x[ipk] - loc) / sigma) ** 2.0) / out[ipk] * out


def get_SNR(prof, fudge=3.25, noise_method=None):
    """Estimate of a profile's signal-to-noise ratio, baseline removed (pplib.py:2289-2308):
    sum / (noise sqrt(Weq)) / fudge with Weq = sum / max.  The profile's sum, maximum and
    noise are taken in one pass on the device (Engine.channel_snrs, which takes whole
    portraits).  noise_method: get_noise's method, 'PS' or 'fit' (None: archive's scope, else 'PS')."""
    from .archive import noise_kwargs
    return default_engine().channel_snrs(np.asarray(prof, dtype=np.float64)[None], fudge=fudge,
                                         **noise_kwargs(noise_method))[0]


def fit_phase_shift(data, model, noise=None, bounds=[-0.5, 0.5], Ns=100, finish='simplex'):
    """Fit a phase shift between a data and a model profile on the GPU (pplib.py:2054):
    Ns-point brute grid over `bounds` (both ends included), then -- like the
    reference, whose scipy.optimize.brute finishes with fmin -- the Nelder-Mead
    simplex to xtol = ftol = 1e-4, retraced step for step, so the returned phase is the
    reference's (~1e-5 rot from the optimum of the correlation).  finish='newton'
    returns the exact local optimum instead."""
    eng = default_engine()
    out = eng.fit_phase_shift_batch(np.asarray(data, dtype=np.float64)[None],
                                    np.asarray(model, dtype=np.float64)[None],
                                    noise=None if noise is None else [noise],
                                    bounds=bounds, Ns=Ns, finish=finish)[0]
    return DataBunch(phase=out[0], phase_err=out[1], scale=out[2],
                     scale_err=out[3], snr=out[4], red_chi2=out[5],
                     duration=out[6])


# ---- legacy 2-parameter fit ------------------------------------------------------
def fit_portrait(data, model, init_params, P, freqs, nu_fit=None, nu_out=None,
                 errs=None, bounds=[(None, None), (None, None)], id=None,
                 quiet=True):
    """(phase, DM) fit with the legacy result fields; runs the same device
    engine as fit_portrait_full with fit_flags = [1,1,0,0,0] (the reference's
    TNC minimiser is not reproduced: both converge to the same optimum)."""
    from .pptoaslib import fit_portrait_full
    x0 = [init_params[0], init_params[1], 0.0, 0.0, 0.0]
    r = fit_portrait_full(data, model, x0, P, freqs, [nu_fit] * 3, [nu_out] * 3,
                          errs, [1, 1, 0, 0, 0], log10_tau=False, sub_id=id, method='TNC',
                          is_toa=True, quiet=quiet)
    with np.errstate(divide='ignore', invalid='ignore'):
        scale_errs = np.abs(r.scales / r.channel_snrs)   # (p_n/sigma_n^2)^-1/2
    return DataBunch(phase=r.phi, phase_err=r.phi_err, DM=r.DM, DM_err=r.DM_err,
                     scales=r.scales, scale_errs=scale_errs, nu_ref=r.nu_DM,
                     covariance=r.covariance_matrix[0, 1], chi2=r.chi2,
                     red_chi2=r.red_chi2, snr=r.snr, duration=r.duration,
                     nfeval=r.nfeval, return_code=r.return_code)


# ---- Gaussian-component fits (ppgauss) ---------------------------------------------
def fit_gaussian_profile(data, init_params, errs, fit_flags=None, fit_scattering=False, quiet=True, **kwargs):
    """Fit Gaussian components to a profile (pplib.py:1842-1922): init_params = [DC, tau [bin],
    (loc, wid, amp) x ngauss].  Returns fitted_params, fit_errs, residuals, chi2, dof.  The
    residuals and the normal equations of every iteration are formed on the GPU."""
    from . import gaussfit
    return gaussfit.fit_gaussian_profile(data, init_params, errs, fit_flags, fit_scattering, quiet, **kwargs)


def fit_gaussian_portrait(model_code, data, init_params, scattering_index, errs, fit_flags, fit_scattering_index,
                          phases, freqs, nu_ref, join_params=[], P=None, quiet=True, **kwargs):
    """Fit evolving Gaussian components to a portrait (pplib.py:1924-2052): init_params = [DC,
    tau [bin], (loc, m_loc, wid, m_wid, amp, m_amp) x ngauss].  Returns fitted_params, fit_errs,
    scattering_index, scattering_index_err, chi2, dof.  join_params = [join_ichans, values, flags] with the period
    P makes it a joined multi-band fit (pplib.py:1992-2017).  The residuals and the normal equations of every iteration are formed on the GPU."""
    from . import gaussfit
    return gaussfit.fit_gaussian_portrait(model_code, data, init_params, scattering_index, errs, fit_flags,
                                          fit_scattering_index, phases, freqs, nu_ref, join_params, P, quiet, **kwargs)


# ---- simulated observations (make_fake_pulsar) ---------------------------------------
fake_chunk_subints = None     # subints generated on the device at once; None: sized from free HBM


def scattering_times(tau, alpha, freqs, nu_tau):
    """Scattering times over frequency: tau (nu / nu_tau)**alpha (pplib.py:4049-4053)."""
    return tau * (np.asarray(freqs, dtype=np.float64) / nu_tau) ** alpha


def scintillation_pattern(nchan, params):
    """The amplitude per channel add_scintillation multiplies a portrait by: a sum of squared sinusoids
    across the band, one for each (amp, cycles, phase) triplet of params (pplib.py:1162-1167)."""
    pattern = np.zeros(int(nchan))
    for isin in range(len(params) // 3):
        a, w, p = params[isin * 3:isin * 3 + 3]
        pattern += a * np.sin(np.linspace(0, w * np.pi, nchan) + p * np.pi) ** 2
    return pattern


def add_scintillation(port, params=None, random=True, nsin=2, amax=1.0, wmax=3.0):
    """Add fake scintillation to an nchan x nbin portrait (pplib.py:1146-1174): params are triplets of
    amplitude, cycles across the band and phase [cycles]; with params None and random, nsin triplets are
    drawn from uniform [0, amax], chi-squared with wmax degrees of freedom and uniform [0, 1] (NumPy's
    global generator, as in the reference)."""
    port = np.asarray(port)
    if params is None and random is False:
        return port
    if params is None:
        params = []
        for isin in range(nsin):
            params += [np.random.uniform(0, amax), np.random.chisquare(wmax), np.random.uniform(0, 1)]
    return np.transpose(np.transpose(port) * scintillation_pattern(len(port), params))


def _DM_nu_term(freqs, xs, Cs, nu_ref):
    """sum_j C_j (nu**x_j - nu_ref**x_j) per channel, Cs padded with ones as add_DM_nu pads them
    (pplib.py:2537-2542)."""
    xs = list(np.atleast_1d(xs))
    if not hasattr(Cs, "__iter__"):
        Cs = np.ones(len(xs))
    if len(Cs) < len(xs):
        Cs = list(Cs) + list(np.ones(len(xs) - len(Cs)))
    freqs = np.asarray(freqs, dtype=np.float64)
    term = np.zeros(freqs.shape)
    for C, x in zip(Cs, xs):
        term = term + C * (freqs ** x - np.float64(nu_ref) ** x)
    return term


def add_DM_nu(port, phase=0.0, DM=None, P=None, freqs=None, xs=[-2.0], Cs=[1.0], nu_ref=np.inf):
    """Rotate a portrait with a power-law DM(nu): rotate_portrait with the frequency term
    sum_j C_j (nu**x_j - nu_ref**x_j) in place of nu**-2 - nu_ref**-2 (pplib.py:2509-2546).  Host NumPy."""
    pFFT = np.fft.rfft(np.asarray(port, dtype=np.float64), axis=1)
    k = np.arange(pFFT.shape[1])
    if DM is None and freqs is None:
        phis = np.full(len(pFFT), phase, dtype=np.float64)
    else:
        phis = phase + Dconst * DM / P * _DM_nu_term(freqs, xs, Cs, nu_ref)
    return np.fft.irfft(pFFT * np.exp(2.0j * np.pi * np.outer(phis, k)), np.shape(port)[1], axis=1)


def fake_pulsar_tables(model, par, nsub=1, npol=1, nchan=512, nu0=1500.0, bw=800.0, tsub=300.0, phase=0.0,
                       dDM=0.0, start_MJD=None, noise_stds=1.0, scales=1.0, dedispersed=False, t_scat=0.0,
                       alpha=scattering_alpha, scint=False, xs=None, Cs=None, nu_DM=np.inf, rng=None):
    """Everything make_fake_pulsar works out on the host, in f64, before the device forms the portraits:
    a DataBunch of freqs [nchan], Ps [nsub], epochs (MJD), delays [nsub,nchan] (rotations, positive = later: phase,
    dDM and the DM(nu) law), disp_delays [nchan] (the ephemeris DM's delay about nu0 that a dispersed archive carries on
    top, zeros for a dedispersed one), amps [nsub,npol,nchan], sigmas [nchan], dmc and the parsed model with the
    scattering it is to carry.
    model: a parsed .gmodel (gmodel.parse_gmodel); par: a parfile.psr_par; rng: the generator of the
    scintillation draws."""
    from .archive import MJD
    chanwidth = bw / nchan
    lofreq = nu0 - (bw / 2)
    freqs = np.linspace(lofreq + (chanwidth / 2.0), lofreq + bw - (chanwidth / 2.0), nchan)

    def per_channel(v, what):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            return v * np.ones(nchan)
        if v.shape != (nchan,):
            raise ValueError("len(%s) != nchan" % what)
        return v.copy()
    sigmas = per_channel(noise_stds, "noise_stds")
    scales = per_channel(scales, "scales")
    P, DM = np.float64(par.P0), np.float64(par.DM)
    Ps = np.full(nsub, P)
    # epochs: seconds added to the start, subint centres (pplib.py:3310-3320)
    start = MJD(np.float64(par.PEPOCH)) if start_MJD is None else MJD(start_MJD)
    epochs = [start + MJD(0, (tsub / 2.0 + i * tsub) / 86400.0) for i in range(nsub)]
    # delays
    D = Dconst / P
    nu2 = freqs ** -2.0 - np.float64(nu0) ** -2.0
    if xs is None:
        delay = phase + D * dDM * nu2
    else:
        delay = phase_transform(phase, DM + dDM, nu0, nu_DM, P) + D * dDM * _DM_nu_term(freqs, xs, Cs, nu_DM)
    delays = np.tile(delay, (nsub, 1))
    # what PSRCHIVE's dededisperse() puts back, as a rotation of its own after the rows are made (see make_fake_pulsar)
    disp_delays = np.zeros(nchan) if dedispersed else D * DM * nu2
    # scattering rides in the model; the modelfile's own overrides t_scat (pplib.py:3351)
    model = dict(model)
    model["params"] = np.array(model["params"], dtype=np.float64)
    if t_scat and not model["params"][1]:
        model["params"][1] = t_scat * (model["nu_ref"] / np.float64(nu0)) ** alpha
        model["alpha"] = np.float64(alpha)
    # amplitudes: scales times the scintillation pattern, drawn once per (subint, polarisation)
    amps = np.empty((nsub, npol, nchan))
    for i in range(nsub):
        for ip in range(npol):
            if scint is False or scint is None:
                pattern = 1.0
            elif scint is True:
                if rng is None:
                    rng = np.random.default_rng()
                params = []
                for isin in range(3):
                    params += [rng.uniform(0, 1.0), rng.chisquare(5.0), rng.uniform(0, 1)]
                pattern = scintillation_pattern(nchan, params)
            else:
                pattern = scintillation_pattern(nchan, list(scint))
            amps[i, ip] = scales * pattern
    return DataBunch(freqs=freqs, Ps=Ps, epochs=epochs, delays=delays, disp_delays=disp_delays, amps=amps,
                     sigmas=sigmas, dmc=1 if dedispersed else 0, DM=DM, nu0=np.float64(nu0), model=model)


def _fake_chunk(eng, nsub, sub_bytes):
    """Subints generated on the device at once: fake_chunk_subints, or what fits half of the free HBM."""
    if fake_chunk_subints is not None:
        return max(1, min(int(nsub), int(fake_chunk_subints)))
    import torch
    free_b, _ = torch.cuda.mem_get_info(eng.device)
    return max(1, min(int(nsub), int(0.5 * free_b // max(sub_bytes, 1))))


def make_fake_pulsar(modelfile, ephemeris, outfile="fake_pulsar.npz", nsub=1, npol=1, nchan=512, nbin=2048,
                     nu0=1500.0, bw=800.0, tsub=300.0, phase=0.0, dDM=0.0, start_MJD=None, weights=None,
                     noise_stds=1.0, scales=1.0, dedispersed=False, t_scat=0.0, alpha=scattering_alpha,
                     scint=False, xs=None, Cs=None, nu_DM=np.inf, state="Stokes", telescope="GBT",
                     quiet=False, seed=None, dtype=np.float32, engine=None):
    """Generate fake pulsar data on the GPU and write them as an .npz archive (pplib.py:3183-3378).

    modelfile is the .gmodel file of the Gaussian-component model; ephemeris a .par file (parfile.psr_par:
    PSR or PSRJ, RAJ, DECJ, F0 or P0, PEPOCH, DM); outfile the .npz to write -- the fields of
    archive.data_from_arrays, which every command here reads -- or None.  nsub, npol, nchan, nbin, nu0 [MHz], bw
    [MHz], tsub [s] shape the data.  phase [rot] delays every subint, with respect to nu0; dDM [cm**-3 pc] is added
    to the ephemeris DM, about nu0.  start_MJD: an MJD, a float, or None for PEPOCH.  weights [nsub,nchan] are
    stored, the data are not zeroed.  noise_stds and scales: a float or one value per channel.  dedispersed=True
    stores the archive dedispersed (dmc = 1), else the ephemeris DM's delay about nu0 is in the data (dmc = 0):
    the finished rows are rotated once more on the device (Engine.rotate_portraits, the convention of
    pptoas._dededisperse), which is what PSRCHIVE's dededisperse() does to the reference's archive.  (One rotation by
    the summed delay is not the same thing: every inverse transform keeps the real part of the Nyquist harmonic only,
    and the two differ by up to 3e-3 of the peak for the example model at 64 bins.)  t_scat [s] at nu0 with index alpha scatters the data, unless
    the modelfile has a TAU of its own.  scint=True multiplies every (subint, polarisation) by a random pattern
    (add_scintillation's, nsin=3, amax=1, wmax=5); a list is its parameter triplets.  xs, Cs, nu_DM simulate a
    DM(nu) as add_DM_nu does.  seed seeds the scintillation draws (numpy.random.default_rng) and the device's
    noise; None draws one and prints it.  dtype: np.float32 or np.float64.  Returns the DataBunch.

    The portraits are formed on the device (Engine.fake_portraits): the model's spectrum, a host table of delays,
    amplitudes per (subint, polarisation, channel) and noise per channel; the polarisations are the same model
    with noise of their own, as in the reference.  Long observations are generated in chunks of subints; the
    archive's bits do not depend on the chunk size.

    Limits.  There is no predictor: every subint's period is 1 / F0, whatever F1 or binary parameters the
    ephemeris holds.  The .npz stores epochs as float days (about 0.6 us near MJD 57000); the DataBunch returned
    keeps day and fraction apart.

    Two departures from the reference as it stands.  (1) With xs None the reference passes the unrotated model
    on (its line 3342) and silently drops phase and dDM; here they are honoured, delay = phase + Dconst dDM
    (nu**-2 - nu0**-2) / P, which is what its docstring describes and its example relies on.  (2) With xs given
    the reference overwrites `phase` by phase_transform(...) inside its loop over subints and polarisations, so the
    transform compounds; here it is applied once to the caller's phase."""
    from . import parfile
    from .archive import data_from_arrays, write_archive
    from .gmodel import read_gmodel
    import torch
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float32 or float64")
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0] >> np.uint64(1))
        if not quiet:
            print("seed = %d" % seed)
    seed = int(seed)
    par = parfile.psr_par(ephemeris)
    t = fake_pulsar_tables(read_gmodel(modelfile), par, nsub=nsub, npol=npol, nchan=nchan, nu0=nu0, bw=bw, tsub=tsub,
                           phase=phase, dDM=dDM, start_MJD=start_MJD, noise_stds=noise_stds, scales=scales,
                           dedispersed=dedispersed, t_scat=t_scat, alpha=alpha, scint=scint, xs=xs, Cs=Cs,
                           nu_DM=nu_DM, rng=np.random.default_rng(seed))
    weights = np.ones([nsub, nchan]) if weights is None else np.asarray(weights, dtype=np.float64)
    if weights.shape != (nsub, nchan):
        raise ValueError("weights must be nsub x nchan")
    eng = engine or default_engine()
    slot = 0
    eng.set_model_gaussian(t.model, t.freqs, nbin, P=t.Ps[0], slot=slot)
    subints = np.empty((nsub, npol, nchan, nbin), dtype=dtype)
    chunk = _fake_chunk(eng, nsub, npol * nchan * nbin * dtype.itemsize)
    dev = torch.empty((chunk, npol, nchan, nbin), dtype=torch.float32 if dtype.itemsize == 4 else torch.float64,
                      device="cuda:%d" % eng.device)
    for s0 in range(0, nsub, chunk):
        n = min(chunk, nsub - s0)
        eng.fake_portraits(dev[:n], t.delays[s0:s0 + n], amps=t.amps[s0:s0 + n], sigmas=t.sigmas, seed=seed,
                           first_subint=s0, slot=slot)
        if not t.dmc:
            # PSRCHIVE's dededisperse(): the finished rows, noise and all, delayed by the ephemeris DM about nu0
            eng.rotate_portraits(dev[:n].view(n * npol, nchan, nbin), t.freqs, t.Ps[0], DM=-float(t.DM), nu_DM=float(nu0))
        subints[s0:s0 + n] = dev[:n].cpu().numpy()
    del dev
    fields = dict(subints=subints, freqs=np.tile(t.freqs, (nsub, 1)), Ps=t.Ps, weights=weights, DM=float(t.DM),
                  dmc=int(t.dmc), doppler_factors=np.ones(nsub), telescope=str(telescope), bw=float(bw),
                  nu0=float(nu0), subtimes=np.full(nsub, float(tsub)), source=str(par.PSR))
    if outfile is not None:
        write_archive(outfile, dict(fields, epochs=t.epochs))
        if not quiet:
            print("\nUnloaded %s.\n" % outfile)
    data = data_from_arrays(epochs=t.epochs, filename="arrays" if outfile is None else str(outfile), **fields)
    data.state = "Intensity" if npol == 1 else state
    data.seed = seed
    return data


def load_data(filename, state=None, dedisperse=False, dededisperse=False, tscrunch=False, pscrunch=False,
              fscrunch=False, rm_baseline=False, flux_prof=False, refresh_arch=True, return_arch=True, quiet=False,
              engine=None, noise_method=None):
    """Load an .npz archive (or take a DataBunch) and apply the operations the reference's load_data hands to
    PSRCHIVE, in its order (pplib.py:2650-2814): state, dedisperse / dededisperse, tscrunch, pscrunch, fscrunch --
    pulseportraiture_amd.scrunch, on the device.  Returns the DataBunch with the reference's fields; prof, prof_noise,
    prof_SNR and (flux_prof=True) flux_prof come from the dedispersed, fully scrunched total intensity, prof_SNR
    being the archive's own where it stores one.  arch is None: there is no PSRCHIVE archive behind an .npz.

    Departures.  rm_baseline defaults to False and True raises NotImplementedError: an .npz holds what PSRCHIVE
    returned after remove_baseline, and the fit ignores the DC term.  state conversions other than to 'Intensity'
    raise.  refresh_arch and return_arch have nothing to act on.

    noise_method ('PS' or 'fit'; the reference's default_noise_method constant): given, noise_stds and SNRs are measured
    anew with it -- stored values too -- here and after every scrunch; None keeps stored values and measures the rest
    from the power spectrum."""
    from .archive import noise_method_scope
    with noise_method_scope(noise_method):
        return _load_data(filename, state, dedisperse, dededisperse, tscrunch, pscrunch, fscrunch, rm_baseline,
                          flux_prof, quiet, engine)


def _load_data(filename, state, dedisperse, dededisperse, tscrunch, pscrunch, fscrunch, rm_baseline, flux_prof, quiet,
               engine):
    from . import scrunch as sc
    from .archive import load_archive, noise_method_in_force
    if rm_baseline:
        raise NotImplementedError("load_data(rm_baseline=True): baseline removal is PSRCHIVE's; an .npz archive holds "
                                  "the data it returned after remove_baseline")
    eng = engine or default_engine()
    if isinstance(filename, dict):
        data = DataBunch(**{k: v for k, v in filename.items()})
        data.setdefault("filename", "arrays")
        if data.get("noise_stds") is None or data.get("SNRs") is None or noise_method_in_force() is not None:
            sc.measured(eng, data)      # (S/N 0 for a dead row, as in the scrunched bunches that follow)
    else:
        data, _ = load_archive(filename, eng)
    if not quiet:
        print("\nReading data from %s on source %s..." % (data.filename, data.source))
    data.state = sc.state_of(data)
    if state is not None and state != data.state:
        if state != "Intensity":
            raise NotImplementedError("load_data(state='%s') from '%s': only the conversion to 'Intensity' is built"
                                      % (state, data.state))
        pscrunch = True
    if dedisperse:
        data = sc.dedisperse(data, engine=eng)
    if dededisperse:
        data = sc.dededisperse(data, engine=eng)
    if tscrunch:
        data = sc.tscrunch(data, engine=eng)
    if pscrunch:
        data = sc.pscrunch(data, engine=eng)
    if fscrunch:
        data = sc.fscrunch(data, engine=eng)
    # the pulse profile: total intensity, dedispersed, scrunched over subints and channels
    total = sc.tscrunch(sc.dedisperse(sc.pscrunch(data, engine=eng), engine=eng), engine=eng)
    if flux_prof:
        fp = total.subints[0, 0].mean(axis=-1)
        data.flux_prof = np.asarray(fp.cpu().numpy() if hasattr(fp, "is_cuda") else fp, dtype=np.float64)
    else:
        data.flux_prof = np.array([])
    total = sc.fscrunch(total, engine=eng)
    prof = total.subints[0, 0, 0]
    data.prof = np.asarray(prof.cpu().numpy() if hasattr(prof, "is_cuda") else prof, dtype=np.float64)
    data.prof_noise = float(total.noise_stds[0, 0, 0])
    own = data.get("prof_SNR")
    data.prof_SNR = float(own) if own is not None else float(total.SNRs[0, 0, 0])
    data.arch = None
    if not quiet:
        nchanx = np.array([len(ich) for ich in data.ok_ichans]).mean()
        print("\tP [ms]             = %.3f\n\
        DM [cm**-3 pc]     = %.6f\n\
        center freq. [MHz] = %.4f\n\
        bandwidth [MHz]    = %.1f\n\
        # bins in prof     = %d\n\
        # channels         = %d\n\
        # chan (mean)      = %d\n\
        # subints          = %d\n\
        # unzapped subint  = %d\n\
        pol'n state        = %s\n" % (data.Ps[0] * 1000.0, data.DM, data.nu0, data.bw, data.nbin, data.nchan, nchanx,
                                      data.nsub, len(data.ok_isubs), data.state))
    return data
