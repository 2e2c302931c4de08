"""Reference-shaped wideband TOA driver: `GetTOAs` / `TOA` (pptoas.py:31-743).

`GetTOAs.get_TOAs` keeps the reference's arguments and result attributes but
replaces the per-subint Python loop (pptoas.py:344-489) by ONE batched device
call per archive: all good subints go to the engine as a [nsub, nchan, nbin]
batch with a channel mask (the per-subint ok_ichans), the phase seed
(pptoas.py:421-457) and the fit run in HIP kernels, and the TOA bookkeeping
(pptoas.py:528-721) is done here on the host.

PSRFITS I/O needs PSRCHIVE, which is outside this package: `datafiles` are
`DataBunch` objects with the fields of the reference's `load_data`
(pplib.py:2803-2813) -- see `data_from_arrays` -- or `.npz` files holding them
(pulseportraiture_amd.archive, which reads and writes them).
"""
import sys
import time

import numpy as np

from . import gmodel, scrunch
from .archive import (MJD, data_from_arrays, good_channel_counts, load_bunch,  # noqa: F401  (the first two: public here)
                      noise_method_in_force)
from .engine import EngineNotSupported, default_engine
from .pplib import DataBunch, Dconst, get_noise, guess_fit_freq, phase_transform, scattering_alpha, weighted_mean

max_nfile = 999
rm_baseline = True


class TOA(object):
    """TOA attributes bundled together (pptoas.py:31-73)."""

    def __init__(self, archive, frequency, MJD, TOA_error, telescope,
                 telescope_code, DM=None, DM_error=None, flags={}):
        self.archive = archive
        self.frequency = frequency
        self.MJD = MJD
        self.TOA_error = TOA_error
        self.telescope = telescope
        self.telescope_code = telescope_code
        self.DM = DM
        self.DM_error = DM_error
        self.flags = flags
        for flag in flags.keys():
            setattr(self, flag, flags[flag])

    def write_TOA(self, inf_is_zero=True, outfile=None):
        write_TOAs(self, inf_is_zero=inf_is_zero, outfile=outfile, append=True)


def toa_string(toa, inf_is_zero=True):
    """One loosely IPTA-formatted TOA line (pplib.py:3465-3497)."""
    freq = 0.0 if (toa.frequency == np.inf and inf_is_zero) else toa.frequency
    s = "%s %.8f %d" % (toa.archive, freq, toa.MJD.intday()) + \
        ("%.15f   %.3f  %s" % (toa.MJD.fracday(), toa.TOA_error,
                               toa.telescope_code))[1:]
    if toa.DM is not None:
        s += " -pp_dm %.7f" % toa.DM
    if toa.DM_error is not None:
        s += " -pp_dme %.7f" % toa.DM_error
    for flag, value in toa.flags.items():
        if value is None:
            continue
        if hasattr(value, "lower"):
            s += " -%s %s" % (flag, value)
        elif 'int' in str(type(value)):
            s += " -%s %d" % (flag, value)
        elif flag.find("_cov") >= 0:
            s += " -%s %.1e" % (flag, value)
        elif flag.find("phs") >= 0:
            s += " -%s %.8f" % (flag, value)
        elif flag.find("flux") >= 0:
            s += " -%s %.5f" % (flag, value)
        else:
            s += " -%s %.3f" % (flag, value)
    return s


def write_TOAs(TOAs, inf_is_zero=True, SNR_cutoff=0.0, outfile=None, append=True):
    """Write TOAs to file or stdout (pplib.py:3445-3503); TOAs below the S/N
    cutoff (or without an snr flag) are skipped like filter_TOAs does."""
    toas = TOAs if hasattr(TOAs, "__len__") else [TOAs]
    toas = [t for t in toas if hasattr(t, "snr") and t.snr >= SNR_cutoff]
    lines = [toa_string(t, inf_is_zero) for t in toas]
    if outfile is not None:
        with open(outfile, 'a' if append else 'w') as of:
            for line in lines:
                of.write(line + "\n")
    else:
        for line in lines:
            print(line)


def _unscattered(mdl):
    """A copy of a parsed .gmodel with its scattering time set to zero."""
    mdl = dict(mdl)
    mdl["params"] = mdl["params"].copy()
    mdl["params"][1] = 0.0
    return mdl


def _dededisperse(eng, port, d, ok_isubs):
    """A DataBunch flagged dmc (stored dedispersed) is put back to its dispersed
    state before fitting, as the reference does by re-loading the archive with
    dededisperse=True (pptoas.py:256-265): every channel is delayed again by the
    stored DM relative to the centre frequency (what PSRCHIVE's dedisperse() took
    out).  Runs on the device (rotate_portraits)."""
    if not d.dmc:
        return port
    isubs = np.asarray(ok_isubs, dtype=int)
    return eng.rotate_portraits(port, d.freqs[isubs], d.Ps[isubs], DM=-float(d.DM),
                                nu_DM=float(d.nu0))


def _to_device_once(eng, port):
    """Host portraits as a device tensor when they fit comfortably in free HBM (so that
    two engine calls do not both pay the H->D copy); unchanged otherwise."""
    try:
        import torch
    except ImportError:
        return port
    if torch.is_tensor(port) or not torch.cuda.is_available():
        return port
    a = np.asarray(port)
    try:
        free_b, _ = torch.cuda.mem_get_info(eng.device)
        if a.nbytes * 2.5 > free_b:
            return port
        return torch.as_tensor(np.ascontiguousarray(a), device="cuda:%d" % eng.device)
    except RuntimeError:
        return port


def _noise_rows(d, isubs):
    """noise_stds[isubs, 0] of a DataBunch, measured from the power spectrum
    (pplib.get_noise, what load_data stores: pplib.py:2727-2731) when the bunch was
    built without them."""
    isubs = np.asarray(isubs, dtype=int)
    if d.noise_stds is not None:
        return np.ascontiguousarray(np.asarray(d.noise_stds)[isubs, 0], dtype=np.float64)
    sub = np.asarray(d.subints)
    return np.array([get_noise(sub[i, 0], method=noise_method_in_force() or "PS", chans=True) for i in isubs],
                    dtype=np.float64)


def _take_subints(subints, ok_isubs):
    """[nok, nchan, nbin] total-intensity portraits of the good subints, without
    copying the archive when they are a contiguous run (fancy indexing would copy
    gigabytes before the H2D transfer even starts)."""
    idx = np.asarray(ok_isubs, dtype=int)
    if hasattr(subints, "is_cuda"):
        # (a device tensor -- an archive scrunched on the device -- stays there)
        return subints[idx.tolist(), 0].contiguous()
    a = np.asarray(subints)
    if len(idx) and np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))):
        return np.ascontiguousarray(a[idx[0]:idx[0] + len(idx), 0])
    return np.ascontiguousarray(a[idx, 0])


def _load_or_skip(datafile, quiet):
    """(DataBunch, name) of an archive, or None for one get_TOAs skips: it cannot be
    loaded, or it has no subint to fit."""
    try:
        data, fname = load_bunch(datafile)
    except RuntimeError as err:
        if not quiet:
            print("Cannot load_data(%s).  Skipping it." % datafile)
            print(err)
        return None
    if not len(data.ok_isubs):
        if not quiet:
            print("No subints to fit for %s.  Skipping it." % fname)
        return None
    return data, fname


def _tscrunched(eng, d, on_device=True):
    """The archive scrunched to one subint on the device (scrunch.tscrunch): what the reference gets from
    load_data(tscrunch=True) (pptoas.py:256-265).  on_device: host subints go to the device first where they fit, and
    the scrunched tensor stays there for the fit."""
    if on_device:
        d = DataBunch(**{k: v for k, v in d.items()})
        d.subints = _to_device_once(eng, d.subints)
    return scrunch.tscrunch(d, engine=eng)


def subint_fit_flags(nchans, fit_flags, carry=None):
    """The fit flags of a run of good subints with `nchans` good channels each, as the
    reference sets them (pptoas.py:475-486): a one-channel subint is fitted for phase
    only; a two-channel subint under fit_DM and fit_GM takes the list LEFT OVER from the
    subint before it (`carry`, across archives too) with GM dropped -- the flags asked
    for with GM dropped when there is none (the first subint of a call, where the
    reference raises NameError).  Returns (list of flag tuples, carry-out)."""
    out = []
    for n in nchans:
        if n == 1:
            fl = [1, 0, 0, 0, 0]
        elif n == 2 and fit_flags[1] and fit_flags[2]:
            # (right after a one-channel subint the left-over list is [1,0,0,0,0] and the
            # two-channel subint is fitted for phase only; after a normal one it becomes phase + DM)
            fl = list(carry) if carry is not None else list(fit_flags)
            fl[2] = 0
        else:
            fl = list(fit_flags)
        carry = fl
        out.append(tuple(fl))
    return out, carry


def deltadm_mean(DMs, DM_errs, DM0, ok_isubs):
    """Weighted mean DM offset of an archive and its error (pptoas.py:665-682)."""
    DeltaDMs = DMs - DM0
    if np.all(DM_errs[ok_isubs]):
        DM_weights = DM_errs[ok_isubs] ** -2
    else:
        DM_weights = np.ones(len(ok_isubs))
    DeltaDM_mean, DeltaDM_var = np.average(DeltaDMs[ok_isubs], weights=DM_weights,
                                           returned=True)
    DeltaDM_var = DeltaDM_var ** -1
    if len(ok_isubs) > 1:
        DeltaDM_var *= np.sum(((DeltaDMs[ok_isubs] - DeltaDM_mean) ** 2) *
                              DM_weights) / (len(ok_isubs) - 1)
    return DeltaDM_mean, DeltaDM_var ** 0.5


def shard_plan(n_archives, rank, world):
    """What a rank of a sharded get_TOAs walks: ("archives", lo, hi) -- a contiguous
    block of whole archives -- when there are at least as many archives as ranks, else
    ("subints", 0, n_archives): every archive, fitting shard_subints of each."""
    from .dist import shard_range
    if n_archives >= world:
        return ("archives",) + shard_range(n_archives, rank, world)
    return ("subints", 0, n_archives)


def shard_subints(mode, nok, rank, world):
    """[j0, j1) of an archive's `nok` good subints that a rank fits under `mode`."""
    from .dist import shard_range
    return (0, nok) if mode == "archives" else shard_range(nok, rank, world)


def _process_group():
    try:
        import torch.distributed as tdist
    except ImportError:
        tdist = None
    if tdist is None or not (tdist.is_available() and tdist.is_initialized()):
        raise ValueError("get_TOAs(distributed=True) needs an initialised torch.distributed "
                         "process group")
    return tdist.get_rank(), tdist.get_world_size()


def _archive_meta(d, fname, DM0):
    """The per-archive entries of the result lists that do not come from the fit."""
    return dict(fname=fname, obs=DataBunch(telescope=d.telescope, backend=d.backend, frontend=d.frontend),
                doppler_fs=d.doppler_factors, nu0=d.nu0, ok_isubs=np.asarray(d.ok_isubs, dtype=int),
                epochs=d.epochs, MJDs=np.array([e.in_days() for e in d.epochs], dtype=np.double),
                Ps=d.Ps, DM0=d.DM if DM0 is None else DM0)


# the result lists that hold one per-subint array (or list) per archive, filled by the bookkeeping
_ARCHIVE_ARRAYS = ("nu_fits", "nu_refs", "phis", "phi_errs", "TOAs", "TOA_errs", "DMs", "DM_errs", "GMs",
                   "GM_errs", "taus", "tau_errs", "alphas", "alpha_errs", "scales", "scale_errs", "snrs",
                   "channel_snrs", "profile_fluxes", "profile_flux_errs", "fluxes", "flux_errs", "flux_freqs",
                   "covariances", "red_chi2s", "nfevals", "rcs")


# the result lists that take the field of _archive_meta of the same name, wideband and narrowband alike, and
# those get_narrowband_TOAs fills with one [nsub, nchan] array per archive
_ARCHIVE_META = ("obs", "doppler_fs", "ok_isubs", "epochs", "MJDs", "Ps")
def narrowband_tau_guesses(freqs, P, nbin, log10_tau, scat_guess=None, model_tau=None, model_nu_ref=None,
                           alpha=None):
    """The scattering-time guess of every channel of a narrowband scattering fit [rot, or
    log10 rot under log10_tau] (pptoas.py:938-962, with the channel's own frequency where
    the reference's sketch names an undefined nu_fit_tau): scat_guess = (tau [s], its
    frequency [MHz], alpha) scaled to the channel, else the Gaussian model's tau [s] scaled
    from its reference frequency with `alpha`, else 0.  Under log10_tau a guess of 0
    becomes 1 / nbin."""
    freqs = np.asarray(freqs, dtype=np.float64)
    if scat_guess is not None:
        tau_s, nu_ref, alpha = scat_guess
        tau = (tau_s / P) * (freqs / nu_ref) ** alpha
    elif model_tau is not None:
        tau = (model_tau / P) * (freqs / model_nu_ref) ** (scattering_alpha if alpha is None else alpha)
    else:
        tau = np.zeros(len(freqs))
    if log10_tau:
        tau = np.log10(np.where(tau == 0.0, 1.0 / nbin, tau))
    return tau


def narrowband_scat_flags(tau, tau_err, phi_tau_cov, P, doppler_factor, log10_tau):
    """The TOA flags of a narrowband scattering fit (pptoas.py:1046-1060; the Doppler
    factor in both branches -- the reference leaves it undefined in the linear one):
    the scattering time in microseconds in the barycentric frame and its error."""
    df = doppler_factor
    if log10_tau:
        flags = {'scat_time': 10 ** tau * P / df * 1e6, 'log10_scat_time': tau + np.log10(P / df),
                 'log10_scat_time_err': tau_err}
    else:
        flags = {'scat_time': tau * P / df * 1e6, 'scat_time_err': tau_err * P / df * 1e6}
    flags['phi_tau_cov'] = phi_tau_cov
    return flags


_NARROWBAND_ARRAYS = ("phis", "phi_errs", "TOAs", "TOA_errs", "taus", "tau_errs", "scales", "scale_errs",
                      "channel_snrs", "profile_fluxes", "profile_flux_errs", "covariances", "channel_red_chi2s",
                      "nfevals", "rcs")


def merge_blocks(blocks):
    """One archive rebuilt from the blocks of the ranks that fitted its subints (in rank
    order, i.e. subint order): each block carries its subints' rows of the per-subint
    arrays.  Returns (arrays, TOAs, summed fit duration, meta)."""
    meta, nsub = blocks[0]["meta"], blocks[0]["nsub"]
    arrays = {}
    for name, v in blocks[0]["arrays"].items():
        if isinstance(v, list):
            full = list(np.zeros([nsub, 3]))
            for b in blocks:
                for i, row in zip(b["rows"], b["arrays"][name]):
                    full[i] = row
        else:
            full = np.zeros((nsub,) + v.shape[1:], dtype=v.dtype)
            for b in blocks:
                full[b["rows"]] = b["arrays"][name]
        arrays[name] = full
    toas = [t for b in blocks for t in b["toas"]]
    return arrays, toas, sum(b["fit_duration"] for b in blocks), meta


def toa_flags(d, isub, fl, p, e, cov, GM_out, df, nu_ref_tau, snr, gof, tmplt, opt, flux=None):
    """The flags of one wideband TOA (pptoas.py:607-657) of subint `isub` of the DataBunch `d`, fitted
    under the flags `fl`: p, e = its parameters and their errors, cov = the covariance of the fitted
    ones, GM_out = the GM as reported, df = the Doppler factor applied, nu_ref_tau = the scattering
    reference frequency, flux = (flux, flux_err, flux_ref_freq) under opt.print_flux.

    The statements stand in the reference's order ON PURPOSE: a dict lists its keys in the order
    they were first set, and that is the order toa_string writes the flags of a .tim line in."""
    nchan, nbin, P = d.nchan, d.nbin, d.Ps[isub]
    freqsx = d.freqs[isub, np.asarray(d.ok_ichans[isub], dtype=int)]
    flags = {}
    if fl[2]:
        flags['gm'] = GM_out
        flags['gm_err'] = e[2]
    if fl[3]:
        if opt.log10_tau:
            flags['scat_time'] = 10 ** p[3] * P / df * 1e6
            flags['log10_scat_time'] = p[3] + np.log10(P / df)
            flags['log10_scat_time_err'] = e[3]
        else:
            flags['scat_time'] = p[3] * P / df * 1e6
            flags['scat_time_err'] = e[3] * P / df * 1e6
        flags['scat_ref_freq'] = nu_ref_tau * df
        flags['scat_ind'] = p[4]
    if fl[4]:
        flags['scat_ind_err'] = e[4]
    flags['be'] = d.backend
    flags['fe'] = d.frontend
    flags['f'] = d.frontend + "_" + d.backend
    flags['nbin'] = int(nbin)
    flags['nch'] = int(nchan)
    flags['nchx'] = int(len(freqsx))
    flags['bw'] = freqsx.max() - freqsx.min()
    flags['chbw'] = abs(d.bw) / nchan
    flags['subint'] = int(isub)
    flags['tobs'] = d.subtimes[isub]
    flags['fratio'] = freqsx.max() / freqsx.min()
    flags['tmplt'] = tmplt
    flags['snr'] = snr
    if opt.nu_refs is not None and fl[0] and fl[1]:
        flags['phi_DM_cov'] = cov[0, 1]
    flags['gof'] = gof
    if opt.print_phase:
        flags['phs'] = p[0]
        flags['phs_err'] = e[0]
    if opt.print_flux:
        flags['flux'] = flux[0]
        flags['flux_err'] = flux[1]
        flags['flux_ref_freq'] = flux[2]
    if opt.print_parangle:
        flags['par_angle'] = d.parallactic_angles[isub]
    for k, v in opt.addtnl_toa_flags.items():
        flags[k] = v
    return flags


class GetTOAs(object):
    """Measure wideband TOAs and DMs (pptoas.py:75-1419, the get_TOAs path)."""

    def __init__(self, datafiles, modelfile, quiet=False):
        if isinstance(datafiles, (list, tuple)):
            self.datafiles = list(datafiles)
        elif isinstance(datafiles, str) and not datafiles.endswith(".npz"):
            self.datafiles = [line.rstrip("\n") for line in open(datafiles)]
        else:
            self.datafiles = [datafiles]
        if len(self.datafiles) > max_nfile:
            print("Too many archives.  See/change max_nfile(=%d) in pptoas.py." % max_nfile)
            sys.exit()
        self.is_FITS_model = False
        self.modelfile = modelfile
        for name in ("obs", "doppler_fs", "nu0s", "nu_fits", "nu_refs", "ok_idatafiles",
                     "ok_isubs", "epochs", "MJDs", "Ps", "phis", "phi_errs", "TOAs",
                     "TOA_errs", "DM0s", "DMs", "DM_errs", "DeltaDM_means",
                     "DeltaDM_errs", "GMs", "GM_errs", "taus", "tau_errs", "alphas",
                     "alpha_errs", "scales", "scale_errs", "snrs", "channel_snrs",
                     "profile_fluxes", "profile_flux_errs", "fluxes", "flux_errs",
                     "flux_freqs", "red_chi2s", "channel_red_chi2s", "covariances",
                     "nfevals", "rcs", "fit_durations", "order", "TOA_list",
                     "zap_channels"):
            setattr(self, name, [])
        self.instrumental_response_dict = self.ird = \
            {'DM': 0.0, 'wids': [], 'irf_types': []}
        self.quiet = quiet
        self._gmodels = {}      # model file -> its parsed .gmodel (None: not a .gmodel)

    # -- template ----------------------------------------------------------
    def _gmodel(self):
        """The parsed .gmodel, or None if the model file is not one (then it is
        tried as a spline model: the reference's fallback order, pptoas.py:352-379)."""
        if isinstance(self.modelfile, dict):
            mdl = self.modelfile
        else:
            if self.modelfile not in self._gmodels:         # (parsed once per distinct model file)
                try:
                    mdl = gmodel.read_gmodel(self.modelfile)
                    if mdl["nu_ref"] is None or not mdl["ngauss"]:
                        mdl = None
                except (UnicodeDecodeError, ValueError, IndexError):
                    mdl = None
                self._gmodels[self.modelfile] = mdl
            mdl = self._gmodels[self.modelfile]
        if mdl is not None:
            self.model_name, self.ngauss = mdl["name"], mdl["ngauss"]
            self.model_code, self.model_nu_ref = mdl["code"], mdl["nu_ref"]
            self.gparams, self.alpha = mdl["params"], mdl["alpha"]
        return mdl

    def _model_for(self, freqs_row, nbin, P, unscattered=False):
        """Template portrait (host array) at this subint's frequencies."""
        mdl = self._gmodel()
        if mdl is None:
            from .splmodel import read_spline_model
            self.model_name, port = read_spline_model(self.modelfile, freqs_row, nbin,
                                                      quiet=True)
            return port
        return gmodel.gaussian_portrait(_unscattered(mdl) if unscattered else mdl, freqs_row, nbin, P)

    def _load_template(self, eng, slot, freqs_row, nbin, P, unscattered=False):
        """Put the template for these frequencies into a model slot of the engine:
        Gaussian-component models are synthesised on the device, spline models are
        evaluated on the host and uploaded."""
        mdl = self._gmodel()
        if mdl is None:
            # spline (.spl) template: B-spline curve x eigenvectors evaluated on the
            # device straight into the slot (no host portrait)
            from .splmodel import read_spline_model
            name, _, _, mean_prof, eigvec, tck = read_spline_model(self.modelfile, quiet=True)
            self.model_name = name
            if np.asarray(eigvec).reshape(len(mean_prof), -1).shape[1] <= 32 and \
                    (not np.asarray(eigvec).size or int(tck[2]) <= 5):
                eng.set_model_spline(mean_prof, eigvec, tck, freqs_row, nbin, slot=slot)
                return
        if mdl is None or mdl["ngauss"] > 64:
            eng.set_model(self._model_for(freqs_row, nbin, P, unscattered), slot=slot)
            return
        eng.set_model_gaussian(_unscattered(mdl) if unscattered else mdl, freqs_row, nbin, P, slot=slot)

    def _template_slot(self, eng, slots, key, d, isub, P, unscattered, use_ird, ichans=None):
        """The engine's model slot of the template `key` among an archive's `slots` (key -> slot),
        loaded on first sight from subint isub's frequencies at period P; with use_ird it is
        multiplied there by the instrumental response formed over the channels `ichans` (None:
        all of them) -- in the Fourier domain on the device: constant responses x per-channel
        dispersive smearing."""
        if key not in slots:
            if len(slots) >= 64:
                raise NotImplementedError("more than 64 distinct templates in one archive")
            slots[key] = len(slots)
            self._load_template(eng, slots[key], d.freqs[isub], d.nbin, P, unscattered=unscattered)
            if use_ird:
                from .pptoaslib import instrumental_response_device_args
                freqs = d.freqs[isub] if ichans is None else d.freqs[isub, ichans]
                rconst, smear = instrumental_response_device_args(
                    d.nbin, freqs, self.ird['DM'], d.Ps[isub], self.ird['wids'], self.ird['irf_types'],
                    nchan=d.nchan, ichans=ichans)
                eng.apply_response(slots[key], rconst, smear)
        return slots[key]

    def _reference_seed_inputs(self, port, d, ok_isubs, mask, tau_lin, nu_fit_tau, fit_scat, use_ird):
        """What the reference's phase guess is formed from (pptoas.py:421-457), per good
        subint: the weights of the channel mean, the mean frequency of the good channels and
        the template's mean profile over them (scattered by the guessed tau when fitting
        scattering): (w, nu_mean, mprofs)."""
        isubs = np.asarray(ok_isubs, dtype=int)
        nok, nchan, nbin = port.shape
        w = np.asarray(d.weights, dtype=np.float64)[isubs] * mask
        freqs = d.freqs[isubs]
        nu_mean = np.array([freqs[j, mask[j] > 0].mean() for j in range(nok)])
        mprofs, cache = np.empty((nok, nbin)), {}
        for j, isub in enumerate(isubs):
            key = (d.freqs[isub].tobytes(), float(d.Ps[isub]), mask[j].tobytes(),
                   float(tau_lin[j]), float(nu_fit_tau[j]))
            if key not in cache:
                ich = np.where(mask[j] > 0)[0]
                modelx = self._model_for(d.freqs[isub], nbin, d.Ps[isub], unscattered=fit_scat)[ich]
                if use_ird:
                    from .pptoaslib import instrumental_response_port_FT
                    irf = instrumental_response_port_FT(nbin, d.freqs[isub, ich], self.ird['DM'], d.Ps[isub],
                                                        self.ird['wids'], self.ird['irf_types'])
                    modelx = np.fft.irfft(irf * np.fft.rfft(modelx, axis=-1), axis=-1)
                mprof = modelx.mean(axis=0)
                if fit_scat:
                    k = np.arange(nbin // 2 + 1)
                    mprof = np.fft.irfft(np.fft.rfft(mprof) / (1.0 + 2.0j * np.pi * k * tau_lin[j]))
                cache[key] = mprof
            mprofs[j] = cache[key]
        return w, nu_mean, mprofs

    def _reference_phase_seeds(self, eng, port, freqs, P, w, nu_mean, mprofs, nu_fit_DM, DM_guess):
        """phi_guess of every subint exactly as the reference forms it (pptoas.py:421-457), in
        a pass of its own over the portraits: rot_prof = weighted mean over the good channels
        of the portrait dedispersed at DM_guess to their mean frequency (device: rotation +
        mean), fitted against the template's mean profile with fit_phase_shift(Ns=100) -- brute
        grid + SciPy's simplex finish retraced on the device --, then moved from nu_mean to
        nu_fit_DM.  (The route for batches without a single-pass path, Engine.fit_batch's
        ref_seed.)"""
        nok = len(P)
        # rotate_data(portx, 0.0, DM_guess, P, freqsx, nu_mean): the nu_mean term is the
        # same for every channel of a subint and rides on the phase argument; rotation,
        # weighted channel mean (channels of zero weight are not read) and the fit run
        # in one device call
        out = eng.reference_phase_seed(port, freqs, P, w, mprofs,
                                       phi=-Dconst * DM_guess / P * nu_mean ** -2.0,
                                       DM=np.full(nok, DM_guess), nu_DM=np.inf, Ns=100, finish='simplex')
        return np.array([phase_transform(out[j, 0], DM_guess, nu_mean[j], nu_fit_DM[j], P[j], mod=True)
                         for j in range(nok)])

    def get_TOAs(self, datafile=None, tscrunch=False, nu_refs=None, DM0=None,
                 bary=True, fit_DM=True, fit_GM=False, fit_scat=False,
                 log10_tau=True, scat_guess=None, fix_alpha=False,
                 print_phase=False, print_flux=False, print_parangle=False,
                 add_instrumental_response=False, addtnl_toa_flags={},
                 method='trust-ncg', bounds=None, nu_fits=None, show_plot=False,
                 quiet=None, seed='reference', distributed=False):
        """Same arguments as the reference (pptoas.py:150-156), plus `seed` and
        `distributed`.  tscrunch=True scrunches every archive to one subint on the device
        after loading (scrunch.tscrunch: the archive's weights, the epoch rule of that
        module) and fits the scrunched tensor where it is: one TOA per archive.  Not
        supported here: show_plot (it raises) -- it lives in the plotting code.

        seed='reference' (default -- a drop-in returns the reference's numbers): the
        reference's initial guesses, formed the way it forms them (pptoas.py:421-457:
        dedisperse to the mean frequency, weighted mean over the good channels,
        fit_phase_shift with SciPy's simplex finish retraced step for step, phase_transform
        to nu_fit) at the price of one more pass over the data; method='trust-ncg' then
        retraces SciPy's iteration from that very point, and get_TOAs returns the
        reference's own numbers, GM and scattering fits included.

        seed='device' (the fast path, ~2.3x the throughput): the phase seed is formed inside
        the fit (the exact maximum of the channel-summed cross-correlation on a pilot subset
        of the channels) and every `method` runs the Newton solver to the rounding of the
        objective -- the optimum itself, within ~1e-9 rot of wherever SciPy's iteration
        stops from the reference's own starting point.

        distributed=True shards the work over the ranks of an initialised
        torch.distributed process group (ValueError if there is none; a world of one is
        the single-process path).  Every rank fits on
        default_engine(LOCAL_RANK % torch.cuda.device_count()).  With at least as many
        archives as ranks, each rank takes a contiguous block of archives
        (dist.shard_range); otherwise every rank reads every archive and fits a
        contiguous block of its good subints.  Each rank does the TOA bookkeeping of its
        own subints; one gather brings the per-archive blocks to rank 0, which rebuilds
        every archive, forms DeltaDM_means / DeltaDM_errs from the merged DMs and fills
        the result lists and TOA_list exactly as a one-process run would
        (fit_durations: the sum over the ranks).  On the other ranks the result lists
        stay EMPTY.  A rank that raises reaches the gather with an error record: rank 0
        then raises RuntimeError naming it, and the failing rank re-raises its own error.
        Bit equality with the one-process run rests on a subint's answer not depending
        on the batch it is fitted in."""
        if quiet is None:
            quiet = self.quiet
        if show_plot:
            raise NotImplementedError("plots are outside the accelerated path")
        if seed not in ('device', 'reference'):
            raise ValueError("seed must be 'device' or 'reference'")
        rank, world = _process_group() if distributed else (0, 1)
        use_ird = bool(add_instrumental_response and
                       (self.ird['DM'] or len(self.ird['wids'])))
        if method not in ('trust-ncg', 'Newton-CG', 'TNC'):
            print("Method '%s' is not implemented." % method)
            sys.exit()
        self.nfit = 1 + int(fit_DM) + int(fit_GM) + 2 * int(fit_scat) - int(fix_alpha)
        self.fit_phi, self.fit_DM, self.fit_GM = True, fit_DM, fit_GM
        self.fit_tau = self.fit_alpha = fit_scat
        if fit_scat:
            self.fit_alpha = not fix_alpha
        self.fit_flags = [1, int(self.fit_DM), int(self.fit_GM), int(self.fit_tau),
                          int(self.fit_alpha)]
        self.log10_tau = log10_tau if fit_scat else False
        log10_tau = self.log10_tau
        if (self.fit_GM or fit_scat) and not quiet and rank == 0:
            print("You are using an experimental functionality of pptoas!")
        self.scat_guess = scat_guess
        self.DM0, self.bary = DM0, bary
        self.tscrunch = tscrunch
        self.add_instrumental_response = add_instrumental_response
        opt = DataBunch(nu_refs=nu_refs, nu_fits=nu_fits, bary=bary, fit_scat=fit_scat,
                        log10_tau=log10_tau, use_ird=use_ird, seed=seed, method=method,
                        print_phase=print_phase, print_flux=print_flux,
                        print_parangle=print_parangle, addtnl_toa_flags=addtnl_toa_flags)
        start = time.time()
        datafiles = self.datafiles if datafile is None else [datafile]
        if world > 1:
            self._get_TOAs_sharded(datafiles, opt, rank, world, quiet)
            self._print_total(start, quiet or rank != 0)
            return
        eng = self._engine(False)
        last_fl = None          # (the reference's `fit_flags` variable lives across subints AND archives of one call)
        for iarch, datafile in enumerate(datafiles):
            loaded = _load_or_skip(datafile, quiet)
            if loaded is None:
                continue
            d, fname = loaded
            if tscrunch:
                d = _tscrunched(eng, d)
            self.ok_idatafiles.append(iarch)
            a, arrays, toas, fit_duration = self._fit_archive(eng, d, fname, d.ok_isubs, last_fl, opt)
            last_fl = a.carry
            self.TOA_list.extend(toas)
            self._append_archive(_archive_meta(d, fname, self.DM0), arrays, fit_duration, quiet)
        self._print_total(start, quiet)

    # -- get_TOAs in stages ---------------------------------------------------
    def _engine(self, distributed):
        """The engine this process fits on: device 0, or LOCAL_RANK's device (modulo the
        visible devices) for a rank of a sharded call.  Under the "nccl" backend the
        device is also made current, where gather_object stages its tensors."""
        if not distributed:
            return default_engine()
        import os
        import torch
        import torch.distributed as tdist
        ndev = torch.cuda.device_count()
        if ndev < 1:
            raise RuntimeError("get_TOAs(distributed=True): no GPU visible to this rank")
        dev = int(os.environ.get("LOCAL_RANK", "0")) % ndev
        if tdist.get_backend() == "nccl":
            torch.cuda.set_device(dev)
        return default_engine(dev)

    def _fit_archive(self, eng, d, fname, isubs, carry, opt):
        """The three stages of an archive for the run `isubs` of its good subints (all of them, or a
        rank's slice) with the fit flags carried in: inputs, fit, TOA bookkeeping.  Returns
        (the inputs -- their .carry goes into the next run --, arrays, toas, fit_duration)."""
        a = self._archive_inputs(eng, d, isubs, carry, opt)
        res, fit_duration, slot_means = self._archive_fit(eng, d, a, opt)
        arrays, toas = self._archive_entries(d, fname, a, res, slot_means, opt)
        return a, arrays, toas, fit_duration

    def _archive_inputs(self, eng, d, isubs, carry, opt):
        """Stage 1 of an archive: everything the device calls need for the good subints
        `isubs` (all of an archive's, or a rank's contiguous slice of them) -- channel
        masks, fit and reference frequencies, initial guesses, templates in the engine's
        model slots, the fit flags (subint_fit_flags from the carry-in `carry`), the
        portraits and, for seed='reference', the inputs of the reference's phase guess."""
        fit_scat, use_ird, log10_tau = opt.fit_scat, opt.use_ird, opt.log10_tau
        nu_refs, nu_fits, bary = opt.nu_refs, opt.nu_fits, opt.bary
        nchan, nbin = d.nchan, d.nbin
        DM_stored = d.DM
        isubs = np.asarray(isubs, dtype=int)
        nok = len(isubs)
        flags_per, carry = subint_fit_flags([len(d.ok_ichans[isub]) for isub in isubs],
                                            self.fit_flags, carry)
        mask = np.zeros((nok, nchan), dtype=np.uint8)
        nu_fit_arr = np.zeros((nok, 3))
        nu_ref_arr = np.full((nok, 3), np.nan)
        x0 = np.zeros((nok, 5))
        slots, slot_of = {}, np.zeros(nok, dtype=np.int32)
        errs = None if d.noise_stds is None else \
            np.ascontiguousarray(np.asarray(d.noise_stds)[isubs, 0], dtype=np.float64)
        tau_lin = np.zeros(nok)      # tau_guess [rot] before any log10 (seed='reference')
        for j, isub in enumerate(isubs):
            ich = np.asarray(d.ok_ichans[isub], dtype=int)
            mask[j, ich] = 1
            freqsx = d.freqs[isub, ich]
            key = d.freqs[isub].tobytes() + np.float64(d.Ps[isub]).tobytes() \
                if (fit_scat or use_ird) else d.freqs[isub].tobytes()
            if use_ird:
                key += ich.tobytes()    # the smearing width uses the good channels' spacing
            # (the response of the good channels, pptoas.py:388-394)
            slot_of[j] = self._template_slot(eng, slots, key, d, isub, d.Ps[isub], fit_scat, use_ird, ichans=ich)
            if nu_fits is None:
                nu_fit = guess_fit_freq(freqsx, d.SNRs[isub, 0, ich])
                nu_fit_arr[j] = nu_fit
            else:
                nu_fit_arr[j] = [nu_fits[0], nu_fits[0], nu_fits[-1]]
            if nu_refs is not None:
                nu_ref_arr[j] = [nu_refs[0], nu_refs[0], nu_refs[-1]]
                if bary and nu_refs[-1]:
                    nu_ref_arr[j, 2] = nu_refs[-1] / d.doppler_factors[isub]
            # initial guesses (pptoas.py:421-460); the phase comes from the
            # device seed
            tau_guess, alpha_guess = 0.0, 0.0
            if fit_scat:
                P = d.Ps[isub]
                if self.scat_guess is not None:
                    tau_s, tau_ref, alpha_guess = self.scat_guess
                    tau_guess = (tau_s / P) * (nu_fit_arr[j, 2] / tau_ref) ** alpha_guess
                else:
                    alpha_guess = self.alpha if hasattr(self, 'alpha') else scattering_alpha
                    if hasattr(self, 'gparams'):
                        tau_guess = (self.gparams[1] / P) * \
                            (nu_fit_arr[j, 2] / self.model_nu_ref) ** alpha_guess
                    else:
                        tau_guess = 0.0
                tau_lin[j] = tau_guess
                if log10_tau:
                    if tau_guess == 0.0:
                        tau_guess = nbin ** -1
                    tau_guess = np.log10(tau_guess)
            x0[j] = [0.0, DM_stored, 0.0, tau_guess, alpha_guess]
        port = _dededisperse(eng, _take_subints(d.subints, isubs), d, isubs)
        ref_in = None
        if opt.seed == 'reference':
            # (batches without a single-pass path read the portraits twice -- seed, fit --:
            # hand them to the device once)
            port = _to_device_once(eng, port)
            ref_in = self._reference_seed_inputs(port, d, isubs, mask, tau_lin, nu_fit_arr[:, 2],
                                                 fit_scat, use_ird)
        return DataBunch(isubs=isubs, mask=mask, nu_fit_arr=nu_fit_arr, nu_ref_arr=nu_ref_arr,
                         x0=x0, flags_per=flags_per, carry=carry, slots=slots, slot_of=slot_of,
                         errs=errs, port=port, ref_in=ref_in)

    def _archive_fit(self, eng, d, a, opt):
        """Stage 2 of an archive: one device call per distinct flag set (normally one)
        over the inputs of _archive_inputs.  Returns (res, fit_duration, slot_means)."""
        seed, method, log10_tau = opt.seed, opt.method, opt.log10_tau
        isubs, port, errs, x0, ref_in = a.isubs, a.port, a.errs, a.x0, a.ref_in
        flags_per, slot_of, mask = a.flags_per, a.slot_of, a.mask
        nok = len(isubs)
        res = None
        for fl in sorted(set(flags_per)):
            sel = np.array([k for k, f in enumerate(flags_per) if f == fl])
            # (all subints in one call is the normal case: no gather copy then)
            if len(sel) == nok:
                psel = port
            elif hasattr(port, "is_cuda"):       # (device tensor: gather on the device)
                import torch
                psel = port[torch.as_tensor(sel, device=port.device)].contiguous()
            else:
                psel = np.ascontiguousarray(port[sel])
            fkw = dict(errs=None if errs is None else errs[sel], nu_fits=a.nu_fit_arr[sel],
                       nu_outs=a.nu_ref_arr[sel], fit_flags=fl, log10_tau=log10_tau, option=0, is_toa=True,
                       model_slot=slot_of[sel], chan_mask=mask[sel], seed_ns=100 if seed == 'device' else 0,
                       method='newton' if seed == 'device' else method)
            fsel, Psel = d.freqs[isubs][sel], np.asarray(d.Ps, dtype=np.float64)[isubs][sel]
            r = None
            if ref_in is not None:
                # the reference's own guess: formed inside the fit's single pass over the
                # portraits where the library has that path, else in a pass of its own
                w_, numean_, mprofs_ = (v[sel] for v in ref_in)
                try:
                    r = eng.fit_batch(psel, fsel, Psel, x0[sel], ref_seed=dict(
                        weights=w_, model_profs=mprofs_, nu_mean=numean_, Ns=100, finish='simplex'), **fkw)
                except EngineNotSupported:
                    x0[sel, 0] = self._reference_phase_seeds(eng, psel, fsel, Psel, w_, numean_, mprofs_,
                                                             a.nu_fit_arr[sel, 0], d.DM)
            if r is None:
                r = eng.fit_batch(psel, fsel, Psel, x0[sel], **fkw)
                if ref_in is not None:
                    # (the fallback route formed the guess in a pass of its own: report it like
                    # the single-pass route does, so every group carries the same keys)
                    r["seed_phase"] = x0[sel, 0].copy()
            if res is None:
                res = {"duration": 0.0}
            for k, v in r.items():
                if isinstance(v, np.ndarray):
                    # (groups may return different key sets: allocate on first sight)
                    if k not in res:
                        res[k] = np.zeros((nok,) + v.shape[1:], dtype=v.dtype)
                    res[k][sel] = v
                elif k != "duration":
                    res.setdefault(k, v)
            res["duration"] += r["duration"]
        fit_duration = res["duration"]
        # template profile means per slot, for the flux estimate (the scattering
        # kernel leaves the mean of a profile unchanged: B_0 = 1)
        slot_means = {}
        if opt.print_flux:
            for sl in set(a.slots.values()):
                slot_means[sl] = eng.model_means(sl, d.nchan, d.nbin)
        return res, fit_duration, slot_means

    def _archive_entries(self, d, fname, a, res, slot_means, opt):
        """Stage 3 of an archive: the TOA bookkeeping on the host (pptoas.py:528-721) for
        the subints a.isubs -- their rows of the archive's per-subint result arrays
        (nsub long; the rows of other subints stay zero) and their TOA objects, in subint
        order.  Returns (arrays, toas); `arrays` is keyed by the result list's name."""
        print_flux = opt.print_flux
        tmplt = self.modelfile if isinstance(self.modelfile, str) else self.model_name
        nsub, nchan = d.nsub, d.nchan
        flags_per, slot_of, nu_fit_arr = a.flags_per, a.slot_of, a.nu_fit_arr
        phis = np.zeros(nsub); phi_errs = np.zeros(nsub)
        TOAs = np.zeros(nsub, dtype="object"); TOA_errs = np.zeros(nsub, dtype="object")
        DMs = np.zeros(nsub); DM_errs = np.zeros(nsub)
        GMs = np.zeros(nsub); GM_errs = np.zeros(nsub)
        taus = np.zeros(nsub); tau_errs = np.zeros(nsub)
        alphas = np.zeros(nsub); alpha_errs = np.zeros(nsub)
        scales = np.zeros([nsub, nchan]); scale_errs = np.zeros([nsub, nchan])
        snrs = np.zeros(nsub); channel_snrs = np.zeros([nsub, nchan])
        red_chi2s = np.zeros(nsub)
        profile_fluxes = np.zeros([nsub, nchan]); profile_flux_errs = np.zeros([nsub, nchan])
        fluxes = np.zeros(nsub); flux_errs = np.zeros(nsub); flux_freqs = np.zeros(nsub)
        covariances = np.zeros([nsub, self.nfit, self.nfit])
        nfevals = np.zeros(nsub, dtype="int"); rcs = np.zeros(nsub, dtype="int")
        nu_fits_out = list(np.zeros([nsub, 3])); nu_refs_out = list(np.zeros([nsub, 3]))
        toas = []
        for j, isub in enumerate(a.isubs):
            fl = flags_per[j]
            P = d.Ps[isub]
            p, e = res["params"][j].copy(), res["param_errs"][j]
            ifit = np.where(fl)[0]
            cov = res["cov"][j][np.ix_(ifit, ifit)]
            TOA_MJD = d.epochs[isub] + MJD(0, (p[0] * P + d.backend_delay) / (3600 * 24.))
            TOA_err = e[0] * P * 1e6   # [us]
            df = d.doppler_factors[isub] if self.bary else 1.0
            DM_out, GM_out = p[1], p[2]
            if self.bary:
                if fl[1]:
                    DM_out *= df
                if fl[2]:
                    GM_out *= df ** 3
            nu_fits_out[isub] = list(nu_fit_arr[j])
            nu_refs_out[isub] = list(res["nu_refs"][j])
            phis[isub], phi_errs[isub] = p[0], e[0]
            TOAs[isub], TOA_errs[isub] = TOA_MJD, TOA_err
            DMs[isub], DM_errs[isub] = DM_out, e[1]
            GMs[isub], GM_errs[isub] = GM_out, e[2]
            taus[isub], tau_errs[isub] = p[3], e[3]
            alphas[isub], alpha_errs[isub] = p[4], e[4]
            nfevals[isub], rcs[isub] = res["nfeval"][j], res["return_code"][j]
            ich = np.asarray(d.ok_ichans[isub], dtype=int)
            scales[isub, ich] = res["scales"][j, ich]
            scale_errs[isub, ich] = res["scale_errs"][j, ich]
            snrs[isub] = res["snr"][j]
            channel_snrs[isub, ich] = res["channel_snrs"][j, ich]
            if cov.shape == covariances[isub].shape:
                covariances[isub] = cov
            elif cov.shape == (1, 1):
                # (`covariances[isub] = results.covariance_matrix`, pptoas.py:598: NumPy broadcasts a 1 x 1 matrix
                # over the whole nfit x nfit slot instead of raising -- a phase-only fit fills every entry with
                # var(phi); reproduced)
                covariances[isub] = cov
            else:
                for ii, a_ in enumerate(ifit):
                    for jj, b_ in enumerate(ifit):
                        if a_ < self.nfit and b_ < self.nfit:
                            covariances[isub][a_, b_] = cov[ii, jj]
            red_chi2s[isub] = res["red_chi2"][j]
            freqsx = d.freqs[isub, ich]
            if print_flux:       # pptoas.py:554-575
                means = slot_means[slot_of[j]][ich]
                profile_fluxes[isub, ich] = means * res["scales"][j, ich]
                profile_flux_errs[isub, ich] = np.abs(means) * res["scale_errs"][j, ich]
                fluxes[isub], flux_errs[isub] = weighted_mean(
                    profile_fluxes[isub, ich], profile_flux_errs[isub, ich])
                flux_freqs[isub], _ = weighted_mean(freqsx, profile_flux_errs[isub, ich])
            DM_flag, DM_err_flag = (DM_out, e[1]) if fl[1] else (None, None)
            flags = toa_flags(d, isub, fl, p, e, cov, GM_out, df, res["nu_refs"][j, 2], res["snr"][j],
                              res["red_chi2"][j], tmplt, opt,
                              flux=(fluxes[isub], flux_errs[isub], flux_freqs[isub]))
            toas.append(TOA(fname, res["nu_refs"][j, 0], TOA_MJD, TOA_err,
                            d.telescope, d.telescope_code, DM_flag,
                            DM_err_flag, flags))
        arrays = dict(nu_fits=nu_fits_out, nu_refs=nu_refs_out, phis=phis, phi_errs=phi_errs,
                      TOAs=TOAs, TOA_errs=TOA_errs, DMs=DMs, DM_errs=DM_errs, GMs=GMs,
                      GM_errs=GM_errs, taus=taus, tau_errs=tau_errs, alphas=alphas,
                      alpha_errs=alpha_errs, scales=scales, scale_errs=scale_errs, snrs=snrs,
                      channel_snrs=channel_snrs, profile_fluxes=profile_fluxes,
                      profile_flux_errs=profile_flux_errs, fluxes=fluxes, flux_errs=flux_errs,
                      flux_freqs=flux_freqs, covariances=covariances, red_chi2s=red_chi2s,
                      nfevals=nfevals, rcs=rcs)
        return arrays, toas

    def _append_archive(self, meta, arrays, fit_duration, quiet):
        """One archive's entries of the result lists; its mean DM offset is formed here
        from the (merged) per-subint DMs (deltadm_mean)."""
        ok_isubs = meta["ok_isubs"]
        DeltaDM_mean, DeltaDM_err = deltadm_mean(arrays["DMs"], arrays["DM_errs"], meta["DM0"],
                                                 ok_isubs)
        self.order.append(meta["fname"])
        for name in _ARCHIVE_META:
            getattr(self, name).append(meta[name])
        self.nu0s.append(meta["nu0"])
        self.DM0s.append(meta["DM0"])
        self.DeltaDM_means.append(DeltaDM_mean)
        self.DeltaDM_errs.append(DeltaDM_err)
        for name in _ARCHIVE_ARRAYS:
            getattr(self, name).append(arrays[name])
        self.fit_durations.append(fit_duration)
        if not quiet:
            print("--------------------------")
            print(meta["fname"])
            print("~%.6f sec/TOA" % (fit_duration / len(ok_isubs)))
            print("Med. TOA error is %.3f us" % (np.median(arrays["phi_errs"][ok_isubs]) *
                                                 meta["Ps"].mean() * 1e6))

    def _print_total(self, start, quiet):
        tot_duration = time.time() - start
        if not quiet and len(self.ok_isubs):
            print("--------------------------")
            print("Total time: %.2f sec, ~%.4f sec/TOA" %
                  (tot_duration, tot_duration / sum(len(o) for o in self.ok_isubs)))

    def _get_TOAs_sharded(self, datafiles, opt, rank, world, quiet):
        """get_TOAs over the ranks of a process group (see its docstring): this rank's
        blocks, ONE gather_object to rank 0, and rank 0's merge."""
        import torch.distributed as tdist
        blocks, error, exc = [], None, None
        try:
            eng = self._engine(True)
            mode, lo, hi = shard_plan(len(datafiles), rank, world)
            if self.tscrunch and mode != "archives":
                # one subint per archive: whole archives only, every rank scrunches its own
                from .dist import shard_range
                mode, (lo, hi) = "archives", shard_range(len(datafiles), rank, world)
            walk_quiet = quiet or rank != 0
            carry = None
            if mode == "archives" and self.fit_DM and self.fit_GM:
                # the flags left over from the archives before this rank's (their weights only)
                for df_ in datafiles[:lo]:
                    carry = subint_fit_flags(good_channel_counts(df_, self.tscrunch), self.fit_flags, carry)[1]
            for iarch in range(lo, hi):
                loaded = _load_or_skip(datafiles[iarch], walk_quiet)
                if loaded is None:
                    continue
                d, fname = loaded
                if self.tscrunch:
                    d = _tscrunched(eng, d)
                ok_isubs = np.asarray(d.ok_isubs, dtype=int)
                nchx = [len(d.ok_ichans[isub]) for isub in ok_isubs]
                j0, j1 = shard_subints(mode, len(ok_isubs), rank, world)
                carry_in = subint_fit_flags(nchx[:j0], self.fit_flags, carry)[1]
                carry = subint_fit_flags(nchx, self.fit_flags, carry)[1]
                if j0 == j1:
                    continue            # (an empty slice of this archive: nothing to send)
                a, arrays, toas, fit_duration = self._fit_archive(eng, d, fname, ok_isubs[j0:j1], carry_in, opt)
                rows = a.isubs
                blocks.append(dict(
                    iarch=iarch, meta=_archive_meta(d, fname, self.DM0), nsub=int(d.nsub), rows=rows,
                    arrays={k: ([v[i] for i in rows] if isinstance(v, list) else v[rows])
                            for k, v in arrays.items()},
                    toas=toas, fit_duration=fit_duration))
        except Exception as err:        # (every rank must reach the gather)
            exc = err
            error = "%s: %s" % (type(err).__name__, err)
            blocks = []
        payload = dict(rank=rank, error=error, blocks=blocks)
        got = [None] * world if rank == 0 else None
        tdist.gather_object(payload, got, dst=0)
        if exc is not None:
            raise exc
        if rank != 0:
            return
        failed = [p for p in got if p["error"] is not None]
        if failed:
            raise RuntimeError("get_TOAs: rank %d failed: %s" % (failed[0]["rank"], failed[0]["error"])
                               + "".join("; rank %d failed: %s" % (p["rank"], p["error"]) for p in failed[1:]))
        by_arch = {}
        for p in got:                    # (rank order: within an archive, subint order)
            for b in p["blocks"]:
                by_arch.setdefault(b["iarch"], []).append(b)
        for iarch in sorted(by_arch):
            arrays, toas, fit_duration, meta = merge_blocks(by_arch[iarch])
            self.ok_idatafiles.append(iarch)
            self.TOA_list.extend(toas)
            self._append_archive(meta, arrays, fit_duration, quiet)

    def get_narrowband_TOAs(self, datafile=None, tscrunch=False, fit_scat=False,
                            log10_tau=True, scat_guess=None, print_phase=False,
                            print_flux=False, print_parangle=False,
                            add_instrumental_response=False, addtnl_toa_flags={},
                            method='trust-ncg', bounds=None, show_plot=False, quiet=None):
        """One TOA per channel (pptoas.py:744-1120): every good channel of every
        good subint is fitted for a phase shift and an amplitude against its
        template profile -- fit_phase_shift, bounds [-0.5, 0.5], Ns = 100 -- in one
        device batch per archive.  print_phase / print_flux cannot work in the
        reference's narrowband path (it reads fields fit_phase_shift does not return)
        and raise.

        fit_scat=True fits a scattering time per channel as well -- the fit the
        reference sketches here (the commented-out fit_phase_shift_scat call,
        pptoas.py:988-991) and does not implement: fit_portrait_full on a one-channel
        portrait, Engine.fit_phase_tau_batch.  The template is the Gaussian model
        without its scattering (a spline model as it is); the guess of every channel is
        narrowband_tau_guesses', at the channel's own frequency (the sketch names a
        nu_fit_tau it never defines); the phase guess is fit_phase_shift's grid against
        the template scattered by that guess.  It fills taus, tau_errs, covariances
        (2 x 2), nfevals and rcs and adds the flags of narrowband_scat_flags.  A channel
        whose fit fails (return code 3: not detected, singular) is reported on stderr
        and gets no TOA."""
        if quiet is None:
            quiet = self.quiet
        if show_plot or print_phase or print_flux:
            raise NotImplementedError("show_plot / print_phase / print_flux "
                                      "are not available for narrowband TOAs")
        if not quiet:
            print("You are using an experimental functionality of pptoas!")
        self.nfit = 2 if fit_scat else 1
        self.fit_phi, self.fit_tau = True, bool(fit_scat)
        self.fit_flags = [1, int(self.fit_tau)]
        self.log10_tau = log10_tau = bool(log10_tau and fit_scat)
        self.scat_guess = scat_guess
        self.tscrunch = tscrunch
        self.add_instrumental_response = add_instrumental_response
        use_ird = bool(add_instrumental_response and
                       (self.ird['DM'] or len(self.ird['wids'])))
        start = time.time()
        datafiles = self.datafiles if datafile is None else [datafile]
        eng = self._engine(False)
        for iarch, datafile in enumerate(datafiles):
            try:
                d, fname = load_bunch(datafile)
            except RuntimeError:
                if not quiet:
                    print("Cannot load_data(%s).  Skipping it." % datafile)
                continue
            if not len(d.ok_isubs):
                if not quiet:
                    print("No subints to fit for %s.  Skipping it." % fname)
                continue
            if tscrunch:
                # (the profiles are gathered on the host below: host subints in, host subints out)
                d = _tscrunched(eng, d, on_device=False)
            self.ok_idatafiles.append(iarch)
            nsub, nchan, nbin = d.nsub, d.nchan, d.nbin
            meta = _archive_meta(d, fname, None)
            ok_isubs = meta["ok_isubs"]
            z2 = lambda dt=np.float64: np.zeros([nsub, nchan], dtype=dt)  # noqa: E731
            phis, phi_errs, taus, tau_errs = z2(), z2(), z2(), z2()
            TOAs, TOA_errs = z2("object"), z2("object")
            scales, scale_errs, channel_snrs = z2(), z2(), z2()
            profile_fluxes, profile_flux_errs, channel_red_chi2s = z2(), z2(), z2()
            covariances = np.zeros([nsub, nchan, self.nfit, self.nfit])
            nfevals, rcs = z2("int"), z2("int")
            # ---- gather every (subint, good channel) profile pair ----
            profs, mprofs, noises, where, tau_guesses = [], [], [], [], []
            sub_all = np.asarray(d.subints)
            if d.dmc:
                sub_all = sub_all.copy()
                sub_all[ok_isubs, 0] = _dededisperse(eng, _take_subints(sub_all, ok_isubs), d, ok_isubs)
            for isub in ok_isubs:
                ich = np.asarray(d.ok_ichans[isub], dtype=int)
                model = np.asarray(self._model_for(d.freqs[isub], nbin, d.Ps[isub], unscattered=fit_scat))
                modelx = model[ich]
                if fit_scat:
                    gm = self._gmodel()
                    tau_guesses.append(narrowband_tau_guesses(
                        d.freqs[isub, ich], d.Ps[isub], nbin, log10_tau, self.scat_guess,
                        None if gm is None else self.gparams[1], None if gm is None else self.model_nu_ref,
                        None if gm is None else self.alpha))
                if use_ird:
                    from .pptoaslib import instrumental_response_port_FT
                    resp = instrumental_response_port_FT(nbin, d.freqs[isub, ich], self.ird['DM'],
                                                         d.Ps[isub], self.ird['wids'],
                                                         self.ird['irf_types'])
                    modelx = np.fft.irfft(resp * np.fft.rfft(modelx, axis=-1), axis=-1)
                profs.append(sub_all[isub, 0, ich])
                mprofs.append(modelx)
                # (NaN: the device measures the noise from the power spectrum)
                noises.append(np.full(len(ich), np.nan) if d.noise_stds is None
                              else np.asarray(d.noise_stds)[isub, 0, ich])
                where += [(isub, ichan) for ichan in ich]
            t0 = time.time()
            if fit_scat:
                scat = eng.fit_phase_tau_batch(np.concatenate(profs), np.concatenate(mprofs),
                                               np.concatenate(noises).astype(np.float64),
                                               tau_guess=np.concatenate(tau_guesses), log10_tau=log10_tau,
                                               bounds=(-0.5, 0.5), Ns=100)
                out = scat[:, [0, 1, 4, 5, 6, 7]]
            else:
                out = eng.fit_phase_shift_batch(np.concatenate(profs), np.concatenate(mprofs),
                                                np.concatenate(noises).astype(np.float64),
                                                bounds=(-0.5, 0.5), Ns=100, finish='simplex')
            fit_duration = time.time() - t0
            # ---- TOA bookkeeping (pptoas.py:994-1088) ----
            for j, ((isub, ichan), r) in enumerate(zip(where, out)):
                phase, phase_err, scale, scale_err, snr, red_chi2 = r[:6]
                P = d.Ps[isub]
                scat_flags = {}
                if fit_scat:
                    from .pptoaslib import phase_tau_covariance
                    nfevals[isub, ichan], rcs[isub, ichan] = int(scat[j, 9]), int(scat[j, 10])
                    if rcs[isub, ichan] not in (0, 1, 2, 4):
                        sys.stderr.write("Fit 'failed' with return code %d: NaN, singular or undetected -- %s "
                                         "subint %d channel %d\n" % (rcs[isub, ichan], fname, isub, ichan))
                        continue
                    taus[isub, ichan], tau_errs[isub, ichan] = scat[j, 2], scat[j, 3]
                    covariances[isub, ichan] = phase_tau_covariance(scat[j])
                    scat_flags = narrowband_scat_flags(scat[j, 2], scat[j, 3], scat[j, 8], P,
                                                       d.doppler_factors[isub], log10_tau)
                TOA_MJD = d.epochs[isub] + MJD(0, (phase * P + d.backend_delay) / (3600 * 24.))
                TOA_err = phase_err * P * 1e6
                phis[isub, ichan], phi_errs[isub, ichan] = phase, phase_err
                TOAs[isub, ichan], TOA_errs[isub, ichan] = TOA_MJD, TOA_err
                scales[isub, ichan], scale_errs[isub, ichan] = scale, scale_err
                channel_snrs[isub, ichan] = snr
                channel_red_chi2s[isub] = red_chi2     # (the reference assigns the whole row)
                toa_flags = dict(scat_flags)
                toa_flags.update({'be': d.backend, 'fe': d.frontend, 'f': d.frontend + "_" + d.backend,
                                  'nbin': int(nbin), 'bw': abs(d.bw) / nchan, 'subint': int(isub),
                                  'chan': int(ichan), 'tobs': d.subtimes[isub],
                                  'tmplt': self.modelfile if isinstance(self.modelfile, str)
                                  else self.model_name, 'snr': snr, 'gof': red_chi2})
                if print_parangle:
                    toa_flags['par_angle'] = d.parallactic_angles[isub]
                for k, v in addtnl_toa_flags.items():
                    toa_flags[k] = v
                self.TOA_list.append(TOA(fname, d.freqs[isub, ichan], TOA_MJD, TOA_err,
                                         d.telescope, d.telescope_code, None, None, toa_flags))
            self.order.append(fname)
            for name in _ARCHIVE_META:
                getattr(self, name).append(meta[name])
            arrays = dict(phis=phis, phi_errs=phi_errs, TOAs=TOAs, TOA_errs=TOA_errs, taus=taus, tau_errs=tau_errs,
                          scales=scales, scale_errs=scale_errs, channel_snrs=channel_snrs,
                          profile_fluxes=profile_fluxes, profile_flux_errs=profile_flux_errs,
                          covariances=covariances, channel_red_chi2s=channel_red_chi2s, nfevals=nfevals, rcs=rcs)
            for name in _NARROWBAND_ARRAYS:
                getattr(self, name).append(arrays[name])
            self.fit_durations.append(fit_duration)
            if not quiet:
                print("--------------------------")
                print(fname)
                print("~%.4f sec/TOA" % (fit_duration / max(1, len(self.TOA_list))))
                print("Med. TOA error is %.3f us" % (np.median(phi_errs[ok_isubs]) *
                                                     d.Ps.mean() * 1e6))
        tot_duration = time.time() - start
        if not quiet and len(self.ok_isubs):
            print("--------------------------")
            print("Total time: %.2f sec, ~%.4f sec/TOA" %
                  (tot_duration, tot_duration / max(1, len(self.TOA_list))))

    def get_channels_to_zap(self, SNR_threshold=8.0, rchi2_threshold=1.3, iterate=True,
                            show=False):
        """Flag channels by per-channel reduced chi^2 and S/N (pptoas.py:1208-1285;
        get_TOAs must have been called first).  The reduced chi^2 of every channel of
        every fitted subint -- rotated data minus scaled template in the time domain,
        dof = nbin - 2, as show_fit / get_red_chi2 form it -- comes from one device
        pass per archive; the threshold logic is the reference's.  Appends to
        self.channel_red_chi2s and self.zap_channels (one entry per archive, each a
        list over its fitted subints)."""
        if show:
            raise NotImplementedError("plots are outside the accelerated path")
        eng = self._engine(False)
        for iarch, ok_idatafile in enumerate(self.ok_idatafiles):
            data, fname = load_bunch(self.datafiles[ok_idatafile])
            if getattr(self, "tscrunch", False):
                # the fit was of the scrunched archive: so is its residual (the reference reloads with
                # load_data(..., tscrunch=self.tscrunch), pptoas.py:1305-1306)
                data = _tscrunched(eng, data)
            d = data
            ok_isubs = np.asarray(self.ok_isubs[iarch], dtype=int)
            nok = len(ok_isubs)
            params = np.zeros((nok, 5))
            slots, slot_of = {}, np.zeros(nok, dtype=np.int32)
            scales = np.zeros((nok, d.nchan))
            for j, isub in enumerate(ok_isubs):
                df = self.doppler_fs[iarch][isub] if self.bary else 1.0
                tau = self.taus[iarch][isub]
                if tau != 0.0 and self.log10_tau:
                    tau = 10.0 ** tau
                params[j] = [self.phis[iarch][isub], self.DMs[iarch][isub] / df,
                             self.GMs[iarch][isub] / df ** 3, tau, self.alphas[iarch][isub]]
                scat = bool(tau != 0.0)
                use_ird = bool(getattr(self, "add_instrumental_response", False) and
                               (self.ird['DM'] or len(self.ird['wids'])))
                key = (d.freqs[isub].tobytes(), scat,
                       np.float64(d.Ps[isub]).tobytes() if use_ird else b"")
                # (show_fit applies the response over all channels, pptoas.py:1389-1395)
                slot_of[j] = self._template_slot(eng, slots, key, d, isub, d.Ps.mean(), scat, use_ird)
                scales[j] = self.scales[iarch][isub]
            port = _dededisperse(eng, _take_subints(d.subints, ok_isubs), d, ok_isubs)
            noise = _noise_rows(d, ok_isubs)
            nu_refs = np.array([self.nu_refs[iarch][isub] for isub in ok_isubs], dtype=np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rchi2 = eng.channel_red_chi2(port, d.freqs[ok_isubs], d.Ps[ok_isubs], params,
                                             nu_refs, scales, noise, slots=slot_of)
            channel_red_chi2s, zap_channels = [], []
            for j, isub in enumerate(ok_isubs):
                ok_ichans = [int(v) for v in d.ok_ichans[isub]]
                channel_snrs = self.channel_snrs[iarch][isub]
                thresh = (SNR_threshold ** 2.0 / len(ok_ichans)) ** 0.5
                red_chi2s, bad = [], []
                for ichan in ok_ichans:
                    r = rchi2[j, ichan]
                    red_chi2s.append(r)
                    if r > rchi2_threshold or np.isnan(r):
                        bad.append(ichan)
                    elif SNR_threshold and channel_snrs[ichan] < thresh:
                        bad.append(ichan)
                if iterate and SNR_threshold and len(bad):
                    old_len, added_new = len(bad), True
                    while added_new and (len(ok_ichans) - len(bad)):
                        thresh = (SNR_threshold ** 2.0 / (len(ok_ichans) - len(bad))) ** 0.5
                        for ichan in ok_ichans:
                            if ichan not in bad and channel_snrs[ichan] < thresh:
                                bad.append(ichan)
                        added_new = bool(len(bad) - old_len)
                        old_len = len(bad)
                channel_red_chi2s.append(red_chi2s)
                zap_channels.append(bad)
            self.channel_red_chi2s.append(channel_red_chi2s)
            self.zap_channels.append(zap_channels)

    # -- the fit's residual portrait -----------------------------------------
    def _fitted_archive(self, datafile):
        """Index among the fitted archives of `datafile` (None: the first one listed), as show_fit
        looks it up (pptoas.py:1332-1335)."""
        if datafile is None:
            datafile = self.datafiles[0]
        for iarch, idatafile in enumerate(self.ok_idatafiles):
            f = self.datafiles[idatafile]
            if f is datafile or (isinstance(f, str) and isinstance(datafile, str) and f == datafile):
                return iarch
        raise ValueError("%s is not among the fitted archives" % (datafile if isinstance(datafile, str) else "datafile"))

    def _fitted_inputs(self, eng, iarch, isubs):
        """What Engine.fit_residuals takes for the fitted subints `isubs` of fitted archive iarch,
        rebuilt from the stored results the way get_channels_to_zap rebuilds them: the Doppler
        factors undone, 10**tau for log10_tau, the unscattered template's slot where tau != 0,
        the instrumental response, the scrunched archive after tscrunch=True, a dedispersed
        archive put back.  Returns (d, port, params, nu_refs, scales, noise, slot_of, mask)."""
        data, fname = load_bunch(self.datafiles[self.ok_idatafiles[iarch]])
        if getattr(self, "tscrunch", False):
            data = _tscrunched(eng, data)
        d = data
        isubs = np.asarray(isubs, dtype=int)
        n = len(isubs)
        params = np.zeros((n, 5))
        slots, slot_of = {}, np.zeros(n, dtype=np.int32)
        scales, mask = np.zeros((n, d.nchan)), np.zeros((n, d.nchan))
        for j, isub in enumerate(isubs):
            df = self.doppler_fs[iarch][isub] if self.bary else 1.0
            tau = self.taus[iarch][isub]
            if tau != 0.0 and self.log10_tau:
                tau = 10.0 ** tau
            params[j] = [self.phis[iarch][isub], self.DMs[iarch][isub] / df,
                         self.GMs[iarch][isub] / df ** 3, tau, self.alphas[iarch][isub]]
            scat = bool(tau != 0.0)
            use_ird = bool(getattr(self, "add_instrumental_response", False) and
                           (self.ird['DM'] or len(self.ird['wids'])))
            key = (d.freqs[isub].tobytes(), scat,
                   np.float64(d.Ps[isub]).tobytes() if use_ird else b"")
            slot_of[j] = self._template_slot(eng, slots, key, d, isub, d.Ps.mean(), scat, use_ird)
            scales[j] = self.scales[iarch][isub]
            mask[j, np.asarray(d.ok_ichans[isub], dtype=int)] = 1.0
        port = _dededisperse(eng, _take_subints(d.subints, isubs), d, isubs)
        nu_refs = np.array([self.nu_refs[iarch][isub] for isub in isubs], dtype=np.float64)
        return d, port, params, nu_refs, scales, _noise_rows(d, isubs), slot_of, mask

    def show_fit(self, datafile=None, isub=0, rotate=0.0, show=False, return_fit=True,
                 savefig=False, quiet=None):
        """The fit of one subint as the reference returns it (pptoas.py:1317-1419; get_TOAs
        must have been called first): (port, model_scaled, ok_ichans, freqs, noise_stds) --
        the subint rotated by the fitted (phi, DM, GM) onto the template, zapped channels
        zeroed, and the template scattered by the fitted (tau, alpha) and multiplied by the
        fitted amplitudes; both turned by `rotate` [rot].  One device call
        (Engine.fit_residuals).  Plots are not drawn here.  `quiet` is taken for the
        reference's signature and has no effect: nothing is printed either way."""
        if show or savefig:
            raise NotImplementedError("plots are outside the accelerated path")
        eng = self._engine(False)
        iarch = self._fitted_archive(datafile)
        d, port, params, nu_refs, scales, noise, slot_of, mask = self._fitted_inputs(eng, iarch, [isub])
        fit = eng.fit_residuals(port, d.freqs[[isub]], d.Ps[[isub]], params, nu_refs, scales, mask=mask,
                                slots=slot_of, frame="model", want=("port", "model"))
        out = []
        for name in ("port", "model"):
            a = fit[name]
            if rotate:
                a = eng.rotate_portraits(a, np.full(d.nchan, np.inf), 1.0, phi=float(rotate))
            out.append((a.cpu().numpy() if hasattr(a, "is_cuda") else a)[0])
        if return_fit:
            return (out[0], out[1], d.ok_ichans[isub], d.freqs[isub], noise[0])

    def get_residuals(self, datafile=None, frame="model", on_device=False):
        """The residual portrait -- data minus fitted model -- of every fitted subint of one
        archive, in one device call (get_TOAs must have been called first).  frame "model": the
        rows aligned with the template (show_fit's port - model_scaled); "data": the rows as
        they were fitted, the model rotated back onto them.  Returns a DataBunch of
        resid[nsub,nchan,nbin] (zero rows for subints and channels that were not fitted; a
        device tensor with on_device), channel_red_chi2[nsub,nchan] (time domain, dof = nbin - 2;
        NaN where nothing was fitted), the noise_stds[nsub,nchan] it was formed with, ok_isubs and
        ok_ichans."""
        eng = self._engine(False)
        iarch = self._fitted_archive(datafile)
        ok_isubs = np.asarray(self.ok_isubs[iarch], dtype=int)
        d, port, params, nu_refs, scales, noise, slot_of, mask = self._fitted_inputs(eng, iarch, ok_isubs)
        if on_device:
            port = _to_device_once(eng, port)
        with np.errstate(divide="ignore", invalid="ignore"):
            fit = eng.fit_residuals(port, d.freqs[ok_isubs], d.Ps[ok_isubs], params, nu_refs, scales, errs=noise,
                                    mask=mask, slots=slot_of, frame=frame, want=("resid", "red_chi2"))
        res, rchi2 = fit["resid"], fit["red_chi2"]
        if hasattr(rchi2, "is_cuda"):
            rchi2 = rchi2.cpu().numpy()
        if hasattr(res, "is_cuda") and not on_device:
            res = res.cpu().numpy()
        shape = (d.nsub, d.nchan, d.nbin)
        if hasattr(res, "is_cuda"):
            resid = res.new_zeros(shape)
            resid[ok_isubs.tolist()] = res
        else:
            resid = np.zeros(shape, dtype=res.dtype)
            resid[ok_isubs] = res
        channel_red_chi2 = np.full((d.nsub, d.nchan), np.nan)
        channel_red_chi2[ok_isubs] = rchi2
        noise_stds = np.full((d.nsub, d.nchan), np.nan)
        noise_stds[ok_isubs] = noise
        return DataBunch(resid=resid, channel_red_chi2=channel_red_chi2, noise_stds=noise_stds, ok_isubs=ok_isubs,
                         ok_ichans=[np.asarray(d.ok_ichans[i], dtype=int) for i in range(d.nsub)])
