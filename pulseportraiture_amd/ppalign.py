"""Iterative alignment and averaging of subintegrations: the array form of
ppalign.align_archives' loop (reference ppalign.py:110-214).

Each subint is fitted for a phase, a DM and channel amplitudes against the
current template -- the reference's own iteration (ppalign.py:180-195): its phase guess
(fit_phase_shift of the dedispersed channel mean, Ns = nbin, SciPy's simplex finish retraced
on the device) and SciPy's trust-ncg retraced from that point, one batched call each --, rotated by the fit and
added to the average with weights scales / errs**2 (one device pass,
Engine.align_accumulate); the average becomes the template of the next iteration.
align_subints takes arrays.  align_archives is the reference's walk over a metafile
of archives (ppalign.py:54-243) -- .npz archives of DataBunch fields; PSRFITS needs
PSRCHIVE -- with the average held on the device from the first subint of the first
archive to the last of the last one (Engine.align_begin / align_add / align_finish).
"""
import numpy as np

from .archive import (data_from_arrays, load_archive, named_datafiles, noise_kwargs, noise_method_in_force,
                      noise_method_scope, write_archive as write_npz)
from .engine import default_engine
from .pplib import Dconst, guess_fit_freq, fit_phase_shift, gaussian_profile, get_noise, get_SNR
from .pptoas import _to_device_once
from .scrunch import tscrunch as _tscrunch


def normalize_portrait(port, method="rms", weights=None, return_norms=False, noise_method=None):
    """Normalise every profile of a portrait (pplib.py:2462-2507).  noise_method: the estimator behind 'rms'
    (get_noise's method; None: archive's scope, else 'PS')."""
    if method not in ("mean", "max", "prof", "rms", "abs"):
        print("Unknown method for normalize_portrait(...), '%s'." % method)
        return None
    port = np.asarray(port, dtype=np.float64)
    norm_port = np.zeros(port.shape)
    norm_vals = np.ones(len(port))
    if method == "prof":
        good = np.where(port.sum(axis=1) != 0.0)[0]
        w = np.ones(len(good)) if weights is None else np.asarray(weights)[good]
        mean_prof = np.average(port[good], axis=0, weights=w)
    for ichan in range(len(port)):
        if port[ichan].any():
            if method == "mean":
                norm = port[ichan].mean()
            elif method == "max":
                norm = port[ichan].max()
            elif method == "prof":
                norm = fit_phase_shift(port[ichan], mean_prof).scale
            elif method == "rms":
                norm = get_noise(port[ichan], method=noise_method_in_force(noise_method) or "PS")
            else:
                norm = (port[ichan] ** 2.0).sum() ** 0.5
            norm_port[ichan] = port[ichan] / norm
            norm_vals[ichan] = norm
    return (norm_port, norm_vals) if return_norms else norm_port


def _rows(a, idx):
    """a[idx] along the first axis, contiguous: NumPy or a device tensor."""
    if hasattr(a, "is_cuda"):
        import torch
        return a[torch.as_tensor(np.asarray(idx), device=a.device)].contiguous()
    return np.ascontiguousarray(a[idx])


def fit_subints(eng, ports, f2, Ps, errs, wts, snrs, mask, templates, DM_guess, fit_dm, slots=None,
                host_ports=None):
    """The reference's fit of every subint of a batch against its template (ppalign.py:180-201):
    its phase guess (fit_phase_shift of the dedispersed channel mean, Ns = nbin, SciPy's simplex
    finish retraced), SciPy's trust-ncg retraced from that point, and the 1-channel hack.

    ports[nsub,nchan,nbin] (NumPy or a device tensor; host_ports: the same rows on the host,
    for the hack), mask[nsub,nchan] the channels each subint uses, templates[i] the host
    template [nchan,nbin] of subint i, row for row with its channels -- resident in model slot
    slots[i] (None: slot 0).  Returns (phase, DM, nu_ref, scales, fit results or None)."""
    nsub, nchan, nbin = (int(v) for v in ports.shape)
    multi = mask.sum(axis=1) > 1          # (subints with one usable channel: the reference's 1-channel hack)
    single = mask.sum(axis=1) == 1
    nu_fit = np.array([guess_fit_freq(f2[i][mask[i] > 0], snrs[i][mask[i] > 0])
                       if mask[i].any() else f2[i].mean() for i in range(nsub)])
    # ---- the reference's own iteration (ppalign.py:180-195) ----
    # phase_guess = fit_phase_shift(average(rotate_data(port, 0, DM_guess, P, freqs, nu_fit), axis=0,
    #                                       weights=weights[ichans]), model[ichans].mean(axis=0), Ns=nbin).phase:
    # rotation to nu_fit, weighted channel mean and the fit (brute grid of nbin points + SciPy's simplex
    # finish retraced) in one device call; the template's mean profile is taken over the channels the
    # subint uses.  Neither wrapped nor moved to another frequency (the rotation is about nu_fit already).
    mprofs = np.empty((nsub, nbin))
    cache = {}
    for i in range(nsub):
        key = (id(templates[i]), mask[i].tobytes())
        if key not in cache:
            ich = np.where(mask[i] > 0)[0]
            cache[key] = templates[i][ich].mean(axis=0) if len(ich) else np.zeros(nbin)
        mprofs[i] = cache[key]
    x0 = np.zeros((nsub, 5))
    x0[:, 1] = DM_guess
    phase, DM, nu_ref = np.zeros(nsub), np.full(nsub, float(DM_guess)), nu_fit.copy()
    scales = np.zeros((nsub, nchan))
    res = None
    isel = np.where(multi)[0]
    if len(isel):
        whole = len(isel) == nsub
        take = (lambda a: a) if whole else (lambda a: np.ascontiguousarray(a[isel]))
        sel_ports = ports if whole else _rows(ports, isel)
        seed = eng.reference_phase_seed(sel_ports, take(f2), take(Ps), take(np.where(mask > 0, wts, 0.0)),
                                        take(mprofs), phi=take(-Dconst * DM_guess / Ps * nu_fit ** -2.0),
                                        DM=np.full(len(isel), float(DM_guess)), nu_DM=np.inf, Ns=nbin,
                                        finish='simplex')
        x0[isel, 0] = seed[:, 0]
        flags = [1, int(bool(fit_dm)), 0, 0, 0]
        # fit_portrait_full(port, model, [phase_guess, DM_guess, 0, 0, 0], P, freqs, [nu_fit] * 3, [None] * 3,
        #                   errs, fit_flags, log10_tau=False): SciPy's trust-ncg retraced from that very point
        res = eng.fit_batch(sel_ports, take(f2), take(Ps), take(x0), errs=take(errs), chan_mask=take(mask),
                            nu_fits=np.repeat(take(nu_fit)[:, None], 3, axis=1), fit_flags=flags,
                            log10_tau=False, method='trust-ncg',
                            model_slot=None if slots is None else take(np.asarray(slots, dtype=np.int32)))
        phase[isel], DM[isel], nu_ref[isel] = res["params"][:, 0], res["params"][:, 1], res["nu_refs"][:, 0]
        scales[isel] = np.where(take(mask) > 0, res["scales"], 0.0)
    if single.any():
        # "1-channel hack" (ppalign.py:196-201): fit_phase_shift of the one profile against its template
        # channel with the channel's noise, DM = the header's, nu_ref = the channel's frequency
        i1 = np.where(single)[0]
        ich = np.array([int(np.where(mask[i] > 0)[0][0]) for i in i1])
        hp = ports if host_ports is None else host_ports
        r1 = eng.fit_phase_shift_batch(np.asarray(hp[i1, ich], dtype=np.float64),
                                       np.array([templates[i][c] for i, c in zip(i1, ich)]),
                                       noise=errs[i1, ich], Ns=nbin, finish='simplex')
        phase[i1], DM[i1], nu_ref[i1] = r1[:, 0], DM_guess, f2[i1, ich]
        scales[i1, ich] = r1[:, 2]
    return phase, DM, nu_ref, scales, res


def align_subints(ports, freqs, Ps, noise_stds, model_port, weights=None, SNRs=None,
                  DM_guess=0.0, fit_dm=True, niter=1, norm=None, engine=None,
                  return_fits=False, quiet=True):
    """Align and average subints against an initial template.

    ports[nsub,nchan,nbin], freqs[nchan] or [nsub,nchan], Ps[nsub],
    noise_stds[nsub,nchan], model_port[nchan,nbin] (the initial guess, same
    channels: the reference's same_freqs branch), weights[nsub,nchan] (0 = channel
    not usable in that subint), SNRs[nsub,nchan] for guess_fit_freq, DM_guess the
    header DM of non-dedispersed data (0.0 if dedispersed).

    Returns the aligned [nchan,nbin] average (channels never hit stay zero), and
    with return_fits=True also the last iteration's fit results.
    """
    eng = engine or default_engine()
    ports = np.asarray(ports)
    nsub, nchan, nbin = ports.shape
    freqs = np.asarray(freqs, dtype=np.float64)
    f2 = freqs if freqs.ndim == 2 else np.broadcast_to(freqs, (nsub, nchan))
    Ps = np.broadcast_to(np.asarray(Ps, dtype=np.float64), (nsub,)).copy()
    errs = np.asarray(noise_stds, dtype=np.float64)
    wts = np.ones((nsub, nchan)) if weights is None else np.asarray(weights, dtype=np.float64)
    snrs = np.ones((nsub, nchan)) if SNRs is None else np.asarray(SNRs, dtype=np.float64)
    mask = (wts > 0.0).astype(np.uint8)
    model_port = np.asarray(model_port, dtype=np.float64)
    res = None
    for it in range(int(niter)):
        if not quiet:
            print("Doing iteration %d..." % (it + 1))
        eng.set_model(model_port)
        phase, DM, nu_ref, scales, res = fit_subints(eng, ports, f2, Ps, errs, wts, snrs, mask,
                                                     [model_port] * nsub, DM_guess, fit_dm)
        w_acc = np.where(mask > 0, scales / errs ** 2.0, 0.0)
        aligned, totw = eng.align_accumulate(ports, f2, Ps, phase, DM, nu_ref, w_acc)
        good = totw > 0
        aligned[good] /= totw[good, None]
        aligned[~good] = 0.0
        model_port = aligned
    if norm in ("mean", "max", "prof", "rms", "abs"):
        model_port = normalize_portrait(model_port, norm)
    return (model_port, res) if return_fits else model_port


# ---------------------------------------------------------------------------
# the walk over archives (ppalign.py:54-243)
# ---------------------------------------------------------------------------
def state_of(data):
    """The polarisation state of an archive as the alignment takes it: its own, or Stokes for four polarisations and
    Intensity for anything else.  (scrunch.state_of is another rule -- two polarisations are Coherence there -- and
    the two give different averages.)"""
    return getattr(data, "state", None) or ("Stokes" if data.npol == 4 else "Intensity")


def _intensity(sub, state):
    """Total intensity [nsub,nchan,nbin] of subints[nsub,npol,nchan,nbin]: polarisation 0, or the
    sum of the first two of a Coherence archive."""
    if sub.shape[1] > 1 and state == "Coherence":
        return np.ascontiguousarray(sub[:, 0] + sub[:, 1])
    return np.ascontiguousarray(sub[:, 0])


def _dedispersed(eng, ports, data, isubs):
    """Total-intensity portraits of subints isubs as load_data(dedisperse=True) has them: an archive stored
    dispersed (dmc = 0, DM != 0) is dedispersed about nu0 (rotate_portraits)."""
    if data.dmc or not data.DM:
        return ports
    return eng.rotate_portraits(ports, np.asarray(data.freqs)[isubs], np.asarray(data.Ps)[isubs],
                                DM=float(data.DM), nu_DM=float(data.nu0))


def profile_SNR(eng, data, state):
    """data.prof_SNR where the archive has one (PSRCHIVE's number cannot be reproduced); otherwise get_SNR of
    the dedispersed profile scrunched over subints and channels with the archive's weights, on the device."""
    if getattr(data, "prof_SNR", None) is not None:
        return float(data.prof_SNR)
    isubs = np.asarray(data.ok_isubs, dtype=int)
    ports = _dedispersed(eng, _intensity(np.asarray(data.subints)[isubs], state), data, isubs)
    w = np.asarray(data.weights, dtype=np.float64)[isubs]
    if not w.sum() > 0:
        return 0.0
    prof = (w[:, :, None] * ports).sum(axis=(0, 1)) / w.sum()
    return float(eng.channel_snrs(prof[None])[0])      # get_SNR (pplib.py:2289-2308)


def initial_template(initial_guess, pscrunch=True, engine=None):
    """(model DataBunch, model_port) from the initial-guess archive as the reference loads it (ppalign.py:
    103-110): dedispersed, T-scrunched with the weights, masks * subints of the first subint, polarisation 0.
    The bunch's freqs[0] and ok_ichans[0] are the model's channels."""
    eng = engine or default_engine()
    data, name = load_archive(initial_guess, eng)
    state = state_of(data)
    if not pscrunch and data.npol == 1:
        raise IndexError(name)
    isubs = np.arange(data.nsub)
    ports = _dedispersed(eng, _intensity(np.asarray(data.subints, dtype=np.float64), state), data, isubs)
    w = np.asarray(data.weights, dtype=np.float64)
    tot = w.sum(axis=0)
    port = np.zeros(ports.shape[1:])
    good = tot > 0
    port[good] = (w[:, good, None] * ports[:, good]).sum(axis=0) / tot[good, None]
    data.model_ok_ichans = np.where(good)[0]
    data.model_freqs = np.asarray(data.freqs, dtype=np.float64)[0]
    return data, port


def nearest_channels(model_freqs, data_freqs):
    """The template channel nearest in frequency to every data channel (ppalign.py:167-172)."""
    return np.array([int(np.argmin(abs(model_freqs - nu))) for nu in data_freqs], dtype=np.int32)


def select_channels(data, isub, model_freqs, model_ok_ichans, same_freqs):
    """(ichans, model_ichans) of one subint (ppalign.py:161-172)."""
    if same_freqs:
        ichans = np.intersect1d(data.ok_ichans[isub], model_ok_ichans)
        return ichans, ichans
    ichans = np.asarray(data.ok_ichans[isub], dtype=int)
    return ichans, nearest_channels(model_freqs, np.asarray(data.freqs)[isub, ichans])


def last_of_each_row(ichans, model_ichans):
    """The data channels whose contribution survives `aligned_port[ipol, model_ichans] += ...`
    (ppalign.py:204-208): NumPy's indexed += is buffered, so of several data channels of ONE subint that
    share a template row only the last one is added (to the portrait and to the weights alike)."""
    keep = {}
    for c, m in zip(ichans, model_ichans):
        keep[int(m)] = int(c)
    return np.array(sorted(keep.values()), dtype=int)


def write_archive(outfile, aligned_port, total_weights, model_data):
    """The averaged portrait as an .npz of DataBunch fields (what the reference unloads into the
    initial guess's archive, ppalign.py:227-242): one subint, DM = 0, dmc = 0, weights 1 where
    anything was added."""
    return write_npz(outfile, dict(
        subints=aligned_port[None], freqs=np.asarray(model_data.freqs, dtype=np.float64)[:1],
        Ps=np.asarray(model_data.Ps, dtype=np.float64)[:1], epochs=model_data.epochs[:1],
        weights=(total_weights > 0).astype(np.float64)[None], DM=0.0, dmc=0, nu0=float(model_data.nu0),
        bw=float(model_data.bw), telescope=str(model_data.telescope), telescope_code=str(model_data.telescope_code),
        backend=str(model_data.backend), frontend=str(model_data.frontend), source=str(model_data.source),
        backend_delay=float(model_data.backend_delay)))


def align_archives(metafile, initial_guess, fit_dm=True, tscrunch=False, pscrunch=True,
                   SNR_cutoff=0.0, outfile=None, norm=None, rot_phase=0.0, place=None,
                   niter=1, quiet=False, engine=None, noise_method=None):
    """Iteratively align and average archives (ppalign.py:54-243).

    Each archive is fitted for a phase, a DM and channel amplitudes against initial_guess; the
    average, weighted by the fitted amplitudes and the channel noise, is the template of the next
    iteration.  It is summed on the device from the first archive to the last (one
    Engine.align_add per archive) and comes back once per iteration.

    metafile: a text file of .npz archive names, or a list of names or DataBunches.
    initial_guess: the .npz archive (or DataBunch) of the initial alignment guess.
    fit_dm=False fits a phase only.  tscrunch=True scrunches every archive to one subint on the device
    before it is aligned (scrunch.tscrunch), as the reference does via load_data(tscrunch=tscrunch).  pscrunch=False
    returns the average Stokes portraits (alignment and weights from total intensity; archives
    of one polarisation are skipped).  SNR_cutoff filters archives by prof_SNR.  outfile defaults
    to <metafile>.algnd.npz.  norm, rot_phase, place (overrides rot_phase), niter, quiet as in the
    reference.  noise_method ('PS' or 'fit'): the estimator of the archives' noise_stds and SNRs, measured anew
    with it, and of the 'rms' norm; None keeps stored values and the power-spectrum estimate.
    Returns (aligned_port[npol,nchan,nbin], total_weights[nchan])."""
    with noise_method_scope(noise_method):
        return _align_archives(metafile, initial_guess, fit_dm, tscrunch, pscrunch, SNR_cutoff, outfile, norm, rot_phase,
                               place, niter, quiet, engine)


def _align_archives(metafile, initial_guess, fit_dm, tscrunch, pscrunch, SNR_cutoff, outfile, norm, rot_phase, place,
                    niter, quiet, engine):
    eng = engine or default_engine()
    if isinstance(metafile, str):
        datafiles = named_datafiles(metafile)
        if outfile is None:
            outfile = metafile + ".algnd.npz"
    else:
        datafiles = list(metafile)
    npol = 1 if pscrunch else 4
    try:
        model_data, model_port = initial_template(initial_guess, pscrunch, eng)
    except IndexError:
        print("%s: has npol = 1; need npol == 4." % initial_guess)
        raise SystemExit
    nchan, nbin = model_port.shape
    model_freqs, model_ok = model_data.model_freqs, model_data.model_ok_ichans
    skip_these, prof_snrs = [], {}
    niter, count = int(niter), 1
    aligned_port, total_weights = np.zeros((npol, nchan, nbin)), np.zeros(nchan)
    eng.set_model(model_port)
    while niter:
        print("Doing iteration %d..." % count)
        eng.align_begin(npol, nchan, nbin)
        if count == 2:
            datafiles = [f for f in datafiles if not any(f is s for s in skip_these)]
        for datafile in datafiles:
            label = datafile if isinstance(datafile, str) else datafile.get("filename", "arrays")
            try:
                data, _ = load_archive(datafile, eng)
                if tscrunch:
                    data = _tscrunch(data, engine=eng)
                state = state_of(data)
                if not pscrunch and data.npol == 1:
                    raise IndexError
                if not pscrunch and state == "Coherence":
                    print("%s: is in the Coherence state; -p needs Stokes archives (PSRCHIVE converts them)." % label)
                    raise SystemExit(1)
            except RuntimeError:
                if not quiet:
                    print("%s: cannot load_data().  Skipping it." % label)
                skip_these.append(datafile)
                continue
            except IndexError:
                if not quiet:
                    print("%s: has npol = 1.  Skipping it." % label)
                skip_these.append(datafile)
                continue
            if data.nbin != nbin:
                if not quiet:
                    print("%s: %d != %d phase bins.  Skipping it." % (label, data.nbin, nbin))
                skip_these.append(datafile)
                continue
            # (an archive without a prof_SNR of its own is measured only where a cutoff asks for it: the measurement
            # reads the whole archive on the host)
            if id(datafile) not in prof_snrs:
                own = getattr(data, "prof_SNR", None)
                prof_snrs[id(datafile)] = profile_SNR(eng, data, state) if own is not None or SNR_cutoff > 0 else np.inf
            if prof_snrs[id(datafile)] < SNR_cutoff:
                if not quiet:
                    print("%s: %d < %d S/N cutoff.  Skipping it." % (label, prof_snrs[id(datafile)], SNR_cutoff))
                skip_these.append(datafile)
                continue
            _align_one_archive(eng, data, state, npol, model_port, model_freqs, model_ok, fit_dm,
                               _to_device_once)
        aligned_port, total_weights = eng.align_finish(0.0, to_slot=0)
        model_port = aligned_port[0]
        niter -= 1
        count += 1
    if norm in ("mean", "max", "prof", "rms", "abs"):
        # normalize_portrait(aligned_port[ipol], norm, weights=None) (ppalign.py:216-219): the norms on the device
        for ipol in range(npol):
            norms = eng.channel_noise(aligned_port[ipol], norm=norm, **noise_kwargs())[1]
            aligned_port[ipol] = aligned_port[ipol] / norms[:, None]
    # rot_phase, then place (ppalign.py:220-226).  While the host rows are still the accumulator's (no norm) the
    # turn is one more finish -- in the spectrum, one inverse transform per row; normalised rows are turned as
    # rotate_data turns them
    resident = norm not in ("mean", "max", "prof", "rms", "abs")

    def turned(port, total):
        if resident:
            return eng.align_finish(total)[0]
        # (rotate_data(port, total), pplib.py:2338-2426: phase only)
        return eng.rotate_portraits(port, np.full(port.shape[1], np.inf), np.ones(len(port)), phi=total)

    if rot_phase:
        aligned_port = turned(aligned_port, float(rot_phase))
    if place is not None:
        prof = np.average(aligned_port[0], axis=0)
        delta = prof.max() * gaussian_profile(len(prof), place, 0.0001)
        turn = float(eng.fit_phase_shift_batch(prof[None], delta[None], Ns=nbin, finish='simplex')[0, 0])
        # (resident: both turns at once from the accumulator; else the second on top of the first)
        aligned_port = turned(aligned_port, float(rot_phase) + turn if resident else turn)
    if outfile is not None:
        outfile = write_archive(outfile, aligned_port, total_weights, model_data)
        if not quiet:
            print("\nUnloaded %s.\n" % outfile)
    return aligned_port, total_weights


def _align_one_archive(eng, data, state, npol, model_port, model_freqs, model_ok, fit_dm, to_device, isubs=None):
    """Fit every good subint of one archive against the template and add it to the resident accumulator
    (ppalign.py:152-208): one upload, one seed, one fit, one align_add.  (isubs: these subints only -- an archive
    whose subints need more template slots than the engine has goes through in runs of subints, in order, which
    the accumulator does not see.)"""
    from ._lib import PP_MAX_SLOTS
    nchan_model, nbin = model_port.shape
    isubs = np.asarray(data.ok_isubs if isubs is None else isubs, dtype=int)
    if not len(isubs):
        return
    freqs = np.asarray(data.freqs, dtype=np.float64)
    try:
        diffs = freqs - model_freqs
        same_freqs = bool(diffs.min() == diffs.max() == 0.0)
    except ValueError:
        same_freqs = False
    if not same_freqs:
        # one template slot per distinct channel map beside slot 0: runs of subints with at most that many maps
        seen, start = set(), 0
        for j, isub in enumerate(isubs):
            seen.add(freqs[isub].tobytes())
            if len(seen) > PP_MAX_SLOTS - 1:
                for part in (isubs[start:j], isubs[j:]):
                    _align_one_archive(eng, data, state, npol, model_port, model_freqs, model_ok, fit_dm, to_device, part)
                return
    DM_guess = float(data.DM) * (not data.dmc)          # = 0.0 if dedispersed
    nchan = data.nchan
    mask = np.zeros((len(isubs), nchan), dtype=np.uint8)
    added = np.zeros((len(isubs), nchan), dtype=bool)
    cmap = None if same_freqs else np.zeros((len(isubs), nchan), dtype=np.int32)
    for j, isub in enumerate(isubs):
        ichans, model_ichans = select_channels(data, isub, model_freqs, model_ok, same_freqs)
        mask[j, ichans] = 1
        if same_freqs:
            added[j, ichans] = True
        else:
            cmap[j] = nearest_channels(model_freqs, freqs[isub])
            added[j, last_of_each_row(ichans, model_ichans)] = True
    sub = np.asarray(data.subints)
    # (a run of consecutive subints is a view: fancy indexing would copy the archive before its upload starts)
    sub = sub[isubs[0]:isubs[0] + len(isubs)] if np.array_equal(isubs, np.arange(isubs[0], isubs[0] + len(isubs))) \
        else sub[isubs]
    if npol == 1 or state == "Coherence":
        host4 = _intensity(sub, state)[:, None]
    else:
        host4 = np.ascontiguousarray(sub)
    dev4 = to_device(eng, host4)
    host = host4[:, 0]
    if hasattr(dev4, "is_cuda"):
        ports = dev4[:, 0].contiguous() if host4.shape[1] > 1 else dev4.reshape(host.shape)
    else:
        ports = np.ascontiguousarray(host)
    # one template slot per distinct channel map; slot 0 is the template itself
    templates, slots = [model_port] * len(isubs), None
    if not same_freqs:
        by_map, slots, templates = {}, np.zeros(len(isubs), dtype=np.int32), []
        for j in range(len(isubs)):
            key = cmap[j].tobytes()
            if key not in by_map:
                by_map[key] = (len(by_map) + 1, np.ascontiguousarray(model_port[cmap[j]]))
                eng.set_model(by_map[key][1], slot=by_map[key][0])
            slots[j] = by_map[key][0]
            templates.append(by_map[key][1])
    f2, Ps = np.ascontiguousarray(freqs[isubs]), np.asarray(data.Ps, dtype=np.float64)[isubs]
    errs = np.asarray(data.noise_stds, dtype=np.float64)[isubs, 0]
    snrs = np.asarray(data.SNRs, dtype=np.float64)[isubs, 0]
    wts = np.asarray(data.weights, dtype=np.float64)[isubs]
    # Every evaluation of the fit is a pass over the cross-spectrum here (option "taylor" 0).  The default solves on a
    # Taylor model of every channel's sums, whose certificate admits a truncation of ~1e-10 at hundreds of harmonics and
    # a DM that is off by a few 1e-4 -- plenty for a TOA, but the average is the next iteration's template and is held to
    # 1e-12 of the reference's
    with eng.options(taylor=0):
        phase, DM, nu_ref, scales, _ = fit_subints(eng, ports, f2, Ps, errs, wts, snrs, mask, templates, DM_guess,
                                                   fit_dm, slots=slots, host_ports=host)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_acc = np.where(added & (mask > 0), scales / errs ** 2.0, 0.0)
    eng.align_add(dev4, f2, Ps, phase, DM, nu_ref, w_acc, cmap)


# ---------------------------------------------------------------------------
# initial guesses of the command line (ppalign.py:341-368)
# ---------------------------------------------------------------------------
def _like(data, subints, weights):
    """A DataBunch of `subints` on the channels, periods and epochs of `data`, DM = 0 and stored dispersed
    (make_constant_portrait's DM=0.0, dmc=False)."""
    n = len(subints)
    return data_from_arrays(subints, np.asarray(data.freqs)[:n], np.asarray(data.Ps)[:n], list(data.epochs)[:n],
                            weights=weights, DM=0.0, dmc=0, telescope=data.telescope,
                            telescope_code=data.telescope_code, backend=data.backend, frontend=data.frontend,
                            bw=data.bw, nu0=data.nu0, source=data.source, backend_delay=data.backend_delay,
                            filename="ppalign.initial_guess")


def constant_portrait(archive, profile, engine=None):
    """make_constant_portrait (pplib.py:958-994): the archive's shape, channels and header with `profile` in
    every row and weights of one."""
    data, _ = load_archive(archive, engine)
    profile = np.asarray(profile, dtype=np.float64)
    assert len(profile) == data.nbin, "len(profile) != number of bins in dummy archive"
    sub = np.broadcast_to(profile, (data.nsub, data.npol, data.nchan, data.nbin)).copy()
    return _like(data, sub, np.ones((data.nsub, data.nchan)))


def scrunched_profile(archive, engine=None):
    """The archive's profile averaged over subints and channels with its weights, dedispersed (what
    make_constant_portrait(profile=None) takes from PSRCHIVE's T-, P- and F-scrunch, up to a scale)."""
    eng = engine or default_engine()
    data, _ = load_archive(archive, eng)
    state = state_of(data)
    isubs = np.arange(data.nsub)
    ports = _dedispersed(eng, _intensity(np.asarray(data.subints, dtype=np.float64), state), data, isubs)
    w = np.asarray(data.weights, dtype=np.float64)
    return (w[:, :, None] * ports).sum(axis=(0, 1)) / w.sum()


def average_guess(datafiles, quiet=True, engine=None):
    """The initial guess when neither -I nor -g is given.  The reference calls `psradd -T` (PSRCHIVE); this is
    the package's own stand-in for it: the weight-weighted mean of all dedispersed subints of all archives, on
    the channels of the first archive that loads, total intensity.  It is formed on the device: one align_add
    per archive at phase 0 with the archive's weights and its own header DM about its nu0 (nothing is turned in
    an archive stored dedispersed); channels of other frequencies go to the nearest channel of the first."""
    eng = engine or default_engine()
    first = None
    for datafile in datafiles:
        try:
            data, name = load_archive(datafile, eng)
        except RuntimeError:
            continue
        state = state_of(data)
        if first is None:
            first = data
            model_freqs = np.asarray(data.freqs, dtype=np.float64)[0]
            eng.align_begin(1, data.nchan, data.nbin)
        if data.nbin != first.nbin:
            continue
        isubs = np.asarray(data.ok_isubs, dtype=int)
        if not len(isubs):
            continue
        freqs = np.asarray(data.freqs, dtype=np.float64)[isubs]
        same = freqs.shape[1] == len(model_freqs) and bool(np.all(freqs == model_freqs))
        cmap = None if same else np.array([nearest_channels(model_freqs, f) for f in freqs])
        DM = float(data.DM) * (not data.dmc)
        eng.align_add(_intensity(np.asarray(data.subints)[isubs], state), freqs, np.asarray(data.Ps)[isubs], 0.0, DM,
                      float(data.nu0), np.asarray(data.weights, dtype=np.float64)[isubs], cmap)
    if first is None:
        raise RuntimeError("no archive of the metafile could be loaded")
    port, totw = eng.align_finish(0.0)
    if not quiet:
        print("Initial guess: the weighted mean of the archives (a stand-in for psradd -T).")
    return _like(first, port[None], (totw > 0).astype(np.float64)[None])
