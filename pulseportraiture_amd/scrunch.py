"""Archive operations the reference hands to PSRCHIVE inside load_data (pplib.py:2650-2814) -- tscrunch, fscrunch,
pscrunch, dedisperse, dededisperse -- on the DataBunches of .npz archives.  The sums run on the device
(Engine.scrunch, one streaming pass, in f64 and in a fixed order), the rotations are Engine.rotate_portraits, noise and
S/N of the result are measured on the device from the scrunched rows (the reference measures them after PSRCHIVE's
operations too); what is left on the host is bookkeeping in f64.

Every operation takes a DataBunch and returns a new one in which every field load_data fills is consistent.  The
subints stay where they were: a device tensor in gives a device tensor out.

Epoch of a time group.  The archive's subints are taken to be folded against one ephemeris, with bin 0 at the pulse
phase of each subint's own epoch (what PSRCHIVE and make_fake_pulsar write), so subints are added as stored.  With W_s
the summed weight of subint s, e_bar is the first member's epoch plus the W_s-weighted mean of the members' offsets
from it, the anchor e_r is the epoch of the good member nearest e_bar, and the group's epoch is
e_r + round((e_bar - e_r) / P_g) P_g in the MJD class's (day, fraction) arithmetic: a whole number k of the group's
periods from the anchor, so the summed profile's bin 0 has the anchor's pulse phase, at a cost of at most |k| dP where
dP is the drift of the period over the group.  PSRCHIVE snaps with the predictor, which an .npz does not have."""
import numpy as np

from .archive import MJD, measure
from .engine import default_engine
from .pplib import DataBunch

STATES = ("Intensity", "Stokes", "Coherence")


def plan_groups(n, ngroups=None):
    """Offsets [ngroups + 1] of `ngroups` contiguous groups of n members (default 1), as equal as contiguous runs
    allow, the larger ones first.  ValueError for fewer than one group or more groups than members."""
    ngroups = 1 if ngroups is None else int(ngroups)
    if ngroups < 1 or ngroups > int(n):
        raise ValueError("cannot form %d groups of %d members" % (ngroups, n))
    q, r = divmod(int(n), ngroups)
    return np.concatenate([[0], np.cumsum([q + 1] * r + [q] * (ngroups - r))]).astype(np.int32)


def state_of(d):
    """The polarisation state of a DataBunch: its own, or the one its npol implies."""
    return getattr(d, "state", None) or {1: "Intensity", 2: "Coherence"}.get(int(d.npol), "Stokes")


def _live(w):
    """The weights pp_scrunch counts: 0 and NaN skip the row."""
    w = np.asarray(w, dtype=np.float64)
    return np.where(np.isnan(w), 0.0, w)


def _wmean(x, w):
    """Weighted mean over the last axis; the plain mean where the total weight is not positive."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    tot = w.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tot > 0, (w * x).sum(axis=-1) / np.where(tot > 0, tot, 1.0), x.mean(axis=-1))


def group_epoch(epochs, Ws, P):
    """The epoch rule of this module's docstring for one time group: epochs (MJD objects), their summed weights and
    the group's period [s].  A group without a good member gets the plain mean of its epochs, not snapped."""
    Ws = np.asarray(Ws, dtype=np.float64)
    offs = np.array([(e - epochs[0]).in_days() for e in epochs])
    good = np.where(Ws > 0)[0]
    if not len(good):
        return epochs[0] + MJD(0, float(offs.mean()))
    ebar = epochs[0] + MJD(0, float((Ws[good] * offs[good]).sum() / Ws[good].sum()))
    r = good[int(np.argmin([abs((epochs[i] - ebar).in_days()) for i in good]))]
    k = np.round((ebar - epochs[r]).in_days() * 86400.0 / P)
    return epochs[r] + MJD(0, float(k * P / 86400.0))


def measured(eng, d, noise_method=None):
    """noise_stds and SNRs [nsub,npol,nchan] of d's rows, on the device (archive.measure; noise_method: its
    estimator).  Here, and for the bunch that pplib.load_data is handed, a row of zeros -- a dead cell, with no noise
    to divide by -- has S/N 0, not the NaN that a loaded archive gets."""
    measure(eng, d, noise_method=noise_method)
    shape = (d.nsub, d.npol, d.nchan)
    d.noise_stds = d.noise_stds.reshape(shape)
    d.SNRs = np.nan_to_num(d.SNRs, nan=0.0).reshape(shape)


def _finish(eng, d, new, subints, weights, remeasure=True):
    """The new bunch: d's fields, `new` over them, and what follows from the weights as in data_from_arrays."""
    out = DataBunch(**{k: v for k, v in d.items()})
    out.update(new)
    nsub, npol, nchan, nbin = (int(v) for v in subints.shape)
    ok_ichans = [np.where(weights[i] > 0)[0] for i in range(nsub)]
    out.update(subints=subints, weights=weights, nsub=nsub, npol=npol, nchan=nchan, nbin=nbin, ok_ichans=ok_ichans,
               ok_isubs=np.array([i for i in range(nsub) if len(ok_ichans[i])], dtype=int),
               masks=(weights > 0)[:, None, :, None], integration_length=float(np.sum(out["subtimes"])))
    if remeasure:
        measured(eng, out)
    return out


def _subints4(d):
    sub = d.subints
    return sub if sub.ndim == 4 else sub[:, None]


def tscrunch(d, nsub=None, engine=None):
    """Add subints with the archive's weights into `nsub` contiguous groups (default: one), PSRCHIVE's tscrunch.
    subtimes add; Ps, doppler_factors and parallactic_angles are means weighted by the subints' summed weights;
    freqs are the weighted-mean frequencies of the members; the epoch follows the rule of the module's docstring."""
    eng = engine or default_engine()
    t_off = plan_groups(d.nsub, nsub)
    w = _live(d.weights)
    out, wout = eng.scrunch(_subints4(d), w, t_off=t_off, pol_mode="keep")
    Ws = w.sum(axis=1)
    freqs = np.asarray(d.freqs, dtype=np.float64)
    grp = [slice(int(a), int(b)) for a, b in zip(t_off[:-1], t_off[1:])]
    Ps = np.array([_wmean(np.asarray(d.Ps)[g], Ws[g]) for g in grp])
    new = dict(Ps=Ps,
               doppler_factors=np.array([_wmean(np.asarray(d.doppler_factors)[g], Ws[g]) for g in grp]),
               parallactic_angles=np.array([_wmean(np.asarray(d.parallactic_angles)[g], Ws[g]) for g in grp]),
               subtimes=np.array([np.sum(np.asarray(d.subtimes, dtype=np.float64)[g]) for g in grp]),
               freqs=np.array([_wmean(freqs[g].T, w[g].T) for g in grp]),
               epochs=[group_epoch(list(d.epochs)[g], Ws[g], Ps[i]) for i, g in enumerate(grp)])
    return _finish(eng, d, new, out, wout)


def _rotated_to_groups(eng, d, f_off, gfreqs):
    """The subints of an archive stored dispersed with every channel rotated to the weighted-mean frequency of its
    group (gfreqs[nsub,ngf]) with the archive's DM: within a group the channels line up, the groups stay dispersed
    against each other.  ONE rotate_portraits call.  That call takes a frequency per (row, channel) and one reference
    for all, and the delay wanted is Dconst DM (nu_c^-2 - nu_g^-2) / P with a reference per group: so it is handed the
    frequency nu' with nu'^-2 = nu_c^-2 - nu_g^-2 + nu_R^-2 and the reference nu_R, half the lowest frequency, which
    keeps nu'^-2 positive.  (The sum rounds at about 5 nu_min^-2 2^-53: some 1e-12 rot at DM 100, 400 MHz, 1.5 ms.)  A
    device tensor is copied first (rotate_portraits turns device rows in place)."""
    sub = _subints4(d)
    nsub, npol, nchan, nbin = (int(v) for v in sub.shape)
    freqs = np.asarray(d.freqs, dtype=np.float64)
    gf = np.repeat(np.asarray(gfreqs, dtype=np.float64), np.diff(f_off), axis=1)
    nu_R = 0.5 * float(freqs.min())
    eff = (freqs ** -2.0 - gf ** -2.0 + nu_R ** -2.0) ** -0.5
    rows = (sub.clone() if hasattr(sub, "is_cuda") else np.asarray(sub)).reshape(nsub * npol, nchan, nbin)
    out = eng.rotate_portraits(rows, np.repeat(eff, npol, axis=0), np.repeat(np.asarray(d.Ps, dtype=np.float64), npol),
                               DM=float(d.DM), nu_DM=nu_R)
    return out.reshape(nsub, npol, nchan, nbin)


def fscrunch(d, nchan=None, engine=None):
    """Add channels with the archive's weights into `nchan` contiguous groups (default: one), PSRCHIVE's fscrunch.
    An archive stored dispersed (dmc = 0, DM != 0) first has every member channel rotated to its group's weighted-mean
    frequency with the archive's DM, on the device; the groups stay dispersed against each other and dmc stays 0.  A
    dedispersed archive is summed as it is."""
    eng = engine or default_engine()
    f_off = plan_groups(d.nchan, nchan)
    w = _live(d.weights)
    freqs = np.asarray(d.freqs, dtype=np.float64)
    grp = [slice(int(a), int(b)) for a, b in zip(f_off[:-1], f_off[1:])]
    gfreqs = np.stack([_wmean(freqs[:, g], w[:, g]) for g in grp], axis=1)
    sub = _subints4(d)
    if not d.dmc and d.DM:
        sub = _rotated_to_groups(eng, d, f_off, gfreqs)
    out, wout = eng.scrunch(sub, w, f_off=f_off, pol_mode="keep")
    return _finish(eng, d, dict(freqs=gfreqs), out, wout)


def pscrunch(d, engine=None):
    """Total intensity, PSRCHIVE's pscrunch, by the archive's state: 'Coherence' adds the first two polarisations,
    'Stokes' keeps the first, 'Intensity' is returned unchanged."""
    eng = engine or default_engine()
    state = state_of(d)
    if state not in STATES:
        raise ValueError("unknown polarisation state '%s'" % state)
    if state == "Intensity" or int(d.npol) == 1:
        return _finish(eng, d, dict(state="Intensity"), _subints4(d), np.asarray(d.weights, dtype=np.float64),
                       remeasure=d.noise_stds is None)
    # (weight 1 for every row that counts: the rows themselves, not a weighted mean; zapped rows come out as zeros)
    w = _live(d.weights)
    out, _ = eng.scrunch(_subints4(d), (w != 0).astype(np.float64), pol_mode="sum01" if state == "Coherence" else "first")
    return _finish(eng, d, dict(state="Intensity"), out, np.asarray(d.weights, dtype=np.float64))


def _rotated(eng, d, sign):
    sub = _subints4(d)
    nsub, npol, nchan, nbin = (int(v) for v in sub.shape)
    dev = hasattr(sub, "is_cuda")
    rows = (sub.clone() if dev else np.asarray(sub)).reshape(nsub * npol, nchan, nbin)
    out = eng.rotate_portraits(rows, np.repeat(np.asarray(d.freqs, dtype=np.float64), npol, axis=0),
                               np.repeat(np.asarray(d.Ps, dtype=np.float64), npol), DM=sign * float(d.DM),
                               nu_DM=float(d.nu0))
    return out.reshape(nsub, npol, nchan, nbin)


def dedisperse(d, engine=None):
    """The archive with the delay of its DM about nu0 taken out (dmc = 1); unchanged when it is stored that way."""
    eng = engine or default_engine()
    w = np.asarray(d.weights, dtype=np.float64)
    if d.dmc:
        return _finish(eng, d, {}, _subints4(d), w, remeasure=d.noise_stds is None)
    return _finish(eng, d, dict(dmc=1), _rotated(eng, d, +1.0) if d.DM else _subints4(d), w)


def dededisperse(d, engine=None):
    """The archive with the delay of its DM about nu0 put back (dmc = 0); unchanged when it is stored that way."""
    eng = engine or default_engine()
    w = np.asarray(d.weights, dtype=np.float64)
    if not d.dmc:
        return _finish(eng, d, {}, _subints4(d), w, remeasure=d.noise_stds is None)
    return _finish(eng, d, dict(dmc=0), _rotated(eng, d, -1.0) if d.DM else _subints4(d), w)
