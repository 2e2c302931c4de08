"""A plain reference of what the ppgauss device kernels compute (pp_gaussfit.h, and the row code it shares with the
template synthesis in pp_extra.h), written from the algorithm -- gen_gaussian_portrait (pplib.py:853-930) and what it
calls: evolve_parameter, gaussian_profile on get_bin_centers, the scattering filter, rotate_data -- in np.longdouble
with scipy.fft (which transforms long double in long double), and the exact normal equations of integer rows.  No GPU.
tests/test_gauss_refs_cpu.py pins it to the true reference's fixtures; tests/test_gpu_gauss_kernels.py holds the
kernels against it at the row plans, harmonics and sample counts the fixtures do not reach.

A parameter vector is the fit's: [DC, tau [bin], (loc, m_loc, wid, m_wid, amp, m_amp) x ngauss, scattering index].

The second half of the module is the input family of those two test files and the bars of its cases, so that the
CPU file (which records how far the f64 host construction is from this reference) and the GPU file (whose bar that
distance may widen) speak of the same cases."""
import zlib

import numpy as np
import scipy.fft

LD = np.longdouble
PI = np.arctan2(LD(0), LD(-1))
DCONST = 0.000241 ** -1         # pplib.Dconst: an f64 constant of the algorithm, widened as it is


# ---- the model rows ---------------------------------------------------------------------------------
def _evolve(freqs, nu_ref, value, slope, digit):
    """evolve_parameter -> [nchan, ngauss]: '0' a power law value (nu / nu_ref)^slope -- taken in logs by the true
    reference, so a non-positive value gives NaN --, else linear value + slope (nu - nu_ref)."""
    f = np.asarray(freqs, dtype=LD)[:, None]
    value, slope = np.asarray(value, dtype=LD)[None], np.asarray(slope, dtype=LD)[None]
    if digit == "0":
        with np.errstate(all="ignore"):
            return np.where(value > 0, value * (f / LD(nu_ref)) ** slope, LD("nan"))
    return value + slope * (f - LD(nu_ref))


def bin_centres(nbin):
    """get_bin_centers: numpy.linspace in f64, only then widened."""
    return np.linspace(1.0 / (nbin * 2), 1.0 - 1.0 / (nbin * 2), nbin).astype(LD)


def _component(x, loc, wid, flip=False):
    """gaussian_profile(nbin, loc, wid) on the bin centres x -> (row, margin).  A wrapped Gaussian about loc % 1,
    zero beyond 20 sigma, scaled so that the curve through the samples has the value exp(-z^2 / 2) at the largest
    sample, z measured from loc itself (not loc % 1).  margin is the relative gap between the largest and the
    second-largest sample: how close the choice of that sample came to going the other way (inf when the component
    is off or no sample is non-zero).  flip takes the second-largest sample as the peak: the other choice."""
    if not wid > 0:                         # (NaN too)
        return np.zeros(len(x), dtype=LD), np.inf
    sigma = wid / (2 * np.sqrt(2 * np.log(LD(2))))
    mean = loc - np.floor(loc)
    xw = np.where(x > mean + LD(0.5), x - 1, x) if mean < LD(0.5) else np.where(x < mean - LD(0.5), x + 1, x)
    z = (xw - mean) / sigma
    val = np.where(np.abs(z) < 20, np.exp(-z * z / 2) / (sigma * np.sqrt(2 * PI)), LD(0))
    order = np.argsort(-val, kind="stable")
    if val[order[0]] == 0:
        return val, np.inf
    margin = float((val[order[0]] - val[order[1]]) / val[order[0]])
    ipk = order[1] if flip and val[order[1]] > 0 else order[0]
    zpk = (xw[ipk] - loc) / sigma
    return np.exp(-zpk * zpk / 2) / val[ipk] * val, margin


def _vectors(sets):
    sets = np.atleast_2d(np.asarray(sets, dtype=np.float64))
    if (sets.shape[1] - 3) % 6 or sets.shape[1] < 9:
        raise ValueError("a parameter vector holds 3 + 6 ngauss values")
    return sets


def rotations(join_s, band, freqs, nu_ref, P):
    """phi_n [nchan] of one set: phase_j + Dconst DM_j (nu_n^-2 - nu_ref^-2) / P, j the channel's band; 0 in none."""
    f = np.asarray(freqs, dtype=LD)
    phi = np.zeros(len(f), dtype=LD)
    for n, j in enumerate(np.asarray(band)):
        if j >= 0:
            phi[n] = LD(join_s[j, 0]) + LD(DCONST) * LD(join_s[j, 1]) * (f[n] ** -2 - LD(nu_ref) ** -2) / LD(P)
    return phi


def portrait(sets, freqs, nbin, code, nu_ref, join=None, band=None, P=None, flip=None):
    """gen_gaussian_portrait of every parameter vector -> long double [nsets, nchan, nbin].  join [nsets, njoin, 2] =
    (phase, Delta-DM) of every set and band, band [nchan] the band of every channel (-1: in none), P the period: a
    channel in a band is rotated by phi_n after the scattering.  flip [nsets, ngauss] (bool): the components whose peak
    sample is chosen the other way (see _component)."""
    sets = _vectors(sets)
    freqs = np.asarray(freqs, dtype=np.float64)
    x = bin_centres(nbin)
    k = np.arange(nbin // 2 + 1)
    out = np.empty((len(sets), len(freqs), nbin), dtype=LD)
    for s, v in enumerate(sets):
        comps = v[2:-1].reshape(-1, 6)
        locs = _evolve(freqs, nu_ref, comps[:, 0], comps[:, 1], code[0])
        wids = _evolve(freqs, nu_ref, comps[:, 2], comps[:, 3], code[1])
        amps = _evolve(freqs, nu_ref, comps[:, 4], comps[:, 5], code[2])
        for n in range(len(freqs)):
            row = np.zeros(nbin, dtype=LD)
            for c in range(len(comps)):
                row += amps[n, c] * _component(x, locs[n, c], wids[n, c], flip is not None and flip[s, c])[0]
            out[s, n] = LD(v[0]) + row
        phi = None
        if join is not None and band is not None and np.any(np.asarray(join)[s] != 0):
            phi = rotations(np.asarray(join)[s], band, freqs, nu_ref, P)
        if v[1] == 0.0 and phi is None:
            continue
        taus = LD(v[1]) / nbin * (freqs.astype(LD) / LD(nu_ref)) ** LD(v[-1])
        for n in range(len(freqs)):
            if taus[n] == 0 and (phi is None or phi[n] == 0):
                continue
            H = scipy.fft.rfft(out[s, n])
            if taus[n] != 0:
                H = H / (1 + 2j * PI * k * taus[n])
                H[-1] = H[-1].real              # (what irfft keeps of the Nyquist term, before any rotation)
            if phi is not None and phi[n] != 0:
                turn = k * phi[n]
                turn = 2 * PI * (turn - np.rint(turn))
                H = H * (np.cos(turn) + 1j * np.sin(turn))
                H[-1] = H[-1].real
            out[s, n] = scipy.fft.irfft(H, n=nbin)
    assert out.dtype == LD
    return out


def residuals(sets, data, errs, freqs, code, nu_ref, join=None, band=None, P=None, flip=None):
    """(data - portrait) / errs -> long double [nsets, nchan, nbin]; errs [nchan]."""
    data = np.asarray(data)
    model = portrait(sets, freqs, data.shape[-1], code, nu_ref, join, band, P, flip)
    return (data.astype(LD)[None] - model) / np.asarray(errs, dtype=LD)[None, :, None]


def peak_margin(sets, freqs, nbin, code, nu_ref):
    """[nsets, nchan, ngauss]: _component's margin of every component in every channel."""
    sets = _vectors(sets)
    x = bin_centres(nbin)
    out = np.empty((len(sets), len(freqs), (sets.shape[1] - 3) // 6))
    for s, v in enumerate(sets):
        comps = v[2:-1].reshape(-1, 6)
        locs = _evolve(freqs, nu_ref, comps[:, 0], comps[:, 1], code[0])
        wids = _evolve(freqs, nu_ref, comps[:, 2], comps[:, 3], code[1])
        for n in range(len(freqs)):
            for c in range(len(comps)):
                out[s, n, c] = _component(x, locs[n, c], wids[n, c])[1]
    return out


# ---- the normal equations, exactly --------------------------------------------------------------------
def gram_rows(R_int, shifts):
    """The f64 rows and steps gram_exact speaks of: R_0 = R_int[0], R_a = R_0 + 2^-s_a R_int[a], h_a = 2^-s_a.  Every
    R_a is an exact f64 (asserted), so R_a - R_0 and its quotient by h_a are exact too: V_a = R_int[a]."""
    R_int = np.asarray(R_int, dtype=np.int64)
    shifts = np.asarray(shifts, dtype=np.int64)
    assert len(shifts) == len(R_int) - 1 and np.all(shifts >= 0) and np.all(shifts <= 40)
    h = 2.0 ** -shifts.astype(np.float64)
    R = np.empty(R_int.shape)
    R[0] = R_int[0]
    for a in range(1, len(R_int)):
        scaled = R_int[0] * (1 << int(shifts[a - 1])) + R_int[a]        # R_a 2^s_a, an integer
        assert np.abs(scaled).max() < 2 ** 53
        R[a] = scaled.astype(np.float64) * h[a - 1]
        assert np.array_equal((R[a] - R[0]) / h[a - 1], R_int[a])
    return R, h


def gram_exact(R_int, shifts):
    """(chi2, g, G) exactly, as the kernel's V_0 = R_0, V_a = (R_a - R_0) / h_a define them, of the rows of
    gram_rows(R_int, shifts): V = R_int, so chi2 = V_0 . V_0, g_a = V_a . V_0, G_ab = V_a . V_b in integers.  In int64
    where nrow max|V|^2 < 2^53 (then every partial sum of every order is an exact f64 as well), else in Python
    integers."""
    V = np.asarray(R_int, dtype=np.int64)
    gram_rows(V, shifts)                    # (the rows are what the docstring says)
    if V.shape[1] * int(np.abs(V).max()) ** 2 < 2 ** 53:
        S = V @ V.T
    else:
        S = np.array([[sum(int(p) * int(q) for p, q in zip(V[a], V[b])) for b in range(len(V))] for a in range(len(V))],
                     dtype=object)
    return S[0, 0], S[0, 1:], S[1:, 1:]


def integer_rows(nsets, nrow, seed):
    """(R_int [nsets, nrow], shifts [nsets - 1]): random nonzero integers in [-512, 512], steps 2^-3 ... 2^-20."""
    rng = np.random.default_rng(seed)
    R = rng.integers(1, 513, size=(nsets, nrow)) * rng.choice([-1, 1], size=(nsets, nrow))
    return R.astype(np.int64), rng.integers(3, 21, size=nsets - 1)


# ---- the input family ---------------------------------------------------------------------------------
# the five-component edge model of tests/golden/make_golden_ppgauss.py: wrap at phase 0/1, a loc outside [0,1), a
# non-positive width
EDGE = [[0.02, -1e-5, 0.03, 2e-6, 3.0, -5e-4], [0.97, 2e-5, 0.012, -1e-6, 1.5, 1e-3], [0.50, 0.0, 0.2, 1e-5, 0.4, 0.0],
        [1.30, 0.0, 0.05, 0.0, 1.0, 0.0], [0.70, 0.0, -0.01, 0.0, 1.0, 0.0]]
NU_REF, ALPHA, DC = 1500.0, -3.7, 0.01
FREQS = np.array([1180.0, 1340.0, 1500.0, 1660.0, 1820.0])
ERRS = np.array([0.05, 0.07, 0.11, 0.06, 0.09])
BAND = np.array([0, -1, 1, 0, 1])           # two bands and a channel in none
PERIOD = 0.005
NARROW, ON_EDGE, ON_CENTRE, OUTSIDE = 5, 6, 7, 3      # component numbers
TAU_BINS = 0.9
CODES = ("000", "011")
POW2_NBIN = (32, 128, 512, 2048, 4096, 8192)          # M = 16, 64, 256, 1024, 2048, 4096
ANY_NBIN = (8, 250, 3000, 4094)                       # the general-length route, both ends of its range


def family_comps(nbin):
    """The edge model plus three components of no evolution: FWHM 1.2 bins, a fifth of a bin past a bin edge (its
    samples alternate in sign against the Nyquist harmonic almost fully); a mean exactly on a bin edge; a mean exactly
    on a bin centre."""
    narrow = [(int(0.6 * nbin) + 0.2) / nbin, 0.0, 1.2 / nbin, 0.0, 8.0, 0.0]
    on_edge = [int(0.4 * nbin) / nbin, 0.0, 2.0 / nbin, 0.0, 2.0, 0.0]
    on_centre = [(int(0.8 * nbin) + 0.5) / nbin, 0.0, 2.0 / nbin, 0.0, 2.0, 0.0]
    return np.array(EDGE + [narrow, on_edge, on_centre])


def on_edge(sets, nbin):
    """[nsets, ngauss] (bool): the components whose loc parameter sits on a bin edge, loc nbin a whole number (to 1e-6
    of a bin).  ON_EDGE on purpose; the edge model's loc 0.50 at every even row length, its 0.02, 0.97 and 1.30 at some.
    Read from the parameters, never from a margin.  Where such a loc does not evolve (or at nu_ref) the two samples
    beside the mean tie to rounding, and which of them is taken as the peak decides nothing: the row is the same
    (tests/test_gauss_refs_cpu.py shows that through the reference, with every one of them flipped)."""
    loc = _vectors(sets)[:, 2:-1:6] * float(nbin)
    return np.abs(loc - np.rint(loc)) < 1e-6


def vector(comps, dc=DC, tau_bins=0.0, alpha=ALPHA):
    return np.concatenate([[dc, tau_bins], np.ravel(comps), [alpha]])


def row_sets(nbin):
    """Four sets of one launch: the base point, tau stepped from 0, alpha stepped (scattered, as the tau-stepped set
    is), a loc stepped."""
    comps = family_comps(nbin)
    moved = comps.copy()
    moved[1, 0] += 1e-3
    return np.array([vector(comps), vector(comps, tau_bins=TAU_BINS), vector(comps, tau_bins=TAU_BINS, alpha=ALPHA + 0.05),
                     vector(moved)])


def joined_sets(nbin):
    """(sets, join [5, 2, 2]): unjoined (an all-zero join), rotated with tau = 0, rotated and scattered, phase-only,
    Delta-DM-only."""
    comps = family_comps(nbin)
    sets = np.array([vector(comps), vector(comps), vector(comps, tau_bins=TAU_BINS), vector(comps), vector(comps)])
    join = np.zeros((5, 2, 2))
    join[1] = join[2] = [[0.137, 2e-3], [-0.0421, -1e-3]]
    join[3, :, 0] = [0.137, -0.0421]
    join[4, :, 1] = [2e-3, -1e-3]
    return sets, join


def extreme_sets(nbin, ngauss=None):
    """The filter's extremes: 2 pi M tau_n ~ 1e6, tau = 1e-12 rot, tau = 0, alpha = 0 and alpha = -4.4 (scattered);
    ngauss 1 or 16 instead: the narrow component alone, or the family's eight twice (the second eight moved by 0.11)."""
    comps = family_comps(nbin)
    if ngauss == 1:
        return np.array([vector(comps[NARROW:NARROW + 1]), vector(comps[NARROW:NARROW + 1], tau_bins=TAU_BINS)])
    if ngauss == 16:
        more = comps.copy()
        more[:, 0] += 0.11
        comps = np.vstack([comps, more])
        return np.array([vector(comps), vector(comps, tau_bins=TAU_BINS)])
    huge = 1e6 / (2 * np.pi * (nbin // 2)) * nbin       # [bin]
    return np.array([vector(comps, tau_bins=huge), vector(comps, tau_bins=1e-12 * nbin), vector(comps),
                     vector(comps, tau_bins=TAU_BINS, alpha=0.0), vector(comps, tau_bins=TAU_BINS, alpha=-4.4)])


def indexed_sets(nbin, nsets=100):
    """Every set with a dc, tau, alpha and one component value of its own (set 0 unscattered)."""
    comps = family_comps(nbin)
    out = []
    for s in range(nsets):
        c = comps.copy()
        c[s % len(c), (0, 2, 4)[s % 3]] *= 1.0 + 1e-3 * (s + 1)
        out.append(vector(c, dc=DC + 1e-3 * s, tau_bins=0.05 * s, alpha=ALPHA + 0.01 * s))
    return np.array(out)


class Case(object):
    """One launch of residual rows (or of template rows): its inputs, and -- on demand, once -- the long-double
    reference, the f64 host construction's distance from it, and the bar."""

    def __init__(self, name, nbin, code, sets, freqs=FREQS, errs=ERRS, join=None, seed=0):
        self.name, self.nbin, self.code, self.sets = name, nbin, code, np.asarray(sets, dtype=np.float64)
        self.freqs, self.errs, self.join = np.asarray(freqs), np.asarray(errs), join
        self.band = None if join is None else BAND[:len(self.freqs)]
        self.seed = seed
        self._ref = None

    def kw(self):
        return dict(join=self.join, band=self.band, P=PERIOD) if self.join is not None else {}

    def reference(self):
        """dict(model, data, rows, standing, host, bar): the long-double model rows [nsets, nchan, nbin]; the data --
        the model of a vector with shifted parameters plus seeded noise, on a grid of 2^-20 (exact in f32 too); the
        long-double residual rows; per channel the standing bar 2e-14 max|model| / sigma_n + spacing(max|data| /
        sigma_n), the f64 host construction's largest distance from the rows, and the bar: the larger of the standing
        bar and ten times that distance."""
        if self._ref is None:
            from pulseportraiture_amd import gaussfit
            model = portrait(self.sets, self.freqs, self.nbin, self.code, NU_REF, **self.kw())
            shifted = self.sets[0].copy()
            shifted[0] += 2e-3
            shifted[2:-1:6] += 3e-4             # every loc
            shifted[6:-1:6] *= 1.02             # every amp
            rng = np.random.default_rng(7000 + self.seed)
            data = portrait(shifted, self.freqs, self.nbin, self.code, NU_REF)[0].astype(np.float64)
            data = np.rint((data + self.errs[:, None] * rng.standard_normal(data.shape)) * 2.0 ** 20) / 2.0 ** 20
            assert np.array_equal(data.astype(np.float32).astype(np.float64), data)
            rows = (data.astype(LD)[None] - model) / self.errs.astype(LD)[None, :, None]
            standing = (2e-14 * float(np.abs(model).max()) / self.errs + np.spacing(np.abs(data).max(axis=1) / self.errs))
            vecs = self.sets
            ichans = None
            if self.join is not None:       # (the host's vectors carry the join parameters in front of the index)
                vecs = np.hstack([self.sets[:, :-1], self.join.reshape(len(self.sets), -1), self.sets[:, -1:]])
                ichans = [np.flatnonzero(self.band == j) for j in range(self.join.shape[1])]
            with np.errstate(invalid="ignore"):
                host = gaussfit.host_residuals(vecs, data, self.errs, self.code, self.freqs, NU_REF, ichans, PERIOD)
            host = np.abs(host.reshape(rows.shape).astype(LD) - rows).max(axis=(0, 2)).astype(np.float64)
            self._ref = dict(model=model, data=data, rows=rows, standing=standing, host=host,
                             bar=np.maximum(standing, 10.0 * host))
        return self._ref

    def margins_ok(self):
        """peak_margin >= 1e-9 for every component of every set but the on-edge ones."""
        m = peak_margin(self.sets, self.freqs, self.nbin, self.code, NU_REF)
        keep = ~np.broadcast_to(on_edge(self.sets, self.nbin)[:, None, :], m.shape)
        return float(m[keep].min()) >= 1e-9


_CASES = {}


def case(kind, nbin, code, extra=None):
    """The cases of tests/test_gpu_gauss_kernels.py by name, built once: kind 'rows', 'joined', 'extreme' (extra:
    None, 1 or 16 components), 'indexed'."""
    key = (kind, nbin, code, extra)
    if key not in _CASES:
        name = "%s_n%d_c%s%s" % (kind, nbin, code, "" if extra is None else "_g%d" % extra)
        seed = zlib.crc32(name.encode()) % 100000
        if kind == "rows":
            c = Case(name, nbin, code, row_sets(nbin), seed=seed)
        elif kind == "joined":
            sets, join = joined_sets(nbin)
            c = Case(name, nbin, code, sets, join=join, seed=seed)
        elif kind == "extreme":
            c = Case(name, nbin, code, extreme_sets(nbin, extra), seed=seed)
        elif kind == "indexed":
            c = Case(name, nbin, code, indexed_sets(nbin), freqs=FREQS[[0, 4]], errs=ERRS[[0, 4]], seed=seed)
        else:
            raise ValueError(kind)
        _CASES[key] = c
    return _CASES[key]


def all_cases():
    """Every (kind, nbin, code, extra) of the GPU file's row tests (a to d, and f through the 'rows' cases)."""
    out = []
    for code in CODES:
        for nbin in POW2_NBIN + ANY_NBIN:
            out += [("rows", nbin, code, None), ("joined", nbin, code, None)]
        for nbin in (2048, 250):
            out += [("extreme", nbin, code, None), ("extreme", nbin, code, 1), ("extreme", nbin, code, 16)]
    for nbin in (32, 100):
        out.append(("indexed", nbin, "000", None))
    return out
