"""Plain references of the fit's residual portrait (pp_resid.h k_resid, k_resid_harm; GetTOAs.show_fit), written from
the formulas: NumPy and np.longdouble only, no GPU, nothing imported from the package.  tests/test_resid_cpu.py pins
them to the reference's show_fit (tests/golden/showfit.npz) and to rot_refs' rotate_ld / scatter_ld;
tests/test_gpu_resid_kernels.py and tests/test_gpu_ppresid.py hold the device against them.

For row (i, n) with delay phi_n, scattering time tau_n [rot], amplitude a_n, data harmonics d_k and template harmonics
m_k, k = 0 .. M, B_k = 1 / (1 + 2 pi i k tau_n):
    frame "model":  D_k = d_k e^{2 pi i k phi_n},  Mo_k = a_n B_k m_k
    frame "data":   D_k = d_k,                     Mo_k = a_n B_k m_k e^{-2 pi i k phi_n}
    port = irfft(D), model = irfft(Mo), resid = irfft(D - Mo); irfft keeps the real part at DC and Nyquist."""
from functools import lru_cache

import numpy as np

from tests import rot_refs as rr

LD = np.longdouble
FRAMES = ("model", "data")
POW2 = [32, 64, 1024, 2048, 8192]        # every row plan's class of the tuned transforms (64-thread, 256, 512 threads)
ANY = [8, 62, 250, 1026]                 # both ends of the chirp-z classes, and M = 125 (odd)
NSUB, NCHAN = 2, 3


def _harmonics(data_row, model_row, phi_n, tau_n, scale, frame, ld):
    """(D, Mo) as complex pairs (re, im) of harmonics 0 .. M, in long double or f64.  The phasors' turns k phi_n mod 1
    are exact either way (rot_refs.turns_ld): NumPy's k * phi_n would round the product."""
    if frame not in FRAMES:
        raise ValueError(frame)
    nbin = len(data_row)
    k = np.arange(nbin // 2 + 1)
    if ld:
        (dr, di), (mr, mi) = rr._spec_ld(data_row), rr._spec_ld(model_row)      # (kept by the row's bytes: both frames ask)
        c, s = rr.phasor_ld(k, phi_n)
        x = rr.PI2 * k.astype(LD) * LD(tau_n)
        a = LD(scale)
    else:
        d, m = np.fft.rfft(np.asarray(data_row, dtype=np.float64)), np.fft.rfft(np.asarray(model_row, dtype=np.float64))
        dr, di, mr, mi = d.real, d.imag, m.real, m.imag
        c, s = (v.astype(np.float64) for v in rr.phasor_ld(k, phi_n))
        x = 2 * np.pi * k * float(tau_n)
        a = float(scale)
    if tau_n != 0:
        den = 1 / (1 + x * x)
        mr, mi = (mr + mi * x) * den, (mi - mr * x) * den
    mr, mi = a * mr, a * mi
    if frame == "model":
        dr, di = dr * c - di * s, dr * s + di * c
    else:
        mr, mi = mr * c + mi * s, mi * c - mr * s          # times e^{-2 pi i k phi_n}
    return (dr, di), (mr, mi)


def rows_ld(data_row, model_row, phi_n, tau_n, scale, frame):
    """{port, model, resid} of one row in long double.  The transform is linear, so resid is port - model: at 2^-64
    that is the transform of the harmonics' difference, and a long-double transform of 8192 bins takes a second."""
    nbin = len(data_row)
    (dr, di), (mr, mi) = _harmonics(data_row, model_row, phi_n, tau_n, scale, frame, True)
    port = np.asarray(data_row, dtype=LD) if frame == "data" else rr.irfft_ld(dr, di, nbin)
    model = rr.irfft_ld(mr, mi, nbin)
    return dict(port=port, model=model, resid=port - model)


def rows_f64(data_row, model_row, phi_n, tau_n, scale, frame):
    """The same with NumPy's f64 transforms."""
    nbin = len(data_row)
    (dr, di), (mr, mi) = _harmonics(data_row, model_row, phi_n, tau_n, scale, frame, False)
    return dict(port=np.fft.irfft(dr + 1j * di, nbin), model=np.fft.irfft(mr + 1j * mi, nbin),
                resid=np.fft.irfft((dr - mr) + 1j * (di - mi), nbin))


def rows_composed_ld(data_row, model_row, phi_n, tau_n, scale, frame):
    """{port, model} from rot_refs' rotate_ld and scatter_ld, one after the other (what show_fit does, and its mirror
    image in the data's frame)."""
    m = LD(scale) * rr.scatter_ld(model_row, tau_n)
    if frame == "model":
        return dict(port=rr.rotate_ld(data_row, phi_n), model=m)
    return dict(port=np.asarray(data_row, dtype=LD), model=rr.rotate_ld(m, -phi_n))


def red_chi2_f64(resid_row, sigma):
    """get_red_chi2 of a residual row: sum r^2 / sigma^2 / (nbin - 2)."""
    r = np.asarray(resid_row, dtype=np.float64)
    return float(np.sum(r * r) / sigma ** 2 / (len(r) - 2))


def portrait_f64(data, templates, slots, phin, taun, scales, frame):
    """{port, model, resid}[nsub, nchan, nbin] of every row by rows_f64."""
    nsub, nchan, nbin = data.shape
    out = {w: np.empty((nsub, nchan, nbin)) for w in ("port", "model", "resid")}
    for i in range(nsub):
        for n in range(nchan):
            r = rows_f64(data[i, n], templates[slots[i], n], phin[i, n], taun[i, n], scales[i, n], frame)
            for w in out:
                out[w][i, n] = r[w]
    return out


# ==== inputs shared by the CPU and the GPU file ============================================================
SUBS = [1, 3]          # of rot_refs.b1_case: (phi, DM at a finite nu_DM, a negative scale) and (phi, DM, tau, alpha)


@lru_cache(maxsize=None)
def case(nbin):
    """2 subints x 3 channels cut from rot_refs.b1_case(nbin) -- subints 1 and 3, channels 0 .. 2, on templates 1 and
    0 --: per-subint frequency rows, tau = 0 next to tau != 0, scales[0, 2] < 0; f32-exact data and templates."""
    c = rr.b1_case(nbin)
    cut = lambda a: np.ascontiguousarray(a[SUBS][:, :NCHAN])       # noqa: E731
    out = dict(data=cut(c["data"]), templates=np.ascontiguousarray(c["templates"][:, :NCHAN]),
               slots=[rr.B_SLOTS[i] for i in SUBS], freqs=cut(c["freqs"]), P=c["P"][SUBS], params=c["params"][SUBS],
               nu_refs=c["nu_refs"][SUBS], scales=cut(c["scales"]), sigma=cut(c["sigma"]), phin=cut(c["phin"]),
               taun=cut(c["taun"]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def ld_rows(nbin):
    """The (subint, channel) rows that get a long-double reference: rot_refs.ld_rows' choice for a 2 x 3 cube -- four
    rows spread over both subints, two (one of each subint) at nbin >= 4094, where a long-double transform takes about
    a second."""
    rows = [0, 4] if nbin >= 4094 else rr.ld_rows(nbin, NSUB * NCHAN)
    return [(r // NCHAN, r % NCHAN) for r in rows]


@lru_cache(maxsize=None)
def reference(nbin, frame):
    """{port, model, resid}[2, 3, nbin] in f64 by rows_f64, and {(i, n): rows_ld} for ld_rows(nbin)."""
    c = case(nbin)
    full = portrait_f64(c["data"], c["templates"], c["slots"], c["phin"], c["taun"], c["scales"], frame)
    ld = {p: rows_ld(c["data"][p], c["templates"][c["slots"][p[0]], p[1]], c["phin"][p], c["taun"][p], c["scales"][p],
                     frame) for p in ld_rows(nbin)}
    return full, ld


def scale_of(c):
    """max |data row| + |a_n| max |model row| for every row of a case: what the bars multiply."""
    tm = np.stack([c["templates"][s] for s in c["slots"]])
    return np.abs(c["data"]).max(axis=-1) + np.abs(c["scales"]) * np.abs(tm).max(axis=-1)
