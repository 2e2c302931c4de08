"""NumPy restatement of pp_scrunch for the tests: every output element is the f64 sum of its members in ascending
(subint, channel) order -- a sequential loop, not np.sum, whose pairwise order differs -- divided once at the end."""
import numpy as np


def live(w):
    return not (w == 0.0 or w != w)


def scrunch_ref(ports, weights, t_off=None, f_off=None, pol_mode="keep"):
    """(out, wout, bound): out[ngt,npol',ngf,nbin] and wout[ngt,ngf] as pp_scrunch defines them, and per element
    bound = (n + 2) 2^-53 sum|w x| / sum w, n the cell's live member count (0 for dead cells): what a sequential f64
    sum of n products and one division may differ by under any contraction of its multiply-adds."""
    x = np.asarray(ports)
    if x.ndim == 3:
        x = x[:, None]
    x = x.astype(np.float64)
    nsub, npol, nchan, nbin = x.shape
    w = np.broadcast_to(np.asarray(weights, dtype=np.float64), (nsub, nchan))
    t_off = np.arange(nsub + 1) if t_off is None else np.asarray(t_off)
    f_off = np.arange(nchan + 1) if f_off is None else np.asarray(f_off)
    ngt, ngf = len(t_off) - 1, len(f_off) - 1
    npo = npol if pol_mode == "keep" else 1
    out = np.zeros((ngt, npo, ngf, nbin))
    absum = np.zeros((ngt, npo, ngf, nbin))
    wout = np.zeros((ngt, ngf))
    bound = np.zeros((ngt, npo, ngf, nbin))
    for gt in range(ngt):
        for gf in range(ngf):
            members = [(s, c) for s in range(t_off[gt], t_off[gt + 1]) for c in range(f_off[gf], f_off[gf + 1])
                       if live(w[s, c])]
            W = 0.0
            for s, c in members:
                W += w[s, c]
            if not W > 0.0:
                continue
            wout[gt, gf] = W
            for p in range(npo):
                acc = np.zeros(nbin)
                ab = np.zeros(nbin)
                for s, c in members:
                    if pol_mode == "sum01":
                        acc = acc + w[s, c] * (x[s, 0, c] + x[s, 1, c])
                        ab = ab + abs(w[s, c]) * (np.abs(x[s, 0, c]) + np.abs(x[s, 1, c]))
                    else:
                        acc = acc + w[s, c] * x[s, p, c]
                        ab = ab + abs(w[s, c]) * np.abs(x[s, p, c])
                out[gt, p, gf] = acc / W
                absum[gt, p, gf] = ab
                bound[gt, p, gf] = (len(members) + 2) * 2.0 ** -53 * ab / W
    return out, wout, bound


def group_offsets(n, ngroups):
    """Offsets of `ngroups` contiguous groups of n members, as equal as can be, the larger ones first."""
    q, r = divmod(n, ngroups)
    sizes = [q + 1] * r + [q] * (ngroups - r)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


DCONST = 0.000241 ** -1          # pplib.Dconst


class NumpyEngine(object):
    """The four device calls the archive operations make, in NumPy (a stand-in for the engine in tests without a GPU;
    noise is the plain standard deviation); `log` records them in order."""
    device = 0

    def __init__(self):
        self.log = []

    def scrunch(self, ports, weights, t_off=None, f_off=None, pol_mode="keep"):
        x = np.asarray(ports)
        self.log.append(("scrunch", None if t_off is None else len(t_off) - 1, None if f_off is None else len(f_off) - 1, pol_mode))
        out, wout, _ = scrunch_ref(x, weights, t_off, f_off, pol_mode)
        return (out[:, 0] if x.ndim == 3 else out), wout

    def rotate_portraits(self, ports, freqs, P, phi=0.0, DM=0.0, GM=0.0, nu_DM=np.inf, nu_GM=np.inf):
        x = np.asarray(ports, dtype=np.float64)
        nsub, nchan, nbin = x.shape
        self.log.append(("rotate", float(DM), float(nu_DM)))
        freqs = np.broadcast_to(np.asarray(freqs, dtype=np.float64), (nsub, nchan))
        P = np.broadcast_to(np.asarray(P, dtype=np.float64), (nsub,))
        delay = DCONST * DM * (freqs ** -2.0 - float(nu_DM) ** -2.0) / P[:, None] + phi
        k = np.arange(nbin // 2 + 1)
        return np.fft.irfft(np.fft.rfft(x, axis=-1) * np.exp(2j * np.pi * k * delay[..., None]), n=nbin, axis=-1)

    def channel_noise(self, ports, norm=None, weights=None):
        x = np.asarray(ports, dtype=np.float64)
        self.log.append(("noise", x.shape))
        return x.std(axis=-1), np.ones(x.shape[:-1])

    def channel_snrs(self, ports, fudge=3.25):
        x = np.asarray(ports, dtype=np.float64)
        s = x.std(axis=-1)
        return np.where(s > 0, x.max(axis=-1) / np.where(s > 0, s, 1.0), 0.0)
