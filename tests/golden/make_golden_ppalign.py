#!/usr/bin/env python3
"""ppalign goldens from the TRUE reference: its ppalign.py, converted to Python 3 in the same scratch
directory as pptoas.py (make_golden_ppzap.import_ppzap's way), and its align_archives DRIVEN as it is:
load_data is patched to hand out synthetic DataBunches, sub.Popen to answer the `vap` line, and a small
stand-in `arch` object (tscrunch, pscrunch, convert_state, set_dispersion_measure do nothing) captures what
the reference writes: get_Profile(ipol, ichan).get_amps()[:], set_weight and unload.  No step of the
function is restated.

    ppalign_same.npz      3 archives x 2-3 subints x 32 channels x 256 bins on the template's channels, some
                          zero-weight channels, a subint with one good channel (the 1-channel hack), one
                          archive of another nbin and one below the S/N cutoff (both skipped), one that
                          cannot be loaded.  Cases: niter 1 and 2, fit_dm on and off, every norm,
                          rot_phase 0.1, place 0.3.
    ppalign_same_norms.npz  the norm cases of ppalign_same.npz (its archives), a file of their own for the size limit
    ppalign_mapped.npz    a template of 16 channels, archives of 24 and 16 channels on shifted frequencies, 128 bins
    ppalign_stokes.npz    npol = 4: 2 archives x 2 x 16 x 128 and one npol = 1 archive (skipped under -p)
    ppalign_nbin1000.npz  2 archives x 2 x 12 x 1000 (a general row length)
    ppalign_guesses.npz   the constant-portrait guesses of -g 0.05 and of a 1-channel -I (gaussian_profile)
    ppalign_options.txt   the option names and defaults of the reference's parser

Integer-valued samples are stored as int16 (as ppzap_noise.npz does).  Every archive carries the noise and
S/N per channel load_data would have measured (get_noise, get_SNR), so that the package measures nothing.

Tolerance, measured: every case is also run with the channel order of all archives and of the template
reversed; `<case>_self_dev` = max |un-reversed - plain| / peak.  Noise levels and seeds are such that every
case has self_dev <= 1e-9 (asserted here), i.e. the reference is at no marginal SciPy exit.

Build-container only (needs the reference sources)."""
import contextlib
import copy
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_gettoas as mgt  # noqa: E402

GMODEL = os.path.join(mg.REF, "examples", "example.gmodel")
P0 = 1.0 / 345.67890123456789
SCALE = 200.0           # template peak in stored units: samples are rounded to integers
SELF_DEV_MAX = 1e-9
SEED = int(os.environ.get("PPALIGN_SEED", "100"))   # added to every archive's seed.  Chosen: with 0 the phase-only case of
                                                    # ppalign_same sat at a marginal exit (self_dev 2.3e-9); 100 and 200 do not


def import_ppalign():
    ref, pptoas, tmp = mgt.import_pptoas()
    shutil.copy(os.path.join(mg.REF, "ppalign.py"), tmp)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", "ppalign.py"], cwd=tmp,
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    import ppalign
    return ref, pptoas, ppalign, tmp


# ---- synthetic archives ------------------------------------------------------------------------------------
def band(nchan, lo=1100.0, hi=1900.0):
    d = (hi - lo) / nchan
    return np.linspace(lo + d / 2, hi - d / 2, nchan)


def archive(ref, seed, nsub, nchan, nbin, npol=1, sigma=4.0, freqs0=None, amp=1.0, zero=()):
    """Stored dispersed (dmc = 0) with header DM 0: the example pulsar's portrait, each subint turned by an
    injected phase and DM, white noise, rounded to integers."""
    rng = np.random.default_rng(seed + SEED)
    freqs0 = band(nchan) if freqs0 is None else freqs0
    phases = ref.get_bin_centers(nbin)
    sub = np.zeros((nsub, npol, nchan, nbin))
    Ps = P0 * (1 + 1e-7 * np.arange(nsub))
    inj = []
    for i in range(nsub):
        _, _, model = ref.read_model(GMODEL, phases, freqs0, Ps[i], quiet=True)
        phi, dDM = rng.uniform(-0.3, 0.3), rng.normal(0.0, 4e-4)
        port = SCALE * amp * ref.rotate_data(model, -phi, -dDM, Ps[i], freqs0, 1500.0)
        for ipol in range(npol):
            f = 1.0 if ipol == 0 else (0.4, -0.3, 0.15)[ipol - 1]
            sub[i, ipol] = np.rint(f * port + sigma * rng.standard_normal(port.shape))
        inj.append([phi, dDM])
    weights = np.ones((nsub, nchan))
    for i, n in zero:
        weights[i, n] = 0.0
    return dict(subints=sub.astype(np.int16), freqs=np.tile(freqs0, (nsub, 1)), weights=weights, Ps=Ps,
                inj=np.array(inj))


def bunch(ref, a, name, prof_SNR=1000.0, flip=False):
    """The DataBunch load_data would return for archive `a` (pplib.py:2650-2814); flip: channel order reversed."""
    sub = a["subints"].astype(np.float64)
    freqs, weights = a["freqs"].copy(), a["weights"].copy()
    if flip == "bins":
        sub = sub[..., ::-1].copy()
    elif flip:
        sub, freqs, weights = sub[:, :, ::-1].copy(), freqs[:, ::-1].copy(), weights[:, ::-1].copy()
    nsub, npol, nchan, nbin = sub.shape
    noise = np.zeros((nsub, npol, nchan))
    snrs = np.zeros((nsub, npol, nchan))
    for i in range(nsub):
        for ip in range(npol):
            noise[i, ip] = ref.get_noise(sub[i, ip], chans=True)
            snrs[i, ip] = [ref.get_SNR(sub[i, ip, n]) for n in range(nchan)]
    ok_ichans = [np.compress(weights[i] > 0, np.arange(nchan)) for i in range(nsub)]
    ok_isubs = np.compress((weights > 0).sum(axis=1), np.arange(nsub))
    masks = np.einsum('ij,k', (weights > 0).astype(float), np.ones(nbin))[:, None].repeat(npol, axis=1)
    return ref.DataBunch(subints=sub, freqs=freqs, weights=weights, Ps=a["Ps"], noise_stds=noise, SNRs=snrs,
                         ok_ichans=ok_ichans, ok_isubs=ok_isubs, masks=masks, nsub=nsub, npol=npol, nchan=nchan,
                         nbin=nbin, DM=0.0, dmc=0, prof_SNR=prof_SNR, filename=name, arch=None)


# ---- the stand-ins ------------------------------------------------------------------------------------------
class Capture(object):
    """The `arch` of the initial guess: what align_archives writes into it."""
    def __init__(self, npol, nchan, nbin):
        self.amps = np.zeros((npol, nchan, nbin))
        self.weights = np.full(nchan, np.nan)
        self.outfile = None
        self.calls = []

    def tscrunch(self): self.calls.append("tscrunch")
    def pscrunch(self): self.calls.append("pscrunch")
    def convert_state(self, s): self.calls.append("convert_state " + s)
    def set_dispersion_measure(self, dm): self.calls.append("set_dispersion_measure %r" % dm)
    def get_npol(self): return self.amps.shape[0]
    def get_nchan(self): return self.amps.shape[1]
    def __iter__(self): return iter([self])
    def get_Profile(self, ipol, ichan):
        cap = self

        class Prof(object):
            def get_amps(self): return cap.amps[ipol, ichan]
        return Prof()

    def set_weight(self, ichan, w): self.weights[ichan] = w
    def unload(self, outfile): self.outfile = outfile


def run_reference(ref, ppalign, archives, guess, flip=False, **kw):
    """The TRUE align_archives over `archives` ({name: archive dict or an exception class}) with the initial guess
    `guess` (an archive dict); returns (amps, weights, stdout, calls)."""
    pscrunch = kw.get("pscrunch", True)
    cap = {}

    def load_data(name, **opts):
        a = guess if name == "guess.fits" else archives[name]
        if isinstance(a, type):
            raise a(name)
        d = bunch(ref, a, name, prof_SNR=a.get("prof_SNR", 1000.0), flip=flip)
        if not opts["pscrunch"] and d.npol == 1:
            raise IndexError(name)                       # (load_data indexes polarisation 3 of the Stokes state)
        if opts["pscrunch"] and d.npol > 1:              # Stokes I
            for k in ("subints", "noise_stds", "SNRs", "masks"):
                d[k] = d[k][:, :1]
            d.npol = 1
        if opts.get("return_arch"):
            cap["arch"] = d.arch = Capture(1 if opts["pscrunch"] else 4, d.nchan, d.nbin)
        return d

    class Popen(object):
        def __init__(self, *a, **k):
            g = guess["subints"].shape
            self.stdout = io.BytesIO(b"filename nchan nbin\nguess.fits %d %d\n" % (g[2], g[3]))

    ppalign.load_data, old_popen = load_data, ppalign.sub.Popen
    ppalign.sub.Popen = Popen
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            ppalign.align_archives([n for n in archives], "guess.fits", outfile="out.fits", **kw)
    finally:
        ppalign.sub.Popen = old_popen
    c = cap["arch"]
    assert c.outfile == "out.fits" and not np.isnan(c.weights).any()
    if flip == "bins":
        return c.amps[..., ::-1].copy(), c.weights, buf.getvalue(), c.calls
    amps = c.amps[:, ::-1].copy() if flip else c.amps
    return amps, (c.weights[::-1].copy() if flip else c.weights), buf.getvalue(), c.calls


def run_cases(ref, ppalign, archives, guess, cases, flip=True):
    out, meta, bad = {}, {}, []
    for name, kw in cases.items():
        amps, w, text, calls = run_reference(ref, ppalign, copy.deepcopy(archives), guess, **kw)
        ramps, rw, _, _ = run_reference(ref, ppalign, copy.deepcopy(archives), guess, flip=flip, **kw)
        peak = np.abs(amps).max()
        dev = float(np.abs(ramps - amps).max() / peak)
        assert np.array_equal(w, rw)
        print("%-28s peak %.4g self_dev %.2e  %s" % (name, peak, dev, text.replace("\n", " | ")[:150]))
        bad = bad + [(name, dev)] if dev > SELF_DEV_MAX else bad
        out[name + "_amps"], out[name + "_weights"], out[name + "_self_dev"] = amps, w, dev
        meta[name] = dict(kwargs=kw, stdout=text, arch_calls=calls)
    assert not bad, bad
    return out, meta


def store(fname, archives, guess, out, meta, only=None, with_archives=True):
    """(only: the cases whose names start with one of these; with_archives=False: a file of cases whose archives are in
    another golden -- a file of every case of ppalign_same would pass the size limit of a committed file)"""
    keep = lambda name: only is None or name.startswith(tuple(only))      # noqa: E731
    arrays = {k: v for k, v in out.items() if keep(k)}
    meta = {k: v for k, v in meta.items() if keep(k)}
    for name, a in (list(archives.items()) + [("guess.fits", guess)]) if with_archives else []:
        if isinstance(a, type):
            meta.setdefault("_unloadable", []).append(name)
            continue
        for k in ("subints", "freqs", "weights", "Ps", "inj"):
            arrays["%s__%s" % (name, k)] = a[k]
        arrays["%s__prof_SNR" % name] = a.get("prof_SNR", 1000.0)
        b = bunch(REFMOD[0], a, name)                 # what load_data measures: get_noise, get_SNR of every row
        arrays["%s__noise_stds" % name], arrays["%s__SNRs" % name] = b.noise_stds, b.SNRs
    arrays["archive_names"] = np.array([n for n in archives])
    arrays["meta"] = json.dumps(dict(cases=meta, driven="the true align_archives, no step restated",
                                     **mg.versions()))
    path = os.path.join(HERE, fname)
    np.savez_compressed(path, **arrays)
    print(fname, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 660000


NORMS = ["mean", "max", "prof", "rms", "abs"]
REFMOD = []


def main():
    ref, pptoas, ppalign, tmp = import_ppalign()
    REFMOD.append(ref)
    # ---- same frequencies ----
    guess = archive(ref, 11, 1, 32, 256, sigma=1.0, zero=[(0, 3), (0, 17)])
    archives = {
        "a0.fits": archive(ref, 21, 3, 32, 256, zero=[(0, 5), (1, 5), (1, 30), (2, 3)]),
        "missing.fits": RuntimeError,
        "a1.fits": archive(ref, 22, 2, 32, 256, amp=0.7, zero=[(1, n) for n in range(32) if n != 12]),   # the hack
        "short.fits": archive(ref, 23, 2, 32, 128),
        "faint.fits": dict(archive(ref, 24, 2, 32, 256, amp=0.05), prof_SNR=7.0),
        "a2.fits": archive(ref, 25, 3, 32, 256, amp=1.4, zero=[(0, 0), (2, 31)]),
    }
    cases = {"niter1": dict(SNR_cutoff=10.0), "niter2": dict(SNR_cutoff=10.0, niter=2),
             "nodm": dict(SNR_cutoff=10.0, fit_dm=False), "nodm_niter2": dict(SNR_cutoff=10.0, fit_dm=False, niter=2),
             "rot": dict(SNR_cutoff=10.0, rot_phase=0.1), "place": dict(SNR_cutoff=10.0, place=0.3),
             "quiet": dict(SNR_cutoff=10.0, quiet=True)}
    for n in NORMS:
        cases["norm_" + n] = dict(SNR_cutoff=10.0, norm=n)
    cases["norm_prof_niter2"] = dict(SNR_cutoff=10.0, norm="prof", niter=2)      # the command line's test
    out, meta = run_cases(ref, ppalign, archives, guess, cases)
    store("ppalign_same.npz", archives, guess, out, meta, only=[c for c in cases if not c.startswith("norm_")])
    store("ppalign_same_norms.npz", archives, guess, out, meta, only=["norm_"], with_archives=False)
    # ---- other channels than the template's: nearest template channel, several data channels per template row and
    # rows nothing lands on.  The second run reverses the BINS here, not the channels: of the data channels of one
    # subint that share a template row the reference keeps the last one only (its indexed += is buffered, ppalign.py:
    # 204-208), so a reversed channel order is another average, not another rounding of this one
    guess = archive(ref, 51, 1, 16, 128, sigma=1.0, freqs0=band(16, 1100.0, 1900.0))
    archives = {"m0.fits": archive(ref, 52, 2, 24, 128, freqs0=band(24, 1130.0, 1670.0), zero=[(0, 7), (1, 20)]),
                "m1.fits": archive(ref, 53, 2, 16, 128, freqs0=band(16, 1217.0, 1817.0), amp=1.2, zero=[(1, 3)])}
    cases = {"mapped": dict(), "mapped_niter2": dict(niter=2), "mapped_nodm": dict(fit_dm=False)}
    out, meta = run_cases(ref, ppalign, archives, guess, cases, flip="bins")
    meta["_self_dev"] = "second run with the phase bins reversed (see make_golden_ppalign.py)"
    # the channel selection of every subint by the reference's own expressions (ppalign.py:166-172), for the CPU test
    gf = guess["freqs"][0]
    for name, a in archives.items():
        for isub in range(len(a["subints"])):
            ichans = np.compress(a["weights"][isub] > 0, np.arange(a["weights"].shape[1]))
            out["%s__ichans_%d" % (name, isub)] = ichans
            out["%s__model_ichans_%d" % (name, isub)] = np.array([np.argmin(abs(gf - a["freqs"][isub, c])) for c in ichans])
    store("ppalign_mapped.npz", archives, guess, out, meta, only=list(cases) + [n + "__" for n in archives])
    # ---- Stokes ----
    guess = archive(ref, 31, 1, 16, 128, npol=4, sigma=1.0)
    archives = {"s0.fits": archive(ref, 32, 2, 16, 128, npol=4, zero=[(0, 2)]),
                "intensity.fits": archive(ref, 33, 2, 16, 128),
                "s1.fits": archive(ref, 34, 2, 16, 128, npol=4, amp=1.3, zero=[(1, 9)])}
    cases = {"stokes": dict(pscrunch=False), "stokes_niter2_norm": dict(pscrunch=False, niter=2, norm="max"),
             "stokes_rot": dict(pscrunch=False, rot_phase=0.1), "intensity_of_stokes": dict()}
    store("ppalign_stokes.npz", archives, guess, *run_cases(ref, ppalign, archives, guess, cases))
    # ---- a general row length ----
    guess = archive(ref, 41, 1, 12, 1000, sigma=1.0)
    archives = {"n0.fits": archive(ref, 42, 2, 12, 1000, zero=[(1, 4)]),
                "n1.fits": archive(ref, 43, 2, 12, 1000, amp=0.8)}
    cases = {"nbin1000": dict(), "nbin1000_niter2_place": dict(niter=2, place=0.3)}
    store("ppalign_nbin1000.npz", archives, guess, *run_cases(ref, ppalign, archives, guess, cases))
    # ---- constant-portrait guesses: the profiles make_constant_portrait is given ----
    np.savez_compressed(os.path.join(HERE, "ppalign_guesses.npz"),
                        g005_256=ref.gaussian_profile(256, 0.5, 0.05), g005_1000=ref.gaussian_profile(1000, 0.5, 0.05),
                        one_channel_profile=SCALE * ref.gaussian_profile(256, 0.4, 0.03),
                        place_delta_256=ref.gaussian_profile(256, 0.3, 0.0001))
    # ---- the parser's options ----
    src = open(os.path.join(tmp, "ppalign.py")).read()
    ns = {}
    import optparse
    import re
    body = src[src.index("    parser = OptionParser(usage)"):src.index("    (options, args) = parser.parse_args()")]
    exec("from optparse import OptionParser\nusage=''\n" + re.sub(r"^    ", "", body, flags=re.M), ns)
    with open(os.path.join(HERE, "ppalign_options.txt"), "w") as f:
        for o in ns["parser"].option_list:
            if o.dest:
                f.write("%s\t%s\t%s\t%r\n" % (",".join(o._short_opts + o._long_opts), o.dest, o.action, o.default))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
