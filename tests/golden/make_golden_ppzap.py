#!/usr/bin/env python3
"""ppzap goldens from the TRUE reference: its ppzap.py, converted to Python 3 in the same
scratch directory as pptoas.py (make_golden_gettoas.import_pptoas), run on synthetic archives
(DataBunch objects handed to a patched load_data; no PSRCHIVE).

    ppzap_noise.npz   three archives (6x64x256, 4x48x1000, 5x32x2048; integer-valued samples,
                      stored as int16): normalised channel noise and norms of the good subints
                      for every normalize_portrait method, get_zap_channels at nstd 3 and 5
                      (every method but 'rms', whose normalised noise is 1 up to rounding),
                      print_paz_cmds bytes for modify x all_subs (stdout and outfile), and the
                      stdout / -o bytes of the reference's command line (noise method)
    ppzap_model.npz   the -m flow on two archives (those of gettoas_zap.npz and archive 0 of
                      gettoas_opt_two_archives.npz) with example.gmodel: the paz bytes, which
                      list every zapped channel of every fitted subint

Build-container only (needs the reference sources)."""
import contextlib
import copy
import io
import os
import runpy
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_gettoas as mgt  # noqa: E402

NORMS = ["none", "mean", "max", "prof", "rms", "abs"]
SHAPES = [(6, 64, 256, 101), (4, 48, 1000, 102), (5, 32, 2048, 103)]
NAMES = ["arch0.npz", "arch1.npz", "arch2.npz"]
# norm 'rms' makes every normalised noise 1 up to rounding: its clip decides on rounding alone,
# so it has noise and norms here but no zap lists
CLIPPED = [n for n in NORMS if n != "rms"]
# the noise-method command lines (after -d list.txt)
CLI = [["-n", "5", "-N", "prof", "-o", "paz.txt"], ["-n", "3", "--modify"], ["-n", "3", "-N", "mean"],
       ["-n", "5", "--modify", "-o", "paz.txt"], ["-n", "5", "-N", "max"],
       ["-n", "3", "-N", "abs", "--modify"]]


def import_ppzap():
    ref, pptoas, tmp = mgt.import_pptoas()
    shutil.copy(os.path.join(mg.REF, "ppzap.py"), tmp)
    subprocess.run([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n", "ppzap.py"], cwd=tmp,
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    import ppzap
    return ref, pptoas, ppzap, tmp


def noise_archive(seed, nsub, nchan, nbin):
    rng = np.random.default_rng(seed)
    ph = (np.arange(nbin) + 0.5) / nbin
    prof = 60.0 * np.exp(-0.5 * ((ph - 0.3) / 0.02) ** 2) + 25.0 * np.exp(-0.5 * ((ph - 0.55) / 0.05) ** 2)
    amp = rng.uniform(0.5, 1.5, nchan)
    sig = np.full((nsub, nchan), 2.0)
    hot = rng.random((nsub, nchan)) < 0.08
    sig[hot] *= rng.uniform(2.0, 10.0, hot.sum())
    x = amp[None, :, None] * prof + sig[..., None] * rng.standard_normal((nsub, nchan, nbin))
    x = np.rint(x).astype(np.int16)
    weights = np.ones((nsub, nchan))
    for i in range(nsub):
        off = rng.choice(nchan, size=3, replace=False)
        weights[i, off] = 0.0
        x[i, off[0]] = 0                      # a zapped channel with no data, two that keep theirs
    x[0, 7] = 0                               # an all-zero row of weight 1
    weights[1] = 0.0                          # an all-zero-weight subint: shifts paz -w
    freqs = np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1))
    Ps = np.full(nsub, 0.003)
    return x, weights, freqs, Ps


def ref_bunch(ref, x, weights, freqs, Ps):
    sub = x.astype(np.float64)[:, None]
    nsub, _, nchan, nbin = sub.shape
    ok_ichans = [np.compress(weights[i] > 0, np.arange(nchan)) for i in range(nsub)]
    ok_isubs = np.compress((weights > 0).mean(axis=1), np.arange(nsub))
    noise = np.zeros((nsub, 1, nchan))
    for i in range(nsub):
        noise[i, 0] = ref.get_noise(sub[i, 0], chans=True)          # load_data, pplib.py:2727-2731
    return ref.DataBunch(subints=sub, weights=weights, freqs=freqs, Ps=Ps, nsub=nsub, nchan=nchan,
                         nbin=nbin, npol=1, noise_stds=noise, ok_isubs=ok_isubs, ok_ichans=ok_ichans)


def copied(ref, d):
    return ref.DataBunch(**copy.deepcopy(dict(d)))


def clip_margin(noise, ichans, nstd):
    """Smallest |noise - threshold| / |threshold| over every round of the clip."""
    ichans, worst = list(ichans), np.inf
    while len(ichans):
        v = noise[ichans]
        thr = np.median(v) + nstd * np.std(v)
        worst = min(worst, np.min(np.abs(v - thr)) / abs(thr))
        bad = set(np.where(v > thr)[0])
        if not bad:
            break
        ichans = [c for j, c in enumerate(ichans) if j not in bad]
    return worst


@contextlib.contextmanager
def captured():
    """stdout of the reference, which resets sys.stdout to sys.__stdout__ (ppzap.py:95)."""
    buf, old, old0 = io.StringIO(), sys.stdout, sys.__stdout__
    sys.stdout = sys.__stdout__ = buf
    try:
        yield buf
    finally:
        sys.stdout, sys.__stdout__ = old, old0


def run_cli(ref, pptoas, tmp, argv, bunches, files):
    """The reference's ppzap.py __main__ in a fresh directory; (stdout, outfile text)."""
    work = tempfile.mkdtemp(prefix="ppzap_cli_")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        for name, text in files.items():
            open(name, "w").write(text)
        pptoas.load_data = lambda f, *a, **k: copied(ref, bunches[f])
        pptoas.file_is_type = lambda f, t: f.endswith(".txt")
        sys.argv = ["ppzap.py"] + argv
        with captured() as buf:
            runpy.run_path(os.path.join(tmp, "ppzap.py"), run_name="__main__")
        out = open("paz.txt").read() if os.path.exists("paz.txt") else ""
        return buf.getvalue(), out
    finally:
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


def noise_golden(ref, pptoas, ppzap, tmp):
    store, bunches = {}, {}
    for ia, (nsub, nchan, nbin, seed) in enumerate(SHAPES):
        x, w, f, P = noise_archive(seed, nsub, nchan, nbin)
        d = ref_bunch(ref, x, w, f, P)
        bunches[NAMES[ia]] = d
        store.update({"a%d_subints" % ia: x, "a%d_weights" % ia: w, "a%d_freqs" % ia: f, "a%d_Ps" % ia: P,
                      "a%d_ok_isubs" % ia: np.asarray(d.ok_isubs)})
        for norm in NORMS:
            noise, norms = [], []
            for isub in d.ok_isubs:
                port = d.subints[isub, 0]
                if norm == "none":
                    pn, nv = port, np.ones(nchan)
                else:
                    pn, nv = ref.normalize_portrait(port, method=norm, weights=d.weights[isub], return_norms=True)
                noise.append(ref.get_noise(pn, chans=True))
                norms.append(nv)
            store["a%d_noise_%s" % (ia, norm)] = np.array(noise)
            store["a%d_norms_%s" % (ia, norm)] = np.array(norms)
            if norm not in CLIPPED:
                continue
            dn = copied(ref, d)
            dn.noise_stds[d.ok_isubs, 0] = np.array(noise)
            for nstd in (3, 5):
                zl = ppzap.get_zap_channels(dn, nstd=nstd)
                for isub in d.ok_isubs:
                    m = clip_margin(dn.noise_stds[isub, 0], d.ok_ichans[isub], nstd)
                    assert m > 1e-9, (ia, norm, nstd, isub, m)
                mask = np.zeros((len(d.ok_isubs), nchan), dtype=np.uint8)
                for j, z in enumerate(zl):
                    mask[j, np.asarray(z, dtype=int)] = 1
                store["a%d_zap_%s_%d" % (ia, norm, nstd)] = mask
    # print_paz_cmds on the zap lists of -N prof -n 5
    zl = [[list(np.nonzero(r)[0]) for r in store["a%d_zap_prof_5" % ia]] for ia in range(3)]
    for modify in (0, 1):
        for all_subs in (0, 1):
            with captured() as buf:
                ppzap.print_paz_cmds(NAMES, zl, all_subs=bool(all_subs), modify=bool(modify))
            store["paz_%d%d_stdout" % (modify, all_subs)] = np.array(buf.getvalue())
            work = tempfile.mkdtemp(prefix="ppzap_paz_")
            path = os.path.join(work, "paz.txt")
            open(path, "w").write("# kept\n")                        # -o appends
            with captured() as buf:
                ppzap.print_paz_cmds(NAMES, zl, all_subs=bool(all_subs), modify=bool(modify), outfile=path)
            store["paz_%d%d_file" % (modify, all_subs)] = np.array(open(path).read())
            store["paz_%d%d_file_stdout" % (modify, all_subs)] = np.array(buf.getvalue().replace(path, "OUTFILE"))
            shutil.rmtree(work, ignore_errors=True)
    with captured() as buf:
        ppzap.print_paz_cmds([], [], quiet=False)
    store["paz_nothing"] = np.array(buf.getvalue())
    listing = {"list.txt": "".join(n + "\n" for n in NAMES)}
    for k, argv in enumerate(CLI):
        out, filed = run_cli(ref, pptoas, tmp, ["-d", "list.txt"] + argv, bunches, listing)
        store["cli%d_argv" % k] = np.array(argv)
        store["cli%d_stdout" % k] = np.array(out)
        store["cli%d_file" % k] = np.array(filed)
    mg.save("ppzap_noise", **store)


def model_golden(ref, pptoas, tmp):
    """Archives: gettoas_zap.npz's (seed 35, corrupt) and gettoas_opt_two_archives.npz's first."""
    a0, _, _ = mgt.synth_archive(ref, seed=35, corrupt=True)
    a1, _, _ = mgt.synth_archive(ref, seed=41, nsub=3, DM0=34.56789)
    g0 = np.load(os.path.join(HERE, "gettoas_zap.npz"))
    g1 = np.load(os.path.join(HERE, "gettoas_opt_two_archives.npz"))
    assert np.array_equal(g0["subints"], a0.subints) and np.array_equal(g1["in0_subints"], a1.subints)
    bunches = {"zap.npz": a0, "two0.npz": a1}
    listing = {"list.txt": "zap.npz\ntwo0.npz\n"}
    model = os.path.join(mg.REF, "examples", "example.gmodel")
    store = {}
    for k, argv in enumerate([[], ["--modify", "-o", "paz.txt"]]):
        out, filed = run_cli(ref, pptoas, tmp, ["-d", "list.txt", "-m", model] + argv, bunches, listing)
        store["cli%d_argv" % k] = np.array(argv, dtype=str)
        store["cli%d_stdout" % k] = np.array(out)
        store["cli%d_file" % k] = np.array(filed)
    mg.save("ppzap_model", **store)


def main():
    ref, pptoas, ppzap, tmp = import_ppzap()
    noise_golden(ref, pptoas, ppzap, tmp)
    model_golden(ref, pptoas, tmp)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
