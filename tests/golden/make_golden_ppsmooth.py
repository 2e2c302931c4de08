#!/usr/bin/env python3
"""Wavelet-smoothing goldens from the TRUE reference: its pplib.py / ppspline.py converted to Python 3
(make_golden.import_reference, make_golden_ppspline.import_ppspline), with tests/wavelet_ref.PYWT standing in for
PyWavelets -- put into sys.modules['pywt'] BEFORE the reference is imported, so that its own `import pywt as pw`
finds it.  The reference's control flow (threshold scale, brute + fmin, level choice, zeroing, significance,
make_spline_model(smooth=True)) is its own; only swt, iswt and threshold are the stand-in's.

    ppsmooth_wavelet.npz   wavelet_smooth at ppsmooth_cases.WAVELET_CASES x THRESHTYPES x FACTS
    ppsmooth_smart.npz     smart_smooth of ppsmooth_cases.SMART_CASES, an all-zero row and an odd-length row, with the
                           level, factor and evaluation count read off the reference's own calls
    ppsmooth_model_<case>.npz  find_significant_eigvec(return_smooth=True) and make_spline_model(smooth=True)

The script asserts the pass condition at threshold ties: at every factor the reference evaluated, no coefficient
lies within 1e-9 lopt of lopt.

Build-container only (needs the reference sources)."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from tests import wavelet_ref as wr  # noqa: E402

sys.modules["pywt"] = wr.PYWT
import make_golden as mg  # noqa: E402
import make_golden_ppspline as mgs  # noqa: E402
from tests import ppsmooth_cases as sc  # noqa: E402
from tests import ppspline_cases as pc  # noqa: E402

TIE = 1e-9


class Recorder(object):
    """Logs the reference's calls of wavelet_smooth: (nlevel, fact, from the objective?)."""

    def __init__(self, pplib, hard=True):
        self.hard = hard           # (a soft threshold is continuous: no decision hangs on a coefficient at lopt)
        self.pplib, self.log, self.in_obj, self.vals, self.smoothed = pplib, [], False, [], []
        self.true_ws, self.true_obj, self.true_ss = pplib.wavelet_smooth, pplib.fit_wavelet_smooth_function, pplib.smart_smooth
        pplib.wavelet_smooth = self.ws
        pplib.fit_wavelet_smooth_function = self.obj
        pplib.smart_smooth = self.ss

    def ss(self, port, *a, **k):
        out = self.true_ss(port, *a, **k)
        self.smoothed.append(np.array(out))
        return out

    def ws(self, port, wavelet='db8', nlevel=5, threshtype='hard', fact=1.0):
        self.log.append((int(nlevel), float(np.asarray(fact).reshape(-1)[0]), self.in_obj, np.array(port, dtype=np.float64)))
        return self.true_ws(port, wavelet=wavelet, nlevel=nlevel, threshtype=threshtype, fact=fact)

    def obj(self, *a, **k):
        self.in_obj = True
        try:
            v = self.true_obj(*a, **k)
            self.vals.append((int(a[3]), float(v)))
            return v
        finally:
            self.in_obj = False

    def close(self):
        self.pplib.wavelet_smooth, self.pplib.fit_wavelet_smooth_function = self.true_ws, self.true_obj
        self.pplib.smart_smooth = self.true_ss

    def rows(self):
        """Per smart_smooth'ed profile (in call order): (level, fact, nfev, worst tie margin)."""
        out, nfev, margin = [], 0, np.inf
        for nlevel, fact, in_obj, prof in self.log:
            if self.hard:
                margin = min(margin, wr.tie_margin(prof, nlevel, [fact]))
            if in_obj:
                nfev += 1
            else:
                out.append((nlevel, fact, nfev, margin))
                nfev, margin = 0, np.inf
        return out


def wavelet_golden(ref):
    store = {}
    for nbin, nlevel in sc.WAVELET_CASES:
        x = sc.wavelet_input(nbin)
        store["in_%d" % nbin] = x
        m = wr.tie_margin(x, nlevel, [f for f in sc.FACTS if f > 0])
        assert m > TIE, (nbin, nlevel, m)
        worst = 0.0
        for tt in sc.THRESHTYPES:
            for fact in sc.FACTS:
                y = ref.wavelet_smooth(x, wavelet='db8', nlevel=nlevel, threshtype=tt, fact=fact)
                store["out_%d_%d_%s_%g" % (nbin, nlevel, tt, fact)] = y
                # the restatement's two inverse forms on this input: what the value tolerance is ten times of
                alt = wr.wavelet_smooth(x, nlevel, tt, fact, inverse=wr.iswt_adjoint)
                worst = max(worst, np.abs(alt - y).max() / np.abs(x).max())
        store["forms_%d_%d" % (nbin, nlevel)] = worst
        print("    wavelet %5d x %2d  tie margin %.2e  inverse forms differ by %.2e" % (nbin, nlevel, m, worst))
    mg.save("ppsmooth_wavelet", **store)


def smart_golden(ref, pplib):
    store = {}
    inputs = {name: sc.smart_input(name) for name in sc.SMART_CASES}
    inputs["zeros"] = np.zeros(256)
    inputs["odd"] = sc.profile(255, 30.0, 4205)
    for name, x in inputs.items():
        rec = Recorder(pplib, sc.SMART_CASES.get(name, (0, 0, 0, 'hard'))[3] == 'hard')
        try:
            tt = sc.SMART_CASES[name][3] if name in sc.SMART_CASES else "hard"
            y = pplib.smart_smooth(x.copy(), rchi2_tol=0.1, threshtype=tt)
        finally:
            rec.close()
        rows = rec.rows()
        store["in_" + name], store["out_" + name] = x, y
        if rows:
            level, fact, nfev, margin = rows[0]
            assert margin > TIE, (name, margin)
            levels_ok = sorted({lv for lv, v in rec.vals if v != 0})
        else:
            level, fact, nfev, margin, levels_ok = 0, 0.0, 0, np.inf, []
        store["level_" + name], store["fact_" + name], store["nfev_" + name] = level, fact, nfev
        store["zeroed_" + name] = not np.any(y)
        store["valid_levels_" + name] = np.array(levels_ok, dtype=int)
        print("    smart %-10s level %d fact %.6f nfev %d zeroed %s valid levels %s tie margin %.2e" %
              (name, level, fact, nfev, not np.any(y), levels_ok, margin))
    mg.save("ppsmooth_smart", **store)


def model_golden(ref, refspl, pplib, name):
    kw = pc.CASES[name][5]
    port, freqs, weights, bw = pc.make_input(name)
    o, ok, snrs, noise = mgs.ref_object(ref, port, freqs, weights, bw, name)
    rec = Recorder(pplib)
    try:
        refspl.DataPortrait.make_spline_model(o, smooth=True, quiet=True, **kw)
    finally:
        rec.close()
    rows = rec.rows()           # the examined eigenvectors in order, then the mean profile
    assert all(r[3] > TIE for r in rows), (name, [r[3] for r in rows])
    nvec = len(rows) - 1
    ev = o.eigvec[:, :10]
    stats = np.zeros((nvec, 5))
    for iv in range(nvec):
        sm = rec.smoothed[iv]
        a = np.abs(sm)
        power = np.sum(np.abs(np.fft.rfft(sm)[1:]) ** 2)
        rawn = ref.get_noise(ev[:, iv])
        stats[iv] = [power, rawn, a.max(), ref.count_crossings(a, 0.1 * a.max()), power / (rawn * np.sqrt(len(sm) / 2.0))]
    cutoff = kw.get("snr_cutoff", 150.0)
    for lim in (cutoff, 3 * cutoff):
        assert np.all(np.abs(stats[:, 4] - lim) > 1e-6 * lim), (name, stats[:, 4])
    rx, rf = pc.sample_rows(len(ok)), pc.sample_rows(len(port))
    store = dict(freqs=freqs, weights=weights, bw=bw, SNRs=snrs, noise_stds=noise, input_sha256=np.array(pc.sha256(port)),
                 mean_prof=o.mean_prof, smooth_mean_prof=o.smooth_mean_prof, eigvec=ev, smooth_eigvec=o.smooth_eigvec[:, :10],
                 ieig=np.asarray(o.ieig, dtype=int), stats=stats, levels=np.array([r[0] for r in rows]),
                 facts=np.array([r[1] for r in rows]), nfevs=np.array([r[2] for r in rows]),
                 proj_port=np.array(o.proj_port), rows_x=rx, rows=rf, modelx_rows=np.array(o.modelx)[rx],
                 model_rows=np.array(o.model)[rf], reconst_rows=np.array(o.reconst_port)[rx])
    if o.ncomp:
        store.update(t=np.array(o.tck[0]), c=np.array(o.tck[1]), k=int(o.tck[2]), fp=float(o.fp), ier=int(o.ier))
    else:
        store.update(t=np.zeros(0), c=np.zeros((0, 0)), k=0, fp=np.nan, ier=-99)
    mg.save("ppsmooth_model_" + name, **store)
    print("    model %s ieig %s ev_snr %s levels %s nknots %d" % (name, o.ieig, np.round(stats[:, 4], 1), store["levels"], len(store["t"])))


def main():
    ref, refspl, tmp = mgs.import_ppspline()
    pplib = sys.modules["pplib"]
    assert pplib.pw is wr.PYWT, "the reference did not pick up the stand-in"
    which = sys.argv[1:] or ["wavelet", "smart", "model"]
    if "wavelet" in which:
        wavelet_golden(ref)
    if "smart" in which:
        smart_golden(ref, pplib)
    if "model" in which:
        for name in sc.MODEL_CASES:
            model_golden(ref, refspl, pplib, name)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
