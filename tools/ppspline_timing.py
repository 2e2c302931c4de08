#!/usr/bin/env python3
"""Times ppspline on the MI355X and writes one JSON line (and profiles/ppspline_timing.json).

For 512 x 2048 (the dual side: a 512 x 512 matrix) and 4096 x 2048 (the covariance itself, 2048 x 2048), f64,
host input, the example pulsar's portrait times random gains plus noise:

  make_spline_model   wall time of DataPortrait.make_spline_model(smooth=False, max_ncomp=4), best of 3 after a
                      warm-up, and its split: the device stages (pca_gram, pca_basis, pca_project and the two model
                      portraits, each a synchronous call with its copies), numpy.linalg.eigh, splprep
  gram kernel         k_pca_gram alone by HIP events (option "profile"), and its f64 FLOP/s: the 2 x 64 x 64 x m
                      of every computed tile of the upper triangle ("executed"), and n^2 m, the multiply-adds of
                      the matrix's distinct elements ("useful")
  numpy               np.cov(delta.T, aweights=w, ddof=1) and np.linalg.eigh of it on the host's cores, in the same
                      run, for orientation: what the reference's pca spends

    python tools/ppspline_timing.py [--out profiles/ppspline_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def portrait(nchan, nbin, seed=5):
    from pulseportraiture_amd.gmodel import example_model
    from pulseportraiture_amd.pptoas import data_from_arrays
    from pulseportraiture_amd.ppspline import DataPortrait
    from pulseportraiture_amd.engine import default_engine
    rng = np.random.default_rng(seed)
    freqs, clean, P = example_model(nchan, nbin)
    port = rng.uniform(0.5, 1.5, nchan)[:, None] * clean + 0.01 * rng.standard_normal((nchan, nbin))
    eng = default_engine()
    data = data_from_arrays(port[None, None], freqs, [P], [55000.0], noise_stds=eng.channel_noise(port)[0][None, None],
                            SNRs=eng.channel_snrs(port)[None, None], bw=800.0, filename="timing.npz")
    return DataPortrait(data, quiet=True)


def best(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def shape(nchan, nbin):
    from pulseportraiture_amd.engine import default_engine
    from pulseportraiture_amd.ppspline import fit_spline_curve, significant_eigvec
    eng = default_engine()
    dp = portrait(nchan, nbin)
    res = {}
    res["make_spline_model_s"] = best(lambda: dp.make_spline_model(smooth=False, max_ncomp=4, quiet=True))[0]
    snrs = np.asarray(dp.SNRsxs)
    w = snrs / snrs.sum()
    t_gram, (mean_prof, gram, fact) = best(lambda: eng.pca_gram(dp.portx, w))
    t_eigh, (lam, vecs) = best(lambda: np.linalg.eigh(gram))
    isort = np.argsort(lam)[::-1]
    lam, vecs = lam[isort], vecs[:, isort]
    t_basis, (eigvec, stats) = best(lambda: eng.pca_basis(vecs[:, :10], lam[:10]))
    ieig = significant_eigvec(stats, nbin, return_max=4)[0]
    t_proj, (proj, reconst) = best(lambda: eng.pca_project(ieig))
    t_spl, fit = best(lambda: fit_spline_curve(proj, w, dp.freqsxs[0], dp.bw, snrs, dp.noise_stdsxs, quiet=True))
    t_model = best(lambda: eng.spline_portrait(mean_prof, eigvec[:, ieig], fit[0], dp.freqsxs[0]))[0]
    res.update(pca_gram_call_s=t_gram, pca_basis_call_s=t_basis, pca_project_call_s=t_proj, model_portrait_call_s=t_model,
               device_s=t_gram + t_basis + t_proj + 2 * t_model, eigh_s=t_eigh, splprep_s=t_spl, ncomp=len(ieig),
               matrix_order=int(gram.shape[0]), side="dual" if nchan < nbin else "covariance")
    # the Gram kernel alone
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    for _ in range(5):
        eng.pca_gram(dp.portx, w)
    secs, count = eng.kernel_times(reset=True)["pca_gram"]
    eng.set_option("profile", 0)
    n, m = (nchan, nbin) if nchan < nbin else (nbin, nchan)
    nb, mpad = (n + 63) // 64, (m + 15) // 16 * 16
    t_k = secs / count
    res["gram_kernel"] = dict(seconds=t_k, launches=int(count), tiles=nb * (nb + 1) // 2,
                              executed_f64_flops=2.0 * 64 * 64 * mpad * (nb * (nb + 1) // 2),
                              executed_f64_TFLOPs=2.0 * 64 * 64 * mpad * (nb * (nb + 1) // 2) / t_k / 1e12,
                              useful_f64_TFLOPs=float(n) * n * m / t_k / 1e12)
    # the host's pca on the same input
    delta = dp.portx - mean_prof
    t_cov, cov = best(lambda: np.cov(delta.T, aweights=w, ddof=1), reps=2)
    t_heigh = best(lambda: np.linalg.eigh(cov), reps=1)[0]
    res["numpy_same_run"] = dict(cov_s=t_cov, eigh_s=t_heigh, order=int(cov.shape[0]), threads=os.cpu_count())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppspline_timing.json"))
    a = ap.parse_args()
    res = {"%dx%d_f64" % s: shape(*s) for s in ((512, 2048), (4096, 2048))}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
