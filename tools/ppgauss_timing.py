#!/usr/bin/env python3
"""Times pplib.fit_gaussian_portrait on the MI355X and writes profiles/ppgauss_timing.json.

Two shapes, f64, host input: 512 x 2048 with five components (the example pulsar's three and two more) and 64 x 512
with the example pulsar's three; white noise sigma = 0.05, every evolution parameter free, tau fixed at 0, the start the
truth times (1 + 0.003 N(0,1)).  For each:

  device   one full fit through the engine (gauss_fit_begin ... gauss_fit_end): a warm-up, then `--reps` timed fits;
           median, minimum and maximum of the wall time, the Jacobians and trial steps taken, and the kernel split by
           HIP events from Engine.kernel_times() (option "profile", a separate fit so that the events do not sit in
           the timed ones)
  numpy    the same Levenberg-Marquardt driver on gaussfit.numpy_evaluator on this box's cores in the same run: the
           baseline.  Its model is NumPy's channel-vectorised gmodel.gaussian_portrait, not the reference's Python
           loop over channels, so it flatters the reference.  One fit for the large shape, three for the small.

No ratio is fixed in advance.

    python tools/ppgauss_timing.py [--out profiles/ppgauss_timing.json] [--reps 5] [--no-numpy-large]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA = 0.05
EXTRA = [0.31, 0.002, 0.03, -0.5, 1.8, -1.2, 0.62, -0.001, 0.06, 0.8, 0.9, -0.6]      # two more components


def case(nchan, nbin, ncomp, seed=11):
    from pulseportraiture_amd import gmodel
    mdl = gmodel.parse_gmodel(gmodel.EXAMPLE_GMODEL)
    truth = np.array(list(mdl["params"]) + (EXTRA if ncomp == 5 else []))
    truth[1] = 0.0
    freqs = gmodel.example_model(nchan, 8)[0]
    full = dict(params=truth, code=mdl["code"], nu_ref=mdl["nu_ref"], alpha=-4.0, ngauss=ncomp)
    rng = np.random.default_rng(seed)
    data = gmodel.gaussian_portrait(full, freqs, nbin) + SIGMA * rng.standard_normal((nchan, nbin))
    flags = np.ones(len(truth))
    flags[1] = 0
    init = np.where(flags != 0, truth * (1.0 + 0.003 * rng.standard_normal(len(truth))), truth)
    return dict(code=mdl["code"], nu_ref=float(mdl["nu_ref"]), freqs=freqs, data=data, flags=flags, init=init,
                errs=np.full(nchan, SIGMA))


def fit(c, **kw):
    from pulseportraiture_amd import gaussfit
    nbin = c["data"].shape[1]
    t0 = time.perf_counter()
    r = gaussfit.fit_gaussian_portrait(c["code"], c["data"], c["init"], -4.0, c["errs"], c["flags"], False, np.arange(nbin),
                                       c["freqs"], c["nu_ref"], **kw)
    return time.perf_counter() - t0, r


def spread(times):
    return dict(median_s=float(np.median(times)), min_s=float(np.min(times)), max_s=float(np.max(times)), fits=len(times))


def shape(nchan, nbin, ncomp, reps, numpy_reps):
    from pulseportraiture_amd import gaussfit
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    c = case(nchan, nbin, ncomp)
    fit(c, engine=eng)                                  # warm-up
    runs = [fit(c, engine=eng) for _ in range(reps)]
    r = runs[0][1]
    res = dict(nvaried=int(np.sum(c["flags"] != 0)), ncomp=ncomp, chi2_dof=r.chi2 / r.dof, jacobians=int(r.lm_results.niter),
               trial_steps=int(r.lm_results.nfev), message=r.lm_results.message, device=spread([t for t, _ in runs]))
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    fit(c, engine=eng)
    kt = eng.kernel_times(reset=True)
    eng.set_option("profile", 0)
    res["kernels"] = {k: dict(seconds=v[0], launches=int(v[1])) for k, v in kt.items() if v[1]}
    if numpy_reps:
        ev = gaussfit.numpy_evaluator(c["data"], c["errs"], c["code"], c["freqs"], c["nu_ref"])
        nruns = [fit(c, evaluator=ev) for _ in range(numpy_reps)]
        rn = nruns[0][1]
        res["numpy_same_run"] = dict(spread([t for t, _ in nruns]), jacobians=int(rn.lm_results.niter),
                                     trial_steps=int(rn.lm_results.nfev), threads=os.cpu_count(),
                                     max_distance_sigma=float(np.max(np.abs(rn.fitted_params - r.fitted_params)[c["flags"] != 0] /
                                                                     r.fit_errs[c["flags"] != 0])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppgauss_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy-large", action="store_true")
    a = ap.parse_args()
    out = {"64x512_3comp": shape(64, 512, 3, a.reps, 3),
           "512x2048_5comp": shape(512, 2048, 5, a.reps, 0 if a.no_numpy_large else 1)}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
