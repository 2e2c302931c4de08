#!/usr/bin/env python3
"""Times the joined Gaussian fit on the MI355X, and the unjoined fit against another checkout, and writes
profiles/ppgauss_join_timing.json.

  joined     two bands of 256 channels x 2048 bins (1100 ... 1900 MHz), five components (tools/ppgauss_timing.py's),
             white noise sigma = 0.05, every evolution parameter free but the location slopes (a common Delta-DM is
             nearly degenerate with them), tau fixed at 0; band 1's phase fixed, its Delta-DM and both of band 2's
             free.  A warm-up, then `--reps` timed fits through the engine; the kernel split by HIP events from a
             separate fit; and the same driver on gaussfit.numpy_evaluator on this box's cores, once, in the same run.
  unjoined   the 512 x 2048 five-component case of tools/ppgauss_timing.py, on this checkout and -- with --parent DIR,
             a built checkout of the parent commit -- on that one: `--rounds` fresh child processes for each,
             alternating, every one a warm-up and `--reps` timed fits.  The residual kernel gained a branch; reported
             are both medians, each side's own spread (max - min over all its fits), and whether this checkout's median
             is within the two spreads of the parent's.

    python tools/ppgauss_join_timing.py [--out profiles/ppgauss_join_timing.json] [--parent DIR] [--reps 5] [--rounds 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P = 1.0 / 345.67890123456789
JOIN_TRUTH = [0.0, 2e-4, 0.013, -3e-4]


def joined_case(nchan_band=256, nbin=2048, seed=12):
    from pulseportraiture_amd import gmodel
    import ppgauss_timing as pt
    mdl = gmodel.parse_gmodel(gmodel.EXAMPLE_GMODEL)
    truth = np.array(list(mdl["params"]) + pt.EXTRA)
    truth[1] = 0.0
    freqs = gmodel.example_model(2 * nchan_band, 8)[0]
    ichans = [np.arange(nchan_band), np.arange(nchan_band, 2 * nchan_band)]
    full = dict(params=truth, code=mdl["code"], nu_ref=mdl["nu_ref"], alpha=-4.0, ngauss=5)
    rng = np.random.default_rng(seed)
    clean = gmodel.gaussian_portrait(full, freqs, nbin, join_ichans=ichans, join_params=JOIN_TRUTH, P_join=P)
    data = clean + pt.SIGMA * rng.standard_normal(clean.shape)
    flags = np.ones(len(truth))
    flags[1] = 0
    flags[3::6] = 0
    init = np.where(flags != 0, truth * (1.0 + 0.003 * rng.standard_normal(len(truth))), truth)
    join_flags = np.array([0, 1, 1, 1])
    join_init = np.array(JOIN_TRUTH) + join_flags * np.tile([1e-5, 1e-6], 2) * rng.standard_normal(4)
    return dict(code=mdl["code"], nu_ref=float(mdl["nu_ref"]), freqs=freqs, data=data, flags=flags, init=init,
                errs=np.full(len(freqs), pt.SIGMA), join=[ichans, join_init, join_flags])


def joined_fit(c, **kw):
    from pulseportraiture_amd import gaussfit
    nbin = c["data"].shape[1]
    t0 = time.perf_counter()
    r = gaussfit.fit_gaussian_portrait(c["code"], c["data"], c["init"], -4.0, c["errs"], c["flags"], False, np.arange(nbin),
                                       c["freqs"], c["nu_ref"], join_params=c["join"], P=P, **kw)
    return time.perf_counter() - t0, r


def joined(reps):
    import ppgauss_timing as pt
    from pulseportraiture_amd import gaussfit
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    c = joined_case()
    joined_fit(c, engine=eng)                           # warm-up
    runs = [joined_fit(c, engine=eng) for _ in range(reps)]
    r = runs[0][1]
    vary = np.append(c["flags"] != 0, c["join"][2] != 0)
    res = dict(nvaried=int(vary.sum()), ncomp=5, chi2_dof=r.chi2 / r.dof, jacobians=int(r.lm_results.niter),
               trial_steps=int(r.lm_results.nfev), message=r.lm_results.message, device=pt.spread([t for t, _ in runs]),
               join_params=list(r.fitted_params[-4:]), join_param_errs=list(r.fit_errs[-4:]))
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    joined_fit(c, engine=eng)
    kt = eng.kernel_times(reset=True)
    eng.set_option("profile", 0)
    res["kernels"] = {k: dict(seconds=v[0], launches=int(v[1])) for k, v in kt.items() if v[1]}
    ev = gaussfit.numpy_evaluator(c["data"], c["errs"], c["code"], c["freqs"], c["nu_ref"], c["join"][0], P)
    tn, rn = joined_fit(c, evaluator=ev)
    res["numpy_same_run"] = dict(pt.spread([tn]), jacobians=int(rn.lm_results.niter), trial_steps=int(rn.lm_results.nfev),
                                 threads=os.cpu_count(),
                                 max_distance_sigma=float(np.max(np.abs(rn.fitted_params - r.fitted_params)[vary] /
                                                                 r.fit_errs[vary])))
    return res


def unjoined_child(root, reps):
    """The wall times of the unjoined 512 x 2048 fit with the package of the checkout `root`."""
    import ppgauss_timing as pt
    sys.path.insert(0, root)                            # (in front of what ppgauss_timing put there)
    import pulseportraiture_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(pulseportraiture_amd.__file__))) == os.path.abspath(root)
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    c = pt.case(512, 2048, 5)
    pt.fit(c, engine=eng)
    runs = [pt.fit(c, engine=eng) for _ in range(reps)]
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    pt.fit(c, engine=eng)
    kt = eng.kernel_times(reset=True)
    r = runs[0][1]
    print(json.dumps(dict(times=[t for t, _ in runs], jacobians=int(r.lm_results.niter), trial_steps=int(r.lm_results.nfev),
                          chi2=r.chi2, gauss_resid_s=kt["gauss_resid"][0], gauss_resid_launches=int(kt["gauss_resid"][1]))))


def unjoined(parent, reps, rounds):
    sides = {"this": ROOT}
    if parent:
        sides["parent"] = os.path.abspath(parent)
    got = {k: [] for k in sides}
    for _ in range(rounds):
        for k, root in sides.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(reps)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode:
                raise RuntimeError("the child for %s ended with %d: %s" % (k, p.returncode, p.stderr[-2000:]))
            got[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
    import ppgauss_timing as pt
    res = {}
    for k, runs in got.items():
        t = [x for r in runs for x in r["times"]]
        res[k] = dict(pt.spread(t), spread_s=float(np.max(t) - np.min(t)), jacobians=runs[0]["jacobians"],
                      trial_steps=runs[0]["trial_steps"], chi2=runs[0]["chi2"],
                      gauss_resid_s=[r["gauss_resid_s"] for r in runs], gauss_resid_launches=runs[0]["gauss_resid_launches"])
    if parent:
        slower = res["this"]["median_s"] - res["parent"]["median_s"]
        res["this_minus_parent_median_s"] = float(slower)
        res["within_the_spreads"] = bool(slower <= res["this"]["spread_s"] + res["parent"]["spread_s"])
        res["same_chi2_bits"] = bool(res["this"]["chi2"] == res["parent"]["chi2"])
    return res


def main():
    sys.path.insert(0, HERE)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppgauss_join_timing.json"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return unjoined_child(a.child, a.reps)
    sys.path.insert(0, ROOT)
    out = {"joined_2x256x2048_5comp": joined(a.reps), "unjoined_512x2048_5comp": unjoined(a.parent, a.reps, a.rounds)}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
