#!/usr/bin/env python3
"""Time Engine.fit_residuals at 64 x 1 x 4096 x 2048 in f32 and f64, from a device tensor, and write
profiles/ppresid_timing.json:

    python tools/ppresid_timing.py [--out profiles/ppresid_timing.json]

Per dtype, on one tensor and one machine: fit_residuals(want=("resid",)) -- the command's call: the row read once, its
two transforms, one template row from L2 --, the three-output call (want = port, model, resid: three inverse
transforms and three stores), the four-output call, Engine.rotate_portraits alone (the same two transforms and one
store, in place) and Engine.channel_red_chi2 alone (one transform, no store), the last two as they were before this
entry point existed.  Each figure is the host clock around calls that end in a device synchronise, after two warm-up
calls: seconds per call over windows of 10 calls, the median (and the extremes) of seven windows; beside it the
kernel's own time from HIP events round its launch (option profile; families "fit_resid", "synth", "finalize").
fit_residuals allocates its outputs (torch.empty, from the caching allocator after the warm-up); rotate_portraits
writes in place.  The ratio of the residual-only call to rotate_portraits is reported, not gated.
Without a GPU this fails; it does not fall back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSUB, NPOL, NCHAN, NBIN = 64, 1, 4096, 2048
CALLS = 10


def timed(fn, reps=7, warm=2, calls=CALLS):
    """Seconds per call: the median (and the extremes) over `reps` windows of `calls` synchronous calls each."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ts.append((time.perf_counter() - t0) / calls)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_seconds(eng, fn, family):
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    for _ in range(CALLS):
        fn()
    eng.synchronize()
    sec, n = eng.kernel_times(reset=True)[family]
    eng.set_option("profile", 0)
    return sec / max(n, 1)


def measure():
    import torch
    from pulseportraiture_amd.engine import Engine
    from tests import rot_refs as rr
    if not torch.cuda.is_available():
        raise SystemExit("ppresid_timing: no GPU")
    eng = Engine(0)
    rng = np.random.default_rng(20260101)
    freqs = np.linspace(1100.0, 1900.0, NCHAN)
    template = np.stack([rr.gauss_profile(NBIN, 0.3 + 0.02 * n / NCHAN, 0.03) + 0.4 * rr.gauss_profile(NBIN, 0.6, 0.08)
                         for n in range(NCHAN)])
    eng.set_model(template, slot=0)
    P = np.full(NSUB, 0.004)
    params = np.zeros((NSUB, 5))
    params[:, 0] = rng.uniform(-0.5, 0.5, NSUB)
    params[:, 1] = rng.normal(0.0, 1e-3, NSUB)
    nu_refs = np.tile([1500.0, np.inf, np.inf], (NSUB, 1))
    scales = rng.uniform(0.5, 2.0, (NSUB, NCHAN))
    errs = np.full((NSUB, NCHAN), 0.1)
    runs = {}
    for name, tdt in (("f32", torch.float32), ("f64", torch.float64)):
        gen = torch.Generator(device="cuda:0").manual_seed(7)
        src = torch.as_tensor(template, dtype=tdt, device="cuda:0").repeat(NSUB, 1, 1).contiguous()
        src += 0.1 * torch.randn(src.shape, dtype=tdt, device="cuda:0", generator=gen)
        nbytes = src.numel() * src.element_size()
        common = (src, freqs, P, params, nu_refs, scales)
        calls = [
            ("resid_only", lambda: eng.fit_residuals(*common, want=("resid",)), "fit_resid", 2),
            ("three_outputs", lambda: eng.fit_residuals(*common, want=("port", "model", "resid")), "fit_resid", 4),
            ("four_outputs", lambda: eng.fit_residuals(*common, errs=errs, want=("port", "model", "resid", "red_chi2")),
             "fit_resid", 4),
            ("channel_red_chi2", lambda: eng.channel_red_chi2(src, freqs, P, params, nu_refs, scales, errs), "finalize", 1),
            # (last: it turns the tensor in place)
            ("rotate_portraits", lambda: eng.rotate_portraits(src, freqs, P, phi=params[:, 0], DM=params[:, 1], nu_DM=1500.0),
             "synth", 2),
        ]
        for label, fn, family, passes in calls:
            med, lo, hi = timed(fn)
            runs["%s_%s" % (name, label)] = dict(
                seconds=med, seconds_min=lo, seconds_max=hi, kernel_seconds=kernel_seconds(eng, fn, family),
                bytes_moved=passes * nbytes, TB_per_s=passes * nbytes / med / 1e12, rows=NSUB * NCHAN,
                ns_per_row=med / (NSUB * NCHAN) * 1e9)
        rot = runs[name + "_rotate_portraits"]
        for label in ("resid_only", "three_outputs", "four_outputs"):
            r = runs["%s_%s" % (name, label)]
            r["ratio_to_rotate_portraits"] = r["seconds"] / rot["seconds"]
            r["kernel_ratio_to_rotate_portraits"] = r["kernel_seconds"] / rot["kernel_seconds"]
        del src
        torch.cuda.empty_cache()
    eng.close()
    return dict(runs=runs, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppresid_timing.json"))
    opts = ap.parse_args()
    out = dict(shape=[NSUB, NPOL, NCHAN, NBIN],
               method="host clock around windows of %d synchronous calls, seconds per call, median (min, max) of 7 windows "
                      "after 2 warm-up calls; kernel_seconds from HIP events round the launch (option profile); "
                      "bytes_moved = the portrait read once plus one portrait per stored output" % CALLS)
    out.update(measure())
    with open(opts.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
