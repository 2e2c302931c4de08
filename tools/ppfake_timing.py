#!/usr/bin/env python3
"""Time Engine.fake_portraits at 64 x 1 x 4096 x 2048 in f32 and f64 on the GPU and write profiles/ppfake_timing.json:

    python tools/ppfake_timing.py [--out profiles/ppfake_timing.json]

Each figure is the host clock around calls that end in a device synchronise (pp_fake_portraits waits for its stream),
after two warm-up calls: seconds per call over windows of 20 calls, the median of seven windows.  Bytes written per second = the bytes of the destination over that time,
beside the chip's measured streaming rate.  What bounds the kernel is read off two variants of the same call -- without
noise (sigmas None: the rotated harmonics, the inverse transform and the store) and with noise (Philox, log and
sincospi per pair of samples on top) -- and off the least time the store alone could take.  The NumPy composition (rfft phasor irfft plus normal deviates) is timed for ONE subint of that shape.
Without a GPU this fails; it does not fall back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_STREAM_TBS = 6.29          # float4 copy, measured; 8.0 by the data sheet
NSUB, NPOL, NCHAN, NBIN = 64, 1, 4096, 2048


CALLS = 20         # calls per timed window: ~0.1 s of device work


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppfake_timing.json"))
    opts = ap.parse_args()
    import torch
    from pulseportraiture_amd.engine import Engine
    from pulseportraiture_amd.gmodel import gaussian_portrait, read_gmodel
    if not torch.cuda.is_available():
        raise SystemExit("ppfake_timing: no GPU")
    eng = Engine(0)
    model = read_gmodel(os.path.join(ROOT, "tests", "golden", "example.gmodel"))
    P = 1.0 / 345.67890123456789
    freqs = np.linspace(1100.0 + 400.0 / NCHAN, 1900.0 - 400.0 / NCHAN, NCHAN)
    eng.set_model_gaussian(model, freqs, NBIN, P=P, slot=0)
    rng = np.random.default_rng(1)
    delays = rng.uniform(-0.5, 0.5, (NSUB, NCHAN))
    amps = rng.uniform(0.5, 1.5, (NSUB, NPOL, NCHAN))
    sigmas = np.full(NCHAN, 1.5)
    out = dict(shape=[NSUB, NPOL, NCHAN, NBIN], device=torch.cuda.get_device_name(0), hbm_stream_TBps=HBM_STREAM_TBS,
               method="host clock around windows of %d synchronous calls, seconds per call, median of 7 windows after 2 warm-up calls" % CALLS, runs={})
    for name, tdt in (("f32", torch.float32), ("f64", torch.float64)):
        dst = torch.empty((NSUB, NPOL, NCHAN, NBIN), dtype=tdt, device="cuda:0")
        nbytes = dst.numel() * dst.element_size()
        for variant, sg in (("noise", sigmas), ("no_noise", None)):
            med, lo, hi = timed(lambda: eng.fake_portraits(dst, delays, amps=amps, sigmas=sg, seed=7))
            out["runs"]["%s_%s" % (name, variant)] = dict(
                seconds=med, seconds_min=lo, seconds_max=hi, bytes_written=nbytes, TB_per_s=nbytes / med / 1e12,
                share_of_stream_rate=nbytes / med / 1e12 / HBM_STREAM_TBS, samples_per_s=dst.numel() / med)
        del dst
    r = out["runs"]
    for name in ("f32", "f64"):
        full, bare = r[name + "_noise"], r[name + "_no_noise"]
        store = full["bytes_written"] / (HBM_STREAM_TBS * 1e12)       # the least time the store alone could take
        parts = dict(store_at_stream_rate_seconds=store, transform_and_store_seconds=bare["seconds"],
                     noise_arithmetic_seconds=full["seconds"] - bare["seconds"])
        what = "the noise arithmetic (Philox, log, sincospi)" if parts["noise_arithmetic_seconds"] > bare["seconds"] else \
            "the store" if store > 0.5 * full["seconds"] else \
            "the rotated harmonics and the inverse transform (what the call without noise takes)"
        out["bound_" + name] = dict(parts, largest_share=what, summary=(
            "%.2f ms a call: %.2f ms without noise (rotated harmonics, inverse transform, store), %.2f ms more for the noise "
            "arithmetic; the store alone would take %.2f ms at the streaming rate (%.0f %% of the call)" %
            (1e3 * full["seconds"], 1e3 * bare["seconds"], 1e3 * parts["noise_arithmetic_seconds"], 1e3 * store,
             100 * store / full["seconds"])))
    # the NumPy composition of one subint
    port = gaussian_portrait(model, freqs, NBIN, P)

    def numpy_subint():
        k = np.arange(NBIN // 2 + 1)
        rows = np.fft.irfft(np.fft.rfft(port, axis=-1) * np.exp(-2.0j * np.pi * np.outer(delays[0], k)), axis=-1)
        return amps[0, 0][:, None] * rows + sigmas[:, None] * rng.standard_normal(rows.shape)
    med, lo, hi = timed(numpy_subint, reps=3, warm=1, calls=1)
    out["numpy_one_subint_seconds"] = med
    out["numpy_64_subints_seconds_extrapolated"] = med * NSUB
    eng.close()
    with open(opts.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
