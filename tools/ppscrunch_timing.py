#!/usr/bin/env python3
"""Time Engine.scrunch at 64 x 1 x 4096 x 2048 in f32 and f64, from a device tensor, and write
profiles/ppscrunch_timing.json:

    python tools/ppscrunch_timing.py [--out profiles/ppscrunch_timing.json]

Two sums: tscrunch of the 64 subints to one, and fscrunch of the 4096 channels to 64.  Each figure is the host clock
around calls that end in a device synchronise (pp_scrunch waits for its stream), after two warm-up calls: seconds per
call over windows of 20 calls, the median of seven windows.  Bytes read per second = the bytes of the input over that
time, beside the chip's measured streaming rate (profiles/ppfake_timing.json); the kernel's own share of a call is
read from HIP events round its launch in 20 further calls (option profile, kernel family "scrunch").  The route that existed before for the
same sum over subints -- align_begin / align_add / align_finish with zero rotation -- is timed on the same data.
Without a GPU this fails; it does not fall back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_STREAM_TBS = 6.29          # float4 copy, measured (profiles/ppfake_timing.json); 8.0 by the data sheet
NSUB, NPOL, NCHAN, NBIN = 64, 1, 4096, 2048
NGF = 64
CALLS = 20         # calls per timed window


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppscrunch_timing.json"))
    opts = ap.parse_args()
    import torch
    from pulseportraiture_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("ppscrunch_timing: no GPU")
    eng = Engine(0)
    rng = np.random.default_rng(1)
    w = rng.uniform(0.5, 1.5, (NSUB, NCHAN))
    freqs = np.linspace(1100.0, 1900.0, NCHAN)
    P = np.full(NSUB, 0.003)
    t_off = np.array([0, NSUB], dtype=np.int32)
    f_off = np.arange(0, NCHAN + 1, NCHAN // NGF, dtype=np.int32)
    out = dict(shape=[NSUB, NPOL, NCHAN, NBIN], device=torch.cuda.get_device_name(0), hbm_stream_TBps=HBM_STREAM_TBS,
               method="host clock around windows of %d synchronous calls, seconds per call, median of 7 windows after 2 "
                      "warm-up calls" % CALLS, runs={})

    def record(name, med, lo, hi, nbytes):
        out["runs"][name] = dict(seconds=med, seconds_min=lo, seconds_max=hi, bytes_read=nbytes,
                                 TB_per_s=nbytes / med / 1e12, share_of_stream_rate=nbytes / med / 1e12 / HBM_STREAM_TBS)

    def kernel_only(name, fn, nbytes):
        """The kernel's own share of a call (HIP events round the launch, option profile): the rest is the host's --
        the member lists, their upload, the output tensor, the synchronise."""
        eng.set_option("profile", 1)
        eng.kernel_times(reset=True)
        for _ in range(CALLS):
            fn()
        eng.synchronize()
        sec, n = eng.kernel_times(reset=True)["scrunch"]
        eng.set_option("profile", 0)
        out["runs"][name].update(kernel_seconds=sec / max(n, 1), kernel_TB_per_s=nbytes / (sec / max(n, 1)) / 1e12,
                                 kernel_share_of_stream_rate=nbytes / (sec / max(n, 1)) / 1e12 / HBM_STREAM_TBS)

    for name, tdt in (("f32", torch.float32), ("f64", torch.float64)):
        src = torch.randn((NSUB, NPOL, NCHAN, NBIN), dtype=tdt, device="cuda:0")
        nbytes = src.numel() * src.element_size()
        record(name + "_tscrunch_64_to_1", *timed(lambda: eng.scrunch(src, w, t_off=t_off)), nbytes)
        kernel_only(name + "_tscrunch_64_to_1", lambda: eng.scrunch(src, w, t_off=t_off), nbytes)
        record(name + "_fscrunch_4096_to_64", *timed(lambda: eng.scrunch(src, w, f_off=f_off)), nbytes)
        kernel_only(name + "_fscrunch_4096_to_64", lambda: eng.scrunch(src, w, f_off=f_off), nbytes)

        def align_route():
            eng.align_begin(NPOL, NCHAN, NBIN)
            eng.align_add(src, freqs, P, 0.0, 0.0, np.inf, w)
            return eng.align_finish(0.0)
        record(name + "_tscrunch_by_align_add_zero_rotation", *timed(align_route), nbytes)
        del src
    eng.close()
    with open(opts.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
