#!/usr/bin/env python3
"""One alignment iteration over 8 archives x 32 subints x 512 channels x 2048 bins (f32 host arrays), two ways:
(a) align_subints per archive with the averages summed on the host -- the only route before align_archives --
and (b) align_archives with the accumulator resident on the device.  Median of 5 runs each and their spread, and the
share of the accumulator's kernels (family "synth" of Engine.kernel_times) in (b):

    python tools/ppalign_timing.py > profiles/ppalign_timing.json"""
import contextlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NARCH, NSUB, NCHAN, NBIN = 8, 32, 512, 2048


def main():
    from pulseportraiture_amd.engine import default_engine
    from pulseportraiture_amd.ppalign import align_archives, align_subints
    from pulseportraiture_amd.pptoas import data_from_arrays
    from tests.synth_host import model_portrait, P_EXAMPLE
    eng = default_engine()
    freqs, model = model_portrait(NCHAN, NBIN)
    rng = np.random.default_rng(1)
    sigma = 0.05 * model.max()
    archives = []
    for ia in range(NARCH):
        phis = rng.uniform(-0.2, 0.2, NSUB)
        sub = eng.rotate_portraits(np.broadcast_to(model, (NSUB, NCHAN, NBIN)).copy(), freqs, P_EXAMPLE, phi=-phis,
                                   DM=-rng.normal(0.0, 3e-4, NSUB), nu_DM=1500.0)
        sub = (sub + sigma * rng.standard_normal(sub.shape)).astype(np.float32)
        archives.append(data_from_arrays(sub, freqs, np.full(NSUB, P_EXAMPLE), 56000.0 + np.arange(NSUB),
                                         noise_stds=np.full((NSUB, 1, NCHAN), sigma), DM=0.0, dmc=0,
                                         filename="arch%d" % ia))
    guess = data_from_arrays(model[None], freqs, [P_EXAMPLE], [56000.0], noise_stds=np.full((1, 1, NCHAN), sigma),
                             filename="guess")

    def route_a():
        num, den = np.zeros((NCHAN, NBIN)), 0
        for d in archives:
            num += align_subints(d.subints[:, 0], d.freqs, d.Ps, d.noise_stds[:, 0], model, SNRs=d.SNRs[:, 0])
            den += 1
        return num / den

    def route_b():
        with contextlib.redirect_stdout(sys.stderr):        # ("Doing iteration 1...")
            return align_archives(archives, guess, quiet=True)[0][0]

    out = {"shape": "%dx%dx%dx%d_f32_host" % (NARCH, NSUB, NCHAN, NBIN)}
    for name, fn in (("a_align_subints_host_sum", route_a), ("b_align_archives", route_b)):
        fn()                                   # (first call: plans, twiddles, buffers)
        eng.set_option("profile", 1)
        eng.kernel_times(reset=True)
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            walls.append(time.perf_counter() - t0)
        kt = eng.kernel_times(reset=True)
        eng.set_option("profile", 0)
        out[name] = {"wall_s_median": float(np.median(walls)), "wall_s": walls,
                     "spread": float((max(walls) - min(walls)) / np.median(walls)),
                     "kernel_s_per_run": {k: v[0] / 5 for k, v in kt.items() if v[1]},
                     "synth_share_of_wall": kt.get("synth", (0.0, 0))[0] / 5 / float(np.median(walls))}
    out["note"] = ("the routes do not compute the same average: (a) is the plain mean of per-archive weighted averages, "
                   "(b) the weighted average over all subints; 'synth' holds the accumulation kernels of both routes")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
