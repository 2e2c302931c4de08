#!/usr/bin/env python3
"""Time the 'fit' noise method at 64 x 1 x 4096 x 2048 in f32 and f64, from a device tensor, and write
profiles/noisefit_timing.json:

    python tools/noisefit_timing.py [--out profiles/noisefit_timing.json] [--variant name=path.so ...]

Per dtype: Engine.channel_noise(method='fit') with fn 'exp_dc' and 'half_tri', and the power-spectrum estimate
(method='PS', pp_channel_noise as it was before) on the same tensor -- it reads each row once and does the same
transform, so the difference is the cost of the search.  Each figure is the host clock around calls that end in a
device synchronise, after two warm-up calls: seconds per call over windows of 20 calls, the median of seven windows;
for the fit also the kernel's own time from HIP events round its launch (option profile, kernel family
"noise_fit").  The rows are pulses on noise (tests/noisefit_refs.pulse_rows, tiled), not white noise alone: the
search's cost does not depend on the data, its result does, and the result is checked against the NumPy
restatement on 16 rows, which also gives the restatement's seconds per row on this machine's CPU.

--variant times other builds of the library (PP_TOAS_LIB), each in a child process of its own after this one, in
the same call: how the width-table alternatives of DESIGN.md were measured.  Without a GPU this fails; it does not fall back."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSUB, NPOL, NCHAN, NBIN = 64, 1, 4096, 2048
CALLS = 20


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


def measure(cpu_rows=16):
    import torch
    from pulseportraiture_amd.engine import Engine
    from tests import noisefit_refs as nf
    if not torch.cuda.is_available():
        raise SystemExit("noisefit_timing: no GPU")
    eng = Engine(0)
    nrows = NSUB * NPOL * NCHAN
    distinct = nf.pulse_rows(NBIN, 256, 20260101)
    runs = {}
    for name, tdt in (("f32", torch.float32), ("f64", torch.float64)):
        base = torch.as_tensor(distinct, dtype=tdt, device="cuda:0")
        src = base.repeat(nrows // len(distinct), 1).reshape(NSUB, NPOL, NCHAN, NBIN).contiguous()
        rows = src.reshape(nrows, NBIN)
        nbytes = src.numel() * src.element_size()
        for label, kw in (("PS", {}), ("fit_exp_dc", dict(method='fit', fn='exp_dc')),
                          ("fit_half_tri", dict(method='fit', fn='half_tri'))):
            med, lo, hi = timed(lambda: eng.channel_noise(rows, **kw))
            rec = dict(seconds=med, seconds_min=lo, seconds_max=hi, bytes_read=nbytes, rows=nrows,
                       TB_per_s=nbytes / med / 1e12, ns_per_row=med / nrows * 1e9)
            if label != "PS":
                eng.set_option("profile", 1)
                eng.kernel_times(reset=True)
                for _ in range(CALLS):
                    eng.channel_noise(rows, **kw)
                eng.synchronize()
                sec, n = eng.kernel_times(reset=True)["noise_fit"]
                eng.set_option("profile", 0)
                rec.update(kernel_seconds=sec / max(n, 1))
            runs["%s_%s" % (name, label)] = rec
        for label in ("fit_exp_dc", "fit_half_tri"):
            runs["%s_%s" % (name, label)]["ratio_to_PS"] = runs["%s_%s" % (name, label)]["seconds"] / runs[name + "_PS"]["seconds"]
        del src, rows, base
    # the result at this size against the restatement, and the restatement's own cost
    t0 = time.perf_counter()
    want = nf.noise_fit_rows(distinct[:cpu_rows])
    cpu = (time.perf_counter() - t0) / cpu_rows
    got = eng.noise_fit(distinct[:cpu_rows])
    ok = want[3] >= nf.MARGIN_MIN
    check = dict(rows=cpu_rows, rows_compared=int(ok.sum()), kc_equal=bool((got[1][ok] == want[1][ok]).all()),
                 cell_equal=bool((got[2][ok] == want[2][ok]).all()),
                 noise_max_rel=float(np.max(np.abs(got[0][ok] - want[0][ok]) / want[0][ok])))
    eng.close()
    return dict(runs=runs, check=check, numpy_restatement_seconds_per_row=cpu,
                numpy_restatement_hours_for_this_archive=cpu * nrows / 3600.0, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisefit_timing.json"))
    ap.add_argument("--variant", action="append", default=[], metavar="name=path.so")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    opts = ap.parse_args()
    if opts.child:
        print("RESULT " + json.dumps(measure()))
        return
    out = dict(shape=[NSUB, NPOL, NCHAN, NBIN],
               method="host clock around windows of %d synchronous calls, seconds per call, median of 7 windows after 2 "
                      "warm-up calls; kernel_seconds from HIP events round the launch (option profile)" % CALLS)
    out.update(measure())
    variants = {}
    for spec in opts.variant:
        name, path = spec.split("=", 1)
        env = dict(os.environ, PP_TOAS_LIB=os.path.abspath(path))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                           timeout=900)
        if p.returncode != 0:
            raise SystemExit("noisefit_timing: variant %s failed:\n%s" % (name, p.stderr[-2000:]))
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        variants[name] = dict(check=res["check"], runs={k: v for k, v in res["runs"].items() if "_fit_" in k})
    if variants:
        out["variants"] = variants
    with open(opts.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
