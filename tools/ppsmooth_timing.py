#!/usr/bin/env python3
"""Times the wavelet smoothing on the MI355X and writes one JSON line (and profiles/ppsmooth_timing.json).

  smart_smooth of 11 rows x 2048 bins, 11 levels   (make_smooth_spline_model's work: ten eigenvectors and the mean)
  smart_smooth of a 512 x 1024 portrait, 8 levels  (DataPortrait.smooth_portrait(smart=True))

Each is a whole Engine.smart_smooth call on host f64 rows (copies included), the device warmed by one call, the
median of 5.  Beside them the CPU time of the same work in the plain-NumPy restatement (tests/wavelet_ref.py) under
scipy.optimize.brute as the reference calls it: ONE row is run (every level) and its time multiplied by the number
of rows -- the whole portrait would take the better part of an hour.  Device name, date and the clocks the driver
reports go into the file.

    python tools/ppsmooth_timing.py [--out profiles/ppsmooth_timing.json]"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows_of(nrows, nbin, seed):
    from tests import ppsmooth_cases as sc
    rng = np.random.default_rng(seed)
    return np.array([sc.profile(nbin, float(snr), seed + i) for i, snr in enumerate(rng.choice([3.0, 10.0, 30.0, 100.0], nrows))])


def cpu_row(x, nlev):
    import scipy.optimize as opt
    from tests import wavelet_ref as wr
    t0 = time.perf_counter()
    nfev = [0]

    def f(fact, lev):
        nfev[0] += 1
        return wr.objective(float(np.asarray(fact).reshape(-1)[0]), x, lev)
    for lev in range(1, nlev + 1):
        opt.brute(f, ranges=[(0.0, 3.0)], args=(lev,), Ns=30, full_output=True)
    return time.perf_counter() - t0, nfev[0]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2] or "not reported"
    except Exception as e:          # noqa: BLE001
        return "not reported (%s)" % type(e).__name__


def case(nrows, nbin, nlev, seed):
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    rows = rows_of(nrows, nbin, seed)
    eng.smart_smooth(rows, nlev)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out, info = eng.smart_smooth(rows, nlev)
        times.append(time.perf_counter() - t0)
    t_cpu, nfev_cpu = cpu_row(rows[0], nlev)
    return dict(rows=nrows, nbin=nbin, levels=nlev, device_call_s=statistics.median(times), device_call_s_all=times,
                evaluations=int(info["nfev"].sum()), rows_zeroed=int((~out.any(axis=1)).sum()),
                cpu_restatement_one_row_s=t_cpu, cpu_restatement_one_row_evaluations=nfev_cpu,
                cpu_restatement_all_rows_s_extrapolated=t_cpu * nrows, device_row0_evaluations=int(info["nfev"][0]))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppsmooth_timing.json"))
    a = ap.parse_args()
    res = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), "date": datetime.date.today().isoformat(), "clocks": clocks(),
           "host_threads": os.cpu_count(),
           "11x2048_11levels": case(11, 2048, 11, 6100), "512x1024_8levels": case(512, 1024, 8, 6200)}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
