#!/usr/bin/env python3
"""Times ppzap on the MI355X and writes one JSON line (and profiles/ppzap_timing.json):

  kernel   pp_channel_noise on a resident 1024 x 4096 x 2048 f64 batch (68.7 GB), norm None and
           'prof' (the divisors given), wall time of the synchronous call (3 repeats after a
           warm-up; it also copies 2 x 32 MB of results back, 'prof' 32 MB of divisors in), and the
           call's bytes / time against 8 TB/s.  Run it under `rocprofv3 --kernel-trace --stats` for
           the kernel time alone.
  cli      wall time of `python -m pulseportraiture_amd.ppzap_run -d list.txt -n 5` (and -N mean)
           on 64 archives of 16 x 512 x 2048 (f32 .npz), as a child process
  cpu      a per-channel NumPy loop doing the reference's work (one rfft and the top-quarter power per
           row, as get_noise_PS does for load_data's noise) on the same data, on one CPU core

    python tools/time_ppzap.py [--skip-kernel] [--narch 64]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


def kernel(nsub=1024, nchan=4096, nbin=2048):
    import ctypes as C
    import torch
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    x = torch.empty((nsub, nchan, nbin), dtype=torch.float64, device="cuda")
    x.normal_()
    torch.cuda.synchronize()
    nrows = nsub * nchan
    norms, noise, div = np.empty(nrows), np.empty(nrows), np.ones(nrows)
    out = {}
    for name, method in (("none", 0), ("prof", 3)):
        times = []
        for rep in range(4):
            t0 = time.perf_counter()
            rc = eng._lib.pp_channel_noise(eng._ctx, C.c_void_p(x.data_ptr()), _lib.PP_F64, 1, nrows, nbin, method,
                                           div.ctypes.data_as(_lib.c_double_p), norms.ctypes.data_as(_lib.c_double_p),
                                           noise.ctypes.data_as(_lib.c_double_p))
            times.append(time.perf_counter() - t0)
            assert rc == 0, _lib.last_error()
        t = min(times[1:])
        out[name] = dict(call_s=t, calls_s=times[1:], bytes=x.numel() * 8, TBps=x.numel() * 8 / t / 1e12,
                         share_of_8TBps=x.numel() * 8 / t / HBM)
    del x
    torch.cuda.empty_cache()
    return out


def archives(tmp, narch, nsub=16, nchan=512, nbin=2048):
    rng = np.random.default_rng(7)
    ph = (np.arange(nbin) + 0.5) / nbin
    prof = 10.0 * np.exp(-0.5 * ((ph - 0.3) / 0.02) ** 2)
    names = []
    for a in range(narch):
        x = (prof + rng.standard_normal((nsub, nchan, nbin))).astype(np.float32)
        x[:, rng.choice(nchan, 8, replace=False)] *= 5.0
        w = np.ones((nsub, nchan))
        w[:, rng.choice(nchan, 10, replace=False)] = 0.0
        names.append("a%02d.npz" % a)
        np.savez(os.path.join(tmp, names[-1]), subints=x, freqs=np.linspace(1100.0, 1900.0, nchan),
                 Ps=np.full(nsub, 0.003), epochs=np.zeros(nsub), weights=w)
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("".join(n + "\n" for n in names))
    return names


def cli(tmp, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.ppzap_run", "-d", "list.txt", "-n", "5"] + extra,
                       cwd=tmp, env=env, capture_output=True, text=True, timeout=1200)
    t = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(wall_s=t, summary=p.stdout.strip().splitlines()[-1])


# the reference's noise method, measured as it runs: one NumPy power spectrum per channel of every subint
# (its per-channel loop; the noise of a row is the rms of the top quarter of its harmonics' powers / nbin)
CPU_LOOP = r'''
import time, numpy as np
t = 0.0
for name in open("list.txt").read().split():
    port = np.load(name)["subints"].astype(np.float64)
    t0 = time.perf_counter()
    for sub in port:
        noise = np.empty(len(sub))
        for n, row in enumerate(sub):
            p = np.abs(np.fft.rfft(row)) ** 2 / len(row)
            noise[n] = np.sqrt(p[int(0.75 * (len(row) // 2 + 1)):].mean())
    t += time.perf_counter() - t0
print(t)
'''


def cpu(tmp):
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    p = subprocess.run(["taskset", "-c", "0", sys.executable, "-c", CPU_LOOP], cwd=tmp, env=env,
                       capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stderr[-2000:]
    return dict(noise_loop_s=float(p.stdout.strip()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--narch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppzap_timing.json"))
    a = ap.parse_args()
    res = {}
    tmp = tempfile.mkdtemp(prefix="ppzap_time_")
    try:
        # (archives and the child command line first: this process touches the GPU only afterwards)
        archives(tmp, a.narch)
        res["cli_64x16x512x2048_f32"] = {"-n 5": cli(tmp, []), "-n 5 -N mean": cli(tmp, ["-N", "mean"])}
        res["cpu_reference_noise_loop_one_core"] = cpu(tmp)
        if not a.skip_kernel:
            res["kernel_1024x4096x2048_f64"] = kernel()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
