"""Wall-clock of `python -m pulseportraiture_amd.pptoas_run` at --gpus 1 and --gpus 2 on 64 .npz
archives of 16 subints x 512 channels x 2048 bins (float32), and the one-rank split of
get_TOAs' time into the device fits (sum of fit_durations) and the rest (host).

With one GPU on the box, --gpus 2 is two processes sharing that GPU over gloo: what it
measures is whether the per-archive host bookkeeping of two processes overlaps, not a
scaling figure.  Prints one JSON line.

    python tools/time_gettoas_ranks.py [--workdir DIR] [--narch 64] [--nsub 16] [--timeout 1500]
"""
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
MODEL = os.path.join(ROOT, "tests", "golden", "example.gmodel")

SPLIT = r'''
import json, sys, time
from pulseportraiture_amd.pptoas import GetTOAs
gt = GetTOAs(sys.argv[1], sys.argv[2], quiet=True)
t0 = time.time()
gt.get_TOAs(quiet=True)
wall = time.time() - t0
print(json.dumps({"wall_s": wall, "device_s": float(sum(gt.fit_durations)), "ntoa": len(gt.TOA_list)}))
'''


def make_archives(workdir, narch, nsub, nchan, nbin):
    from pulseportraiture_amd.pptoas import MJD
    from tests import synth_host as sh
    freqs, model = sh.model_portrait(nchan, nbin)
    subints = np.empty((nsub, 1, nchan, nbin), dtype=np.float32)
    for i in range(nsub):
        subints[i, 0] = sh.make_inputs(nchan, nbin, seed=500 + i, DM0=30.0, model=model)["data"]
    paths = []
    for ia in range(narch):
        epochs = np.empty(nsub, dtype=object)
        epochs[:] = [MJD(58000 + ia, 0.001 * i) for i in range(nsub)]
        p = os.path.join(workdir, "arch%03d.npz" % ia)
        np.savez(p, subints=subints, freqs=np.broadcast_to(freqs, (nsub, nchan)), Ps=np.full(nsub, sh.P_EXAMPLE),
                 epochs=epochs, noise_stds=np.full((nsub, 1, nchan), 0.05), DM=np.asarray(30.0))
        paths.append(p)
    lst = os.path.join(workdir, "archives.txt")
    with open(lst, "w") as f:
        f.write("".join(p + "\n" for p in paths))
    return lst


def timed(cmd, timeout, env):
    t0 = time.time()
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout,
                       start_new_session=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("failed (%d): %s" % (p.returncode, " ".join(cmd)))
    return time.time() - t0, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--narch", type=int, default=64)
    ap.add_argument("--nsub", type=int, default=16)
    ap.add_argument("--nchan", type=int, default=512)
    ap.add_argument("--nbin", type=int, default=2048)
    ap.add_argument("--timeout", type=float, default=1500.0, help="per run [s]")
    args = ap.parse_args()
    workdir = args.workdir or tempfile.mkdtemp(prefix="pp_time_ranks_")
    os.makedirs(workdir, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT
    try:
        lst = make_archives(workdir, args.narch, args.nsub, args.nchan, args.nbin)
        out = {"archives": args.narch, "shape": [args.nsub, args.nchan, args.nbin], "dtype": "float32",
               "note": "--gpus 2 is two processes sharing one GPU (gloo); not a scaling figure"}
        tims = []
        for n in (1, 2):
            tim = os.path.join(workdir, "gpus%d.tim" % n)
            wall, _ = timed([sys.executable, "-m", "pulseportraiture_amd.pptoas_run", "--gpus", str(n), "-d", lst,
                             "-m", MODEL, "-o", tim, "--quiet"], args.timeout, env)
            out["pptoas_run_gpus%d_wall_s" % n] = round(wall, 3)
            tims.append(open(tim, "rb").read())
        out["same_bytes"] = tims[0] == tims[1]
        _, text = timed([sys.executable, "-c", SPLIT, lst, MODEL], args.timeout, env)
        split = json.loads(text.strip().splitlines()[-1])
        out["one_rank_get_TOAs_s"] = round(split["wall_s"], 3)
        out["one_rank_device_s"] = round(split["device_s"], 3)
        out["one_rank_host_s"] = round(split["wall_s"] - split["device_s"], 3)
        out["toas"] = split["ntoa"]
        print(json.dumps(out))
    finally:
        if args.workdir is None:
            shutil.rmtree(workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
