#!/usr/bin/env python3
"""Times the narrowband scattering fit on the MI355X and writes profiles/nbscat_timing.json.

The workload is archive-shaped: 64 subints x 512 channels x 2048 bins = 32 768 (profile, template) pairs from
example.gmodel without its scattering, every channel scattered by tau = 30 us at 1500 MHz scaled as nu^-4, white
noise sigma = 0.05, log10_tau, the guess 1.5 x the truth at every channel.  Three ways, in the same process, in
alternating order, `--reps` times each after a warm-up:

  phase_tau       Engine.fit_phase_tau_batch, one call; its kernel split (transform / fit) by HIP events from
                  Engine.kernel_times() in a separate call (option "profile"), so that the events do not sit in the
                  timed calls
  per_channel     what the parent commit offers for these numbers: 512 one-channel Engine.fit_batch calls with
                  fit_flags [1,0,0,1,0], every one with its channel's template in slot 0
  phase_only      Engine.fit_phase_shift_batch on the same pairs: the floor, no scattering

    python tools/nbscat_timing.py [--out profiles/nbscat_timing.json] [--reps 5] [--nsub 64] [--nchan 512]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
P = 1.0 / 345.67890123456789


def workload(nsub, nchan, nbin, seed=5):
    from pulseportraiture_amd import gmodel
    mdl = dict(gmodel.parse_gmodel(gmodel.EXAMPLE_GMODEL))
    params = np.array(mdl["params"], dtype=np.float64)
    params[1] = 0.0
    mdl["params"] = params
    d = 800.0 / nchan
    freqs = np.linspace(1100 + d / 2, 1900 - d / 2, nchan)
    model = gmodel.gaussian_portrait(mdl, freqs, nbin, P)
    tau = (30e-6 / P) * (freqs / 1500.0) ** -4.0
    k = np.arange(nbin // 2 + 1)
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-0.5, 0.5, (nsub, 1))
    F = np.fft.rfft(model, axis=-1) / (1.0 + 2.0j * np.pi * k[None] * tau[:, None])
    data = np.empty((nsub, nchan, nbin))
    for i in range(nsub):
        data[i] = np.fft.irfft(F * np.exp(-2.0j * np.pi * k[None] * phi[i]), nbin, axis=-1)
    data += 0.05 * rng.standard_normal(data.shape)
    return dict(data=data, model=model, freqs=freqs, guess=np.log10(1.5 * tau), phi=phi[:, 0], tau=tau)


def stats(ts, nfit):
    ts = np.asarray(ts)
    return dict(seconds=[float(t) for t in ts], median_s=float(np.median(ts)), spread_s=float(ts.max() - ts.min()),
                fits_per_s=float(nfit / np.median(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbscat_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nsub", type=int, default=64)
    ap.add_argument("--nchan", type=int, default=512)
    ap.add_argument("--nbin", type=int, default=2048)
    a = ap.parse_args()
    from pulseportraiture_amd.engine import default_engine
    eng = default_engine()
    w = workload(a.nsub, a.nchan, a.nbin)
    nfit = a.nsub * a.nchan
    profs = w["data"].reshape(nfit, a.nbin)
    mprofs = np.ascontiguousarray(np.broadcast_to(w["model"][None], w["data"].shape)).reshape(nfit, a.nbin)
    guess = np.tile(w["guess"], a.nsub)
    sigma = np.full(nfit, 0.05)
    bychan = [np.ascontiguousarray(w["data"][:, n:n + 1]) for n in range(a.nchan)]

    def phase_tau():
        return eng.fit_phase_tau_batch(profs, mprofs, noise=sigma, tau_guess=guess, log10_tau=True)

    def per_channel():
        out = np.empty((a.nsub, a.nchan, 2))
        for n in range(a.nchan):
            nu = w["freqs"][n]
            eng.set_model(w["model"][n:n + 1], slot=0)
            x0 = np.tile([0.0, 0.0, 0.0, w["guess"][n], 0.0], (a.nsub, 1))
            r = eng.fit_batch(bychan[n], w["freqs"][n:n + 1], P, x0, errs=np.full((a.nsub, 1), 0.05),
                              nu_fits=[[nu, nu, nu]], nu_outs=[[nu, nu, nu]], fit_flags=[1, 0, 0, 1, 0],
                              log10_tau=True, seed_ns=100)
            out[:, n, 0], out[:, n, 1] = r["params"][:, 0], r["params"][:, 3]
        return out

    def phase_only():
        return eng.fit_phase_shift_batch(profs, mprofs, noise=sigma)

    ways = dict(phase_tau=phase_tau, per_channel=per_channel, phase_only=phase_only)
    res = {k: f() for k, f in ways.items()}            # warm-up, and the answers to compare
    times = {k: [] for k in ways}
    for rep in range(a.reps):
        order = list(ways) if rep % 2 == 0 else list(ways)[::-1]
        for k in order:
            t0 = time.perf_counter()
            ways[k]()
            times[k].append(time.perf_counter() - t0)
    eng.set_option("profile", 1)
    eng.kernel_times(reset=True)
    phase_tau()
    kt = eng.kernel_times(reset=True)
    eng.set_option("profile", 0)
    pt = res["phase_tau"]
    dphi = np.abs((pt[:, 0].reshape(a.nsub, a.nchan) - res["per_channel"][..., 0] + 0.5) % 1.0 - 0.5)
    out = dict(workload=dict(nsub=a.nsub, nchan=a.nchan, nbin=a.nbin, nfit=nfit, log10_tau=True, reps=a.reps),
               phase_tau=stats(times["phase_tau"], nfit), per_channel=stats(times["per_channel"], nfit),
               phase_only=stats(times["phase_only"], nfit),
               phase_tau_kernels=dict(transform_s=kt["nbscat_fft"][0], fit_s=kt["nbscat_fit"][0]),
               phase_tau_nfeval=dict(median=float(np.median(pt[:, 9])), max=float(pt[:, 9].max())),
               phase_tau_return_codes={str(int(c)): int((pt[:, 10] == c).sum()) for c in np.unique(pt[:, 10])},
               agreement=dict(max_dphi_vs_per_channel=float(np.nanmax(dphi)),
                              max_dlog10tau_vs_per_channel=float(np.nanmax(np.abs(
                                  pt[:, 2].reshape(a.nsub, a.nchan) - res["per_channel"][..., 1])))))
    out["speedup_vs_per_channel"] = out["per_channel"]["median_s"] / out["phase_tau"]["median_s"]
    out["cost_vs_phase_only"] = out["phase_tau"]["median_s"] / out["phase_only"]["median_s"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
