#!/usr/bin/env python3
"""Goldens of make_fake_pulsar (pplib.make_fake_pulsar, Engine.fake_portraits): the noise-free rows of a simulated
subint, composed with the TRUE reference's own functions in make_fake_pulsar's order (pplib.py:3334-3376):

    read_model(modelfile, phases, freqs, P)
    xs None:  rotate_data(model, -phase, -dDM, P, freqs, nu0)        the line the reference documents (its :3343)
    xs given: add_DM_nu(model, -phase_transform(phase, DM + dDM, nu0, nu_DM, P), -dDM, P, freqs, xs, Cs, nu_DM)
    t_scat and a model TAU of 0:  irfft(scattering_portrait_FT(scattering_times(t_scat / P, alpha, freqs, nu0)) * rfft)
    add_scintillation(port, params),  scales[:, None] * port
    PSRCHIVE's part, dededisperse():  rotate_data(port, 0, -DM, P, freqs, nu0)       unless dedispersed

Build-container only (needs /root/reference); see make_golden.py for how the reference is imported.

    python tests/golden/make_golden_ppfake.py      # writes tests/golden/ppfake_rows.npz and tests/golden/example.par

ppfake_rows.npz   <case>_rows [nchan][nbin], <case>_self_dev, and `cases`: a JSON object of every case's arguments
                  (the keyword arguments of make_fake_pulsar, and the text of its .gmodel file).
                  self_dev = max |un-reversed - plain| / peak of the same composition with the channel order reversed.
example.par       a copy of the reference's examples/example.par (settings only).

Six cases, each with 6 channels over 1100-1900 MHz, at 64 bins (a tuned transform plan) and at 100 (chirp-z).
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

GMODEL = os.path.join(mg.REF, "examples", "example.gmodel")
PARFILE = os.path.join(mg.REF, "examples", "example.par")
F0, DM = 345.67890123456789, 34.56789          # example.par
GEOM = dict(nchan=6, nu0=1500.0, bw=800.0)

CASES = {
    "plain": dict(phase=0.13, dDM=2e-3),
    "dedispersed": dict(phase=0.13, dDM=2e-3, dedispersed=True),
    "dm_nu": dict(phase=0.13, dDM=2e-3, xs=[-2.0, -4.0], Cs=[1.0, 2e5], nu_DM=1400.0),
    "t_scat": dict(phase=0.13, dDM=2e-3, t_scat=5e-5, alpha=-3.6),
    "scint_scales": dict(phase=0.13, dDM=2e-3, scint=[0.7, 1.3, 0.2, 0.4, 3.1, 0.55],
                         scales=[1.0, 0.5, 2.0, 1.5, 0.25, 3.0]),
    # a model with a scattering time of its own: it overrides t_scat (pplib.py:3351)
    "model_tau": dict(phase=0.13, dDM=2e-3, t_scat=5e-5, model_tau=4e-5),
}


def gmodel_text(model_tau=None):
    """The parameter lines of the reference's example.gmodel (comment lines dropped), TAU replaced on request."""
    lines = []
    for line in open(GMODEL):
        body = line.split("#")[0].rstrip()
        if not body.strip():
            continue
        if body.split()[0] == "TAU" and model_tau is not None:
            body = "TAU     %.8f 1" % model_tau
        lines.append(body)
    return "\n".join(lines) + "\n"


def reference_rows(ref, tmp, nbin, kw, reverse=False):
    kw = dict(kw)
    text = gmodel_text(kw.pop("model_tau", None))
    modelfile = os.path.join(tmp, "case.gmodel")
    with open(modelfile, "w") as f:
        f.write(text)
    nchan, nu0, bw = GEOM["nchan"], GEOM["nu0"], GEOM["bw"]
    P = 1.0 / F0
    chanwidth = bw / nchan
    lofreq = nu0 - (bw / 2)
    freqs = np.linspace(lofreq + (chanwidth / 2.0), lofreq + bw - (chanwidth / 2.0), nchan)
    flip = (lambda a: a[::-1].copy()) if reverse else (lambda a: a)
    freqs = flip(freqs)
    phases = ref.get_bin_centers(nbin, lo=0.0, hi=1.0)
    params = ref.read_model(modelfile, quiet=True)[4]
    name, ngauss, model = ref.read_model(modelfile, phases, freqs, P, quiet=True)
    phase, dDM = kw.get("phase", 0.0), kw.get("dDM", 0.0)
    if kw.get("xs") is None:
        port = ref.rotate_data(model, -phase, -dDM, P, freqs, nu0)
    else:
        ph = ref.phase_transform(phase, DM + dDM, nu0, kw["nu_DM"], P)
        port = ref.add_DM_nu(model, -ph, -dDM, P, freqs, kw["xs"], kw["Cs"], kw["nu_DM"])
    if kw.get("t_scat") and not params[1]:
        taus = ref.scattering_times(kw["t_scat"] / P, kw.get("alpha", ref.scattering_alpha), freqs, nu0)
        port = np.fft.irfft(ref.scattering_portrait_FT(taus, nbin) * np.fft.rfft(port, axis=-1), axis=-1)
    if kw.get("scint"):
        # (the pattern runs over the channel index: always applied in the plain order)
        port = flip(ref.add_scintillation(flip(port), kw["scint"]))
    scales = flip(np.asarray(kw.get("scales", 1.0)) * np.ones(nchan))
    port = scales[:, None] * port
    if not kw.get("dedispersed"):
        port = ref.rotate_data(port, 0.0, -DM, P, freqs, nu0)
    return flip(port), text


def main():
    ref, tmp = mg.import_reference()
    try:
        out, cases = {}, {}
        for nbin in (64, 100):
            for cname, kw in CASES.items():
                name = "%s_%d" % (cname, nbin)
                rows, text = reference_rows(ref, tmp, nbin, kw)
                rev, _ = reference_rows(ref, tmp, nbin, kw, reverse=True)
                peak = np.abs(rows).max()
                dev = float(np.abs(rev - rows).max() / peak)
                print("%-20s peak %.4g self_dev %.2e" % (name, peak, dev))
                assert dev < 1e-12, (name, dev)
                out[name + "_rows"], out[name + "_self_dev"] = rows, dev
                args = {k: v for k, v in kw.items() if k != "model_tau"}
                cases[name] = dict(kwargs=dict(args, nbin=nbin, **GEOM), gmodel=text)
        np.savez(os.path.join(HERE, "ppfake_rows.npz"), cases=json.dumps(cases, sort_keys=True), **out,
                 **{k: np.array(v) for k, v in mg.versions().items()})
        shutil.copy(PARFILE, os.path.join(HERE, "example.par"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
