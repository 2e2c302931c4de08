#!/usr/bin/env python3
"""Do two builds of libpptoas_hip.so return the same bits?  (A refactor of the host driver must.)

    python tools/compare_builds.py A.so B.so [outdir]

runs one list of fits -- every flow the driver has, in seconds-sized shapes -- once per library, each in a fresh
child process (PP_TOAS_LIB selects the library), saves every output array to <outdir>/<name>.npz and requires
numpy.testing.assert_array_equal on all of them (NaNs in the same places count as equal).  A == B checks that a
build agrees with itself.  Exit status 1 when some array differs.

    python tools/compare_builds.py --run out.npz        (the child: the list of fits with the library in use)

The synthetic batches come from tests/test_gpu_parity.py's helper _full_shape_case (the bench's recipe), so the tool
follows that helper's signature.  After the fits come the auxiliary entry points -- every export that is no fit -- on
the inputs of that module's split test (_aux_split_inputs: 11 subints x 24 channels, 256 and 100 bins, f64 and f32,
shared and per-subint frequencies, one and two templates), whole and with a work budget of three subints.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("params", "param_errs", "nu_refs", "cov", "chi2", "red_chi2", "snr", "nfeval", "npass", "return_code",
        "scales", "scale_errs", "channel_snrs", "seed_phase")


def fits():
    """Yields (case name, result dict)."""
    import torch
    from tests.test_gpu_parity import _full_shape_case
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.pplib import Dconst
    SCAT = [1, 1, 0, 1, 1]

    def refseed(freqs, model, nsub, mask=None):
        nu_mean = np.array([freqs[mask[i] > 0].mean() if mask is not None else freqs.mean() for i in range(nsub)])
        return dict(weights=None if mask is None else mask.astype(np.float64), model_profs=model.mean(axis=0), nu_mean=nu_mean,
                    Ns=100, finish='simplex')

    # 64 x 256: phase + DM, scattering
    e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(64, 256, [1, 1, 0, 0, 0], False, nsub=4)
    yield "64x256 phiDM", e.fit_batch(data, freqs, P, x0, **kw)
    e.close()
    e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(64, 256, SCAT, True, nsub=4, tau_us=40.0)
    yield "64x256 scat", e.fit_batch(data, freqs, P, x0, **kw)
    e.close()
    # the three solve widths and the rows-in-turn solve: plain, masked with measured noise, Newton
    for C in (256, 640, 2304):
        e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(C, 2048, [1, 1, 0, 0, 0], False, nsub=8)
        mask = np.ones((8, C), dtype=np.uint8)
        mask[:, ::9] = 0
        yield "%dx2048 plain" % C, e.fit_batch(data, freqs, P, x0, **kw)
        yield "%dx2048 masked noise measured" % C, e.fit_batch(data, freqs, P, x0, **dict(kw, errs=None, chan_mask=mask))
        yield "%dx2048 newton" % C, e.fit_batch(data, freqs, P, x0, method="newton", **kw)
        if C == 256:
            # two poor guesses in the batch: re-expansion, then evaluations over a stored cross-spectrum
            xp = x0.copy()
            xp[1, 0] += 6e-3; xp[1, 1] += 4e-3; xp[5, 0] -= 2e-2
            yield "256x2048 two poor guesses", e.fit_batch(data, freqs, P, xp, **kw)
            # the reference's own guess formed in the pass
            yield "256x2048 ref_seed", e.fit_batch(data, freqs, P, x0, ref_seed=refseed(freqs, model, 8), **kw)
            yield "256x2048 ref_seed masked", e.fit_batch(data, freqs, P, x0, ref_seed=refseed(freqs, model, 8, mask),
                                                          **dict(kw, chan_mask=mask))
            yield "256x2048 seed_ns", e.fit_batch(data, freqs, P, x0, seed_ns=100, **kw)
        e.close()
    # scattering, both solvers (Newton at >= 512 channels: the coarse pass), and the reference seed of a scattering fit
    e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(512, 2048, SCAT, True, nsub=4, tau_us=20.0)
    yield "512x2048 scat trust-ncg", e.fit_batch(data, freqs, P, x0, **kw)
    yield "512x2048 scat newton", e.fit_batch(data, freqs, P, x0, method="newton", **kw)
    yield "512x2048 scat ref_seed", e.fit_batch(data, freqs, P, x0, ref_seed=refseed(freqs, model, 4), **kw)
    e.close()
    # a row length without a tuned plan
    e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(300, 1000, [1, 1, 0, 0, 0], False, nsub=4)
    yield "300x1000 plain", e.fit_batch(data, freqs, P, x0, **kw)
    e.close()
    # pp_fit_enqueue three deep: plain / reference-seed / 1024-bin / scattering batches on one context
    e, data, freqs, model, P, x0, errs, nu_fit, kw = _full_shape_case(256, 2048, [1, 1, 0, 0, 0], False, nsub=8)
    rs = refseed(freqs, model, 8)
    f2, m2, _ = gmodel.example_model(256, 1024)
    e.set_model(m2, slot=2)
    d2 = torch.empty((8, 256, 1024), dtype=torch.float64, device="cuda:0")
    inj = np.zeros((8, 3)); inj[:, 1] = 34.56789
    e.synth_portraits(d2, f2, P, inj, 0.05, 7, 0, slot=2)
    slot2 = np.full(8, 2, dtype=np.int32)
    x2 = x0.copy(); x2[:, 0] = (Dconst * 34.56789 / P / nu_fit ** 2 + 0.5) % 1.0 - 0.5
    xs = x0.copy(); xs[:, 3] = -3.0; xs[:, 4] = -4.0
    jobs = [("plain", data, x0, kw), ("ref_seed", data, x0, dict(kw, ref_seed=rs)), ("plain 2", data, x0, kw),
            ("1024-bin", d2, x2, dict(kw, model_slot=slot2)), ("ref_seed 2", data, x0, dict(kw, ref_seed=rs)),
            ("scat", data, xs, dict(kw, fit_flags=SCAT, log10_tau=True)), ("ref_seed 3", data, x0, dict(kw, ref_seed=rs)),
            ("plain 3", data, x0, kw), ("plain 4", data, x0, kw)]
    names = []
    for name, d, x, k in jobs:
        e.enqueue(d, freqs, P, x, **k)
        names.append(name)
        if len(names) == 3:
            yield "chain " + names.pop(0), e.collect()
    while names:
        yield "chain " + names.pop(0), e.collect()
    e.close()


def aux_calls():
    """Yields (case name, {output name: array}) for the auxiliary entry points."""
    import torch
    from tests.test_gpu_parity import _aux_split_inputs, _aux_split_calls
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.engine import Engine
    e = Engine(0)
    gm = gmodel.parse_gmodel(gmodel.EXAMPLE_GMODEL)
    for B in (256, 100):
        for dtype, per_subint, slots in ((np.float64, False, False), (np.float64, True, True), (np.float32, True, True)):
            d = _aux_split_inputs(B, dtype, per_subint, slots)
            tag = "aux %d %s freqs%s slots=%d" % (B, np.dtype(dtype).name, "[nsub,nchan]" if per_subint else "[nchan]", slots)
            ports, C, nsub = d["ports"], d["C"], d["nsub"]
            dev = torch.from_numpy(ports).to("cuda:0")
            for budget in (96e9, 3.4 * C * B * np.dtype(dtype).itemsize):
                e.set_option("max_work_bytes", budget)
                r = _aux_split_calls(e, d)
                out = {"fit_phase_shift_batch": r[0][:, :6], "rotate_portraits": r[1], "align_accumulate": r[2][0],
                       "align_accumulate weights": r[2][1], "channel_red_chi2": r[3], "reference_phase_seed": r[4][:, :6]}
                # the same from device-resident portraits (rotate_portraits works in place: on a copy)
                nu = d["freqs1"].mean()
                out["rotate_portraits device"] = e.rotate_portraits(dev.clone(), d["freqs"], d["P"], phi=d["phi"], DM=d["DM"], nu_DM=nu)
                out["align_accumulate device"] = e.align_accumulate(dev, d["freqs"], d["P"], d["phi"], d["DM"], nu, d["w"])[0]
                out["channel_red_chi2 device"] = e.channel_red_chi2(dev, d["freqs"], d["P"], d["params"], d["nus"], d["scales"],
                                                                  d["errs"], slots=d["slots"])
                out["reference_phase_seed device"] = e.reference_phase_seed(dev, d["freqs"], d["P"], d["w"], d["model"].mean(axis=0),
                                                                          phi=d["phi"], DM=d["DM"], nu_DM=nu)[:, :6]
                out["rfft_rows"] = e.rfft_rows(ports.reshape(-1, B)).view(np.float64)
                for norm in (None, "max", "prof"):
                    out["channel_noise %s" % norm], out["channel_noise %s norms" % norm] = e.channel_noise(ports, norm=norm, weights=d["w"])
                out["channel_noise device"] = e.channel_noise(dev, norm="rms")[0]
                out["channel_snrs"] = e.channel_snrs(ports)
                out["channel_snrs device"] = e.channel_snrs(dev)
                out["zap_median"] = e.zap_median(out["channel_noise None"], np.ones((nsub, C)), 1.5)
                # pca: 24 channels (the dual side), then all the rows as one tall portrait (nchan >= nbin)
                for name, port, w in (("pca", ports[0], d["w"][0]), ("pca tall", ports.reshape(-1, B), d["w"].reshape(-1))):
                    mean_prof, gram, fact = e.pca_gram(port, w)
                    lam, vec = np.linalg.eigh(gram)
                    eigvec, stats = e.pca_basis(vec[:, ::-1][:, :4], lam[::-1][:4])
                    proj, reconst = e.pca_project([2, 0])
                    out.update({name + " mean": mean_prof, name + " gram": gram, name + " basis": eigvec, name + " stats": stats,
                                name + " proj": proj, name + " reconst": reconst})
                # generated templates: to the host, to the device, into a slot; the response on that slot
                out["gaussian_portrait"] = e.gaussian_portrait(gm, d["freqs1"], B, 0.004)
                gdev = torch.empty((C, B), dtype=torch.float64, device="cuda:0")
                e.gaussian_portrait(gm, d["freqs1"], B, 0.004, out=gdev)
                out["gaussian_portrait device"] = gdev
                tck = (np.r_[[d["freqs1"][0]] * 4, [d["freqs1"][-1]] * 4], [np.linspace(-1, 1, 8), np.linspace(2, 0, 8)], 3)
                spl = (d["model"].mean(axis=0), np.stack([np.roll(d["model"][0], 1), np.roll(d["model"][-1], 2)], axis=1), tck)
                out["spline_portrait"] = e.spline_portrait(spl[0], spl[1], spl[2], d["freqs1"])
                out["set_model_gaussian nharm"] = np.array(e.set_model_gaussian(gm, d["freqs1"], B, 0.004, slot=2))
                out["set_model_spline nharm"] = np.array(e.set_model_spline(spl[0], spl[1], spl[2], d["freqs1"], slot=3))
                out["apply_response nharm"] = np.array(e.apply_response(3, rconst=np.exp(-0.01 * np.arange(B // 2 + 1)) + 0j,
                                                                       smear_wid=np.full(C, 1e-3)))
                # what the slots hold, seen through their own calls: the templates' means and noiseless synthetic subints
                for slot in (2, 3):
                    out["model_means slot %d" % slot] = e.model_means(slot, C, B)
                    syn = torch.empty((3, C, B), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0")
                    e.synth_portraits(syn, d["freqs1"], d["P"][:3], np.c_[d["phi"][:3], d["DM"][:3], np.zeros(3)], 0.05, 11, 2,
                                      slot=slot, gains=d["scales"][:3])
                    out["synth_portraits slot %d" % slot] = syn
                    out["channel_red_chi2 slot %d" % slot] = e.channel_red_chi2(
                        dev, d["freqs"], d["P"], d["params"], d["nus"], d["scales"], d["errs"], slots=np.full(nsub, slot, dtype=np.int32))
                yield tag + (" split" if budget < 96e9 else ""), out
            e.set_option("max_work_bytes", 96e9)
    e.close()


def run(path):
    out = {}
    for name, r in fits():
        for key in KEYS:
            if key in r and r[key] is not None:
                v = r[key]
                out[name + "|" + key] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        print("ran", name, flush=True)
    for name, r in aux_calls():
        for key, v in r.items():
            out[name + "|" + key] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        print("ran", name, flush=True)
    np.savez(path, **out)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--run":
        return run(sys.argv[2])
    lib_a, lib_b = sys.argv[1], sys.argv[2]
    outdir = sys.argv[3] if len(sys.argv) > 3 else "."
    os.makedirs(outdir, exist_ok=True)
    paths = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        paths.append(os.path.join(outdir, "compare_%s.npz" % tag))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--run", paths[-1]], check=True, cwd=ROOT,
                       env=dict(os.environ, PP_TOAS_LIB=os.path.abspath(lib)))
    a, b = np.load(paths[0]), np.load(paths[1])
    bad = sorted(set(a.files) ^ set(b.files))
    cases = {}
    for key in sorted(set(a.files) & set(b.files)):
        try:
            np.testing.assert_array_equal(a[key], b[key])
            cases.setdefault(key.split("|")[0], []).append(None)
        except AssertionError:
            bad.append(key)
            cases.setdefault(key.split("|")[0], []).append(key)
    for name, res in cases.items():
        diff = [k.split("|")[1] for k in res if k]
        print("%-36s %2d arrays  %s" % (name, len(res), "DIFFER: " + " ".join(diff) if diff else "equal"))
    print("%s vs %s: %d cases, %d arrays, %d differ" % (lib_a, lib_b, len(cases), len(a.files), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
