#!/usr/bin/env python3
"""Do two checkouts of the Python caller layer (engine.py, pptoas.py) return the same things?  (A refactor must.)

    python <this file> --run out.pkl [cpu|gpu]      in the root of the checkout under test (its package and its
                                                    tests/ are the ones imported: the working directory)
    python <this file> --compare a.pkl b.pkl        exit status 1 when an entry differs

--run executes one fixed list of calls and pickles what comes back.  "cpu" (the default) needs no device: get_TOAs
over fabricated fits (tests/test_pptoas_run_cpu.py's _StubGetTOAs) -- every result list, the .tim line of every TOA
and what was printed.  "gpu": fit_batch, enqueue x 3 + collect x 3 and submit + wait over host arrays and device
tensors with each optional argument, every auxiliary Engine method (tools/compare_builds.py's list), get_TOAs for
.gmodel and .spl templates, get_narrowband_TOAs and get_channels_to_zap, in seconds-sized shapes.
--compare wants assert_array_equal on every array and == on everything else.  Wall-clock values are left out: the
`duration` / `fit_durations` entries, and the digits of the two printed timing lines.
"""
import contextlib
import io
import os
import pickle
import re
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
GOLDEN = os.path.join(os.getcwd(), "tests", "golden")
TIMING = ("duration", "fit_durations")


def plain(x):
    """x as arrays, strings, numbers, lists and dicts only."""
    from pulseportraiture_amd import pptoas
    if isinstance(x, str):
        return x.replace(os.getcwd(), ".")      # (the template's path is a flag of every TOA)
    if isinstance(x, (pptoas.MJD, type(None), bytes, bool, int, float)):
        return repr(x) if isinstance(x, pptoas.MJD) else x
    if isinstance(x, pptoas.TOA):
        return {"line": plain(pptoas.toa_string(x)), "flags": list(x.flags)}
    if hasattr(x, "cpu"):
        return x.cpu().numpy()
    if isinstance(x, np.ndarray) and x.dtype != object:
        return x
    if isinstance(x, (np.ndarray, list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    d = x if isinstance(x, dict) else vars(x)
    return {k: plain(v) for k, v in d.items() if k not in TIMING}


def printed(fn):
    """(what fn() printed, the digits of the timing lines masked)."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn()
    return [re.sub(r"[0-9.]+", "#", ln) if ln.startswith(("~", "Total time")) else ln
            for ln in buf.getvalue().splitlines()]


def snapshot(gt, out):
    skip = ("datafiles", "modelfile", "quiet") + TIMING
    snap = plain({k: v for k, v in vars(gt).items() if not k.startswith("_") and k not in skip})
    snap["printed"] = out
    return snap


def cpu_calls():
    from tests.test_pptoas_run_cpu import _ARCHIVE_SPEC, _KW, _SUBINT_SPEC, MODEL, _StubGetTOAs, _archives
    scat = dict(_KW, fit_scat=True)
    cases = [("KW", _KW), ("KW loud", dict(_KW, quiet=False)), ("scat log10", scat), ("scat linear", dict(scat, log10_tau=False)),
             ("parangle", dict(_KW, print_parangle=True)), ("nu_refs None", dict(_KW, nu_refs=None)), ("bary off", dict(_KW, bary=False))]
    for sname, spec in (("archives", _ARCHIVE_SPEC), ("subints", _SUBINT_SPEC)):
        for name, kw in cases:
            gt = _StubGetTOAs(_archives(spec), MODEL, quiet=True)
            out = printed(lambda: gt.get_TOAs(**kw))
            yield "get_TOAs stub %s %s" % (sname, name), snapshot(gt, out)


def attempt(fn):
    """fn()'s result, or the refusal it raised (a refusal must stay the same refusal; a HIP error ends the run)."""
    from pulseportraiture_amd import _lib
    from pulseportraiture_amd.engine import EngineError
    try:
        return plain(fn())
    except Exception as err:
        if "failed (%d)" % _lib.PP_EHIP in str(err) or (isinstance(err, RuntimeError) and not isinstance(err, EngineError)):
            raise
        return "%s: %s" % (type(err).__name__, err)


def fit_calls():
    import torch
    from pulseportraiture_amd import gmodel
    from pulseportraiture_amd.engine import Engine
    e = Engine(0)
    # (256 x 2048: the smallest shape at which a ref_seed batch has its single-pass path; elsewhere it is refused)
    for (C, B), nsub in (((64, 256), 6), ((24, 100), 4), ((256, 2048), 4)):
        freqs, model, _ = gmodel.example_model(C, B)
        e.set_model(model)
        rng = np.random.default_rng(C)
        host = model[None] * rng.uniform(0.5, 2.0, (nsub, C, 1)) + 0.02 * rng.standard_normal((nsub, C, B))
        P, x0 = np.full(nsub, 0.004), np.zeros((nsub, 5))
        errs = np.full((nsub, C), 0.02)
        mask = np.ones((nsub, C), dtype=np.uint8)
        mask[:, ::7] = 0
        seed = dict(weights=mask.astype(np.float64), model_profs=model.mean(axis=0), Ns=100, finish='simplex',
                    nu_mean=np.array([freqs[m > 0].mean() for m in mask]))
        dev = lambda a: torch.as_tensor(a, device="cuda:0")  # noqa: E731
        base = dict(nu_fits=np.full((nsub, 3), freqs.mean()), fit_flags=[1, 1, 0, 0, 0])
        for dtype in (np.float64, np.float32):
            for where in ("host", "device"):
                data = host.astype(dtype) if where == "host" else dev(host.astype(dtype))
                options = [("plain", dict(base, errs=errs)),
                           ("mask ref_seed", dict(base, errs=errs, chan_mask=mask, ref_seed=seed)),
                           ("measured noise objective", dict(base, chan_mask=mask, objective=True, per_channel=False)),
                           ("device aux records", lambda: dict(base, errs=dev(errs), chan_mask=dev(mask), per_channel="device",
                                                               records=torch.zeros((nsub, 18), dtype=torch.float64, device="cuda:0"))),
                           ("device aux ref_seed", lambda: dict(base, errs=dev(errs), chan_mask=dev(mask),
                                                                ref_seed=dict(seed, weights=dev(seed["weights"]))))]
                for oname, opt in options:
                    tag = "%dx%d %s %s %s" % (C, B, np.dtype(dtype).name, where, oname)
                    make = opt if callable(opt) else (lambda opt=opt: opt)

                    def fit(call):
                        kw = make()
                        r = call(kw)
                        return dict(r, records=kw["records"]) if isinstance(r, dict) and "records" in kw else r

                    yield tag + " fit_batch", attempt(lambda: fit(lambda kw: e.fit_batch(data, freqs, P, x0, **kw)))

                    def submit(kw):
                        e.submit(data, freqs, P, x0, **kw)
                        return e.wait()
                    yield tag + " submit wait", attempt(lambda: fit(submit))
                    queued = [attempt(lambda: fit(lambda kw: e.enqueue(data, freqs, P, x0, **kw))) for _ in range(3)]
                    yield tag + " enqueue", queued + [attempt(e.collect) for q in queued if q is None]
    e.close()


def _bunch(C, B, nsub, seed, dmc=0):
    from pulseportraiture_amd import gmodel, pptoas
    freqs, model, P0 = gmodel.example_model(C, B)
    rng = np.random.default_rng(seed)
    sub = model[None, None] * rng.uniform(0.5, 2.0, (nsub, 1, C, 1)) + 0.05 * rng.standard_normal((nsub, 1, C, B))
    w = np.ones((nsub, C))
    w[1, 3:6] = 0
    w[2] = 0
    w[3, 2:] = 0           # (a two-channel subint: the flag carry)
    return pptoas.data_from_arrays(
        sub, freqs, np.full(nsub, P0) * (1 + 1e-3 * np.arange(nsub)), [pptoas.MJD(58000 + i, 0.25) for i in range(nsub)],
        weights=w, noise_stds=np.full((nsub, 1, C), 0.05), SNRs=np.ones((nsub, 1, C)), DM=10.0, dmc=dmc,
        doppler_factors=1.0 + 1e-4 * np.arange(nsub), bw=800.0, nu0=1500.0, subtimes=np.full(nsub, 60.0),
        parallactic_angles=np.arange(nsub, dtype=float), filename="fake%d.fits" % seed)


def caller_calls():
    from pulseportraiture_amd.pptoas import GetTOAs
    models = [os.path.join(GOLDEN, "example.gmodel"), os.path.join(GOLDEN, "example.spl")]
    all_flags = dict(print_phase=True, print_flux=True, print_parangle=True, nu_refs=(1500.0, None), addtnl_toa_flags={"pta": "X"})
    for (C, B), nsub in (((24, 100), 5), ((64, 256), 8)):
        for model in models:
            for seed in ("reference", "device"):
                cases = [("plain", {}), ("flags GM", dict(all_flags, fit_GM=True)), ("response", dict(add_instrumental_response=True))]
                if model.endswith(".gmodel"):
                    cases += [("scat", dict(all_flags, fit_scat=True)), ("scat linear", dict(fit_scat=True, log10_tau=False))]
                for name, kw in cases:
                    gt = GetTOAs([_bunch(C, B, nsub, 1), _bunch(C, B, nsub, 2, dmc=1)], model, quiet=True)
                    if "add_instrumental_response" in kw:
                        gt.ird.update(DM=30.0, wids=[2.0 / B], irf_types=['rect'])
                    tag = "%dx%d %s seed=%s %s" % (C, B, os.path.basename(model), seed, name)
                    out = attempt(lambda: printed(lambda: gt.get_TOAs(quiet=False, seed=seed, **kw)))
                    if isinstance(out, list):
                        attempt(gt.get_channels_to_zap)
                    yield "get_TOAs + zap " + tag, snapshot(gt, out)
            gt = GetTOAs([_bunch(C, B, nsub, 1), _bunch(C, B, nsub, 2, dmc=1)], model, quiet=True)
            out = attempt(lambda: printed(lambda: gt.get_narrowband_TOAs(quiet=False, print_parangle=True,
                                                                         addtnl_toa_flags={"pta": "X"})))
            yield "narrowband %dx%d %s" % (C, B, os.path.basename(model)), snapshot(gt, out)


def aux_calls():
    sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
    import compare_builds
    for name, out in compare_builds.aux_calls():
        yield name, plain(out)


def run(path, which):
    lists = (cpu_calls,) if which == "cpu" else (fit_calls, aux_calls, caller_calls)
    out = {}
    for calls in lists:
        for name, got in calls():
            assert name not in out, name
            out[name] = got
            print("ran", name, flush=True)
    with open(path, "wb") as fh:
        pickle.dump(out, fh)


def differences(a, b, where):
    """Paths at which a and b differ."""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        try:
            np.testing.assert_array_equal(a, b)
            return [] if a.dtype == b.dtype else [where + " (dtype)"]
        except AssertionError:
            return [where]
    if type(a) is not type(b):
        return [where + " (type)"]
    if isinstance(a, dict):
        return [where + " (keys)"] if list(a) != list(b) else \
            [p for k in a for p in differences(a[k], b[k], "%s|%s" % (where, k))]
    if isinstance(a, list):
        return [where + " (length)"] if len(a) != len(b) else \
            [p for i, (u, v) in enumerate(zip(a, b)) for p in differences(u, v, "%s[%d]" % (where, i))]
    return [] if a == b or (isinstance(a, float) and a != a and b != b) else [where]


def compare(path_a, path_b):
    with open(path_a, "rb") as fa, open(path_b, "rb") as fb:
        a, b = pickle.load(fa), pickle.load(fb)
    bad = ["%s (only in one)" % k for k in sorted(set(a) ^ set(b))]
    for name in [k for k in a if k in b]:
        diff = differences(a[name], b[name], name)
        print("%-72s %s" % (name, "DIFFER: " + " ".join(diff[:6]) if diff else "equal"))
        bad += diff
    print("%s vs %s: %d entries, %d differing" % (path_a, path_b, len(a), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "cpu")
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
