"""The make_fake_pulsar goldens (tests/golden/ppfake_rows.npz, written by tests/golden/make_golden_ppfake.py from the
true reference) as the CPU and the GPU test take them."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARFILE = os.path.join(GOLDEN, "example.par")
GMODEL = os.path.join(GOLDEN, "example.gmodel")
_cache = {}


def cases():
    """{name: dict(kwargs=make_fake_pulsar's keyword arguments, gmodel=the model file's text, rows=[nchan, nbin],
    bar=max(10 self_dev, 1e-12), relative to the rows' peak)}, read once."""
    if not _cache:
        g = np.load(os.path.join(GOLDEN, "ppfake_rows.npz"))
        for name, c in json.loads(str(g["cases"])).items():
            rows = g[name + "_rows"]
            rows.setflags(write=False)
            _cache[name] = dict(kwargs=c["kwargs"], gmodel=c["gmodel"], rows=rows,
                                bar=max(10.0 * float(g[name + "_self_dev"]), 1e-12))
    return _cache


NAMES = ["%s_%d" % (c, nbin) for nbin in (64, 100)
         for c in ("plain", "dedispersed", "dm_nu", "t_scat", "scint_scales", "model_tau")]
