#!/usr/bin/env python3
"""Golden of the fit's residual portrait: run the TRUE reference's GetTOAs.get_TOAs on small synthetic archives
(make_golden_gettoas.py's recipe: a DataBunch built from arrays, PSRCHIVE patched away), then its
show_fit(isub, show=False, return_fit=True) (pptoas.py:1317-1419), and store the inputs, the fitted parameters and the
returned port and model_scaled in tests/golden/showfit.npz.

Cases (keys are prefixed with the case's name):
    zap      8 chan x  64 bin, phi + DM, two zapped channels in the subint shown
    gm       6 chan x 100 bin (a general row length), phi + DM + GM
    scat     8 chan x 128 bin, phi + DM + tau + alpha with log10_tau
    rot      the zap archive again, shown with rotate = 0.1

Build-container only (needs the reference); nothing of the reference's program text is written."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_gettoas as mgg  # noqa: E402

CASES = [
    # name, synth_archive keywords, zapped channels of subint 0, get_TOAs keywords, isub, rotate
    ("zap", dict(seed=71, nsub=3, C=8, B=64), [2, 5], dict(), 0, 0.0),
    ("gm", dict(seed=72, nsub=3, C=6, B=100, GM=0.25), [], dict(fit_GM=True), 0, 0.0),
    ("scat", dict(seed=73, nsub=3, C=8, B=128, tau_us=60.0),
     [], dict(fit_scat=True, log10_tau=True, scat_guess=(50e-6, 1500.0, -4.0)), 0, 0.0),
    ("rot", dict(seed=71, nsub=3, C=8, B=64), [2, 5], dict(), 0, 0.1),
]


def archive(ref, skw, zapped):
    """synth_archive with exactly the channels `zapped` of subint 0 at weight 0 and every other row in use."""
    data, arrays, scal = mgg.synth_archive(ref, **skw)
    w = np.ones_like(arrays["weights"])
    w[0, zapped] = 0.0
    arrays["weights"] = w
    data.weights = w
    data.masks = (w > 0)[:, None, :, None]
    data.ok_ichans = [np.where(w[i] > 0)[0] for i in range(len(w))]
    data.ok_isubs = np.arange(len(w))
    return data, arrays, scal


def main():
    ref, pptoas, tmp = mgg.import_pptoas()
    out = {}
    for name, skw, zapped, gkw, isub, rotate in CASES:
        data, arrays, scal = archive(ref, skw, zapped)
        pptoas.load_data = lambda *a, **k: data
        gt = pptoas.GetTOAs("fake.fits", os.path.join(mg.REF, "examples", "example.gmodel"), quiet=True)
        gt.get_TOAs(quiet=True, **gkw)
        port, model_scaled, ok_ichans, freqs, noise_stds = gt.show_fit("fake.fits", isub, rotate=rotate, show=False,
                                                                       return_fit=True, quiet=True)
        rec = dict(arrays)
        rec.update({"scal_" + k: np.asarray(v) for k, v in scal.items()})
        rec.update({"kw_" + k: np.asarray(v) for k, v in gkw.items()})
        for fld in ("phis", "DMs", "GMs", "taus", "alphas", "scales", "doppler_fs"):
            rec["out_" + fld] = np.asarray(getattr(gt, fld)[0], dtype=np.float64)
        rec["out_nu_refs"] = np.array([list(map(float, r)) for r in gt.nu_refs[0]])
        rec["out_ok_isubs"] = np.asarray(gt.ok_isubs[0])
        rec.update(isub=isub, rotate=rotate, bary=int(gt.bary), log10_tau=int(gt.log10_tau),
                   fit_port=np.asarray(port, dtype=np.float64), fit_model_scaled=np.asarray(model_scaled, dtype=np.float64),
                   fit_ok_ichans=np.asarray(ok_ichans), fit_freqs=np.asarray(freqs), fit_noise_stds=np.asarray(noise_stds))
        out.update({"%s_%s" % (name, k): v for k, v in rec.items()})
    mg.save("showfit", names=np.array([c[0] for c in CASES]), **out)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
