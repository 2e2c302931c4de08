#!/usr/bin/env python3
"""Golden of the 'fit' noise method: the TRUE reference's find_kc, get_noise_fit and get_noise(method='fit').

Build-container only (needs the reference); see make_golden.py for how the reference is imported.

    python tests/golden/make_golden_noisefit.py      # writes tests/golden/noisefit.npz

For each row length of noisefit_refs.LENGTHS_FIXTURE (64, 100, 256, 1000): rows_<nbin> = 8 Gaussian pulses of width
0.02 - 0.15 rot and amplitude 1 - 100 sigma, then noisefit_refs.SPECIAL (pure noise, a constant row, an all-zero row,
an integer-valued row with zero sum, a row whose winner has b = 0).  For each of 'exp_dc' and 'half_tri':
kc_<fn>_<nbin> (find_kc), cell_<fn>_<nbin> (ia, ib, idc: the argmin of the grid find_kc hands to opt.brute, asked
for with full_output=True and the reference's own find_kc_function) and chi2_<fn>_<nbin> [n,2], the chi-squared of
the best and of the runner-up width (each minimised over b and dc).  noise_1d_<nbin> = get_noise_fit(row),
noise_chans_<nbin> = get_noise_fit(rows, chans=True), noise_get_<nbin> = get_noise(row, method='fit'); fkf_* are
find_kc_function and half_triangle_function at one fixed point.

The script asserts what the fixture is there to pin: the zero-sum and all-zero rows have kc = H - 1 and cell 0, the
b = 0 row has ib = 0 and ia = 0, and the all-zero row has noise 0.
"""
import os
import shutil
import sys
import warnings

import numpy as np
import scipy.optimize as opt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from tests import noisefit_refs as nf  # noqa: E402

NPULSE = 8


def brute_cell(ref, pows, fn):
    """The grid search exactly as find_kc sets it up (pplib.py:1474-1485), with the grid kept."""
    data = np.log10(pows)
    lo_hi = (len(data) ** -1, 1.0) if fn == 'exp_dc' else (1, len(data))
    ranges = [tuple(lo_hi), tuple((0, data.max() - data.min())), tuple((data.min(), data.max()))]
    x0, fval, grid, J = opt.brute(ref.find_kc_function, ranges, args=[data, 1.0, fn], Ns=20, full_output=True,
                                  finish=None)
    flat = int(np.argmin(J.ravel()))
    per_a = np.sort(J.reshape(20, -1).min(axis=1))
    return (flat // 400, (flat // 20) % 20, flat % 20), per_a[:2]


def main():
    warnings.simplefilter("ignore")
    ref, tmp = mg.import_reference()
    out = {}
    for nbin in nf.LENGTHS_FIXTURE:
        H = nbin // 2 + 1
        rows = np.concatenate([nf.pulse_rows(nbin, NPULSE, mg.SEED + nbin), nf.special_rows(nbin, mg.SEED + 7 * nbin)])
        out["rows_%d" % nbin] = rows
        spec = {name: NPULSE + i for i, name in enumerate(nf.SPECIAL)}
        for fn in nf.FNS:
            kcs, cells, chi2s = [], [], []
            for row in rows:
                pows = nf.power_spectrum(row)
                with np.errstate(all="ignore"):
                    kcs.append(int(ref.find_kc(pows, fn=fn)))
                    cell, two = brute_cell(ref, pows, fn)
                cells.append(cell)
                chi2s.append(two)
            kcs, cells = np.array(kcs, dtype=np.int32), np.array(cells, dtype=np.int32)
            out["kc_%s_%d" % (fn, nbin)], out["cell_%s_%d" % (fn, nbin)] = kcs, cells
            out["chi2_%s_%d" % (fn, nbin)] = np.array(chi2s)
            for name in ("zeros", "zero_sum_int"):
                assert tuple(cells[spec[name]]) == (0, 0, 0), (nbin, fn, name, cells[spec[name]])
            if fn == 'exp_dc':
                assert kcs[spec["zeros"]] == H - 1 and kcs[spec["zero_sum_int"]] == H - 1, (nbin, kcs)
                assert cells[spec["b0"]][0] == 0 and cells[spec["b0"]][1] == 0, (nbin, cells[spec["b0"]])
            print(nbin, fn, "kc", kcs, "cells", cells.tolist())
        with np.errstate(all="ignore"):
            out["noise_1d_%d" % nbin] = np.array([ref.get_noise_fit(row) for row in rows])
            out["noise_chans_%d" % nbin] = ref.get_noise_fit(rows, chans=True)
            out["noise_get_%d" % nbin] = np.array([ref.get_noise(row, method='fit') for row in rows])
        assert out["noise_1d_%d" % nbin][spec["zeros"]] == 0.0
        print(nbin, "noise", out["noise_1d_%d" % nbin])
    # the two host definitions at one fixed point
    data = np.log10(nf.power_spectrum(out["rows_64"][0]))
    point = (0.3, 1.7, -0.4)
    out["fkf_data"], out["fkf_point"] = data, np.array(point)
    out["fkf_exp_dc"] = ref.find_kc_function(point, data, 1.0, 'exp_dc')
    out["fkf_exp_dc_errs2"] = ref.find_kc_function(point, data, 2.0, 'exp_dc')
    out["fkf_half_tri"] = ref.find_kc_function((7.6, 1.7, -0.4), data, 1.0, 'half_tri')
    out["half_triangle"] = ref.half_triangle_function(7.6, 1.7, -0.4, 33)
    mg.save("noisefit", **out)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
