#!/usr/bin/env python3
"""Goldens of the JOINED Gaussian fit from the TRUE reference: one .gmodel fitted to several bands at once, every
band with a phase offset and a Delta-DM of its own (the "join" paths: gen_gaussian_portrait(..., join_ichans, P),
fit_gaussian_portrait(join_params=...), the metafile branch of DataPortrait, the njoin branches of make_gaussian_model,
write_join_parameters).  The reference runs as in make_golden_ppgauss.py, whose helpers this script imports: converted
to Python 3 in a scratch directory, lmfit replaced by that script's stand-in, every fit solved twice.

    ppgauss_join_rows.npz          fit_gaussian_portrait_function with join_ichans on 7 channels (band 0 = [0, 1, 3],
                                   band 1 = [2, 4, 5], channel 6 in no band) at 64 and 100 bins, codes 000 and 011, the
                                   edge model with and without tau: a base vector (phase2 = 0.37, DM1 = 2e-3, DM2 =
                                   -3e-3), six vectors with one parameter stepped (phase2, DM1, DM2, tau, a loc, the
                                   scattering index) and a base with every join parameter zero
    ppgauss_join_fit_2x8x128.npz   example pulsar, sigma 0.05, two bands of 8 channels, fixloc: inputs, both solves, scatter
    ppgauss_join_fit_3x6x100.npz   ... three bands of 6 channels, 100 bins
    ppgauss_join_model.npz         DataPortrait(metafile) of the two-band case (channels stored in descending order, so
     + ppgauss_join_model.join     that the sort is no identity) and make_gaussian_model(modelfile, niter=1): index
                                   lists, initial join parameters, every pass of check_convergence, the final model and
                                   join parameters, the .join file; and the index lists of the same bands with one
                                   channel zapped

In every fit band 1 has its phase fixed at 0 and its Delta-DM free, the other bands both free; all location slopes are
fixed (with them free a common Delta-DM is nearly degenerate with the slopes, and the reference's two solves part by
7e-4 sigma).  The asserts are make_golden_ppgauss.py's: chi^2/dof within 0.9 ... 1.1, self-scatter < 1e-4 sigma, the two
solves' errors within 1e-5.

Build-container only (needs the reference sources)."""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_ppgauss as mgg  # noqa: E402
from make_golden_ppgauss import EDGE, P_EXAMPLE, SIGMA  # noqa: E402

# ---- residual rows ----------------------------------------------------------------
ROW_FREQS = np.linspace(1180.0, 1820.0, 7)
ROW_ERRS = np.array([0.05, 0.07, 0.11, 0.06, 0.09, 0.05, 0.08])
ROW_BANDS = [[0, 1, 3], [2, 4, 5]]
ROW_JOIN = [0.0, 2e-3, 0.37, -3e-3]             # phase1, DM1, phase2, DM2
NEDGE = 2 + 6 * len(EDGE["comps"])
# the stepped entries of [DC, tau, comps ..., phase1, DM1, phase2, DM2, scattering index] and the size of each step:
# phase2, DM1, DM2, tau, a loc, the scattering index
ROW_STEPS = [(NEDGE + 2, 1e-3), (NEDGE + 1, 1e-4), (NEDGE + 3, 1e-4), (1, 0.3), (2 + 6, 1e-3), (-1, 0.05)]


def rows_golden(ref):
    store = {}
    rng = np.random.default_rng(mg.SEED + 900)
    nchan = len(ROW_FREQS)
    for nbin in (64, 100):
        phases = ref.get_bin_centers(nbin)
        data = rng.standard_normal((nchan, nbin)) * ROW_ERRS[:, None] + 0.3 * np.sin(2 * np.pi * phases)[None]
        errs = np.outer(ROW_ERRS, np.ones(nbin))
        for code in ("000", "011"):
            for tau_bins in (0.0, 0.9):
                base = np.array([EDGE["dc"], tau_bins] + list(np.ravel(EDGE["comps"])) + ROW_JOIN + [EDGE["alpha"]])
                sets = [base]
                for idx, step in ROW_STEPS:
                    v = base.copy()
                    v[idx] += step
                    sets.append(v)
                zero = base.copy()
                zero[NEDGE:NEDGE + 4] = 0.0
                sets = np.array(sets + [zero])
                with np.errstate(invalid="ignore"):
                    rows = np.array([ref.fit_gaussian_portrait_function(
                        mgg.params_of(ref, v), code, phases, ROW_FREQS, EDGE["nu_ref"], data=data, errs=errs,
                        join_ichans=ROW_BANDS, P=P_EXAMPLE) for v in sets])
                    # (the all-zero vector is the unjoined model: rotate_data by nothing is a transform there and back)
                    plain = ref.fit_gaussian_portrait_function(
                        mgg.params_of(ref, np.delete(zero, np.s_[NEDGE:NEDGE + 4])), code, phases, ROW_FREQS, EDGE["nu_ref"],
                        data=data, errs=errs, join_ichans=[], P=None)
                assert np.all(np.isfinite(rows)), (nbin, code, tau_bins)
                assert np.abs(rows[-1] - plain).max() < 1e-13 * np.abs(plain).max()
                tag = "n%d_c%s_t%d" % (nbin, code, int(tau_bins != 0.0))
                # sets: the base and the six steps; zero_set / zero_rows: the base with every join parameter zero
                store[tag + "_sets"], store[tag + "_rows"] = sets[:-1], rows[:-1]
                store[tag + "_zero_set"], store[tag + "_zero_rows"] = sets[-1], rows[-1]
        store["n%d_data" % nbin] = data
    store.update(errs=ROW_ERRS, freqs=ROW_FREQS, band0=np.array(ROW_BANDS[0]), band1=np.array(ROW_BANDS[1]),
                 nu_ref=EDGE["nu_ref"], P=P_EXAMPLE)
    mg.save("ppgauss_join_rows", **store)


# ---- fits -------------------------------------------------------------------------
JOIN_TRUTH = [0.0, 2e-4, 0.013, -3e-4, -0.021, 1e-4]        # phase and Delta-DM of up to three bands


def join_case(ref, nband, nchan_band, nbin, seed):
    """nband adjacent bands of nchan_band channels over 1100 ... 1900 MHz, every band rotated by its own phase and
    Delta-DM; the start is the truth, every free parameter moved by 0.3 % (the join parameters by a few of their errors)."""
    code, nu_ref, truth, alpha = mgg.example_truth(ref)
    truth = truth.copy()
    truth[1] = 0.0
    edges = np.linspace(1100.0, 1900.0, nband + 1)
    freqs = np.concatenate([mgg.band(nchan_band, nu0=0.5 * (lo + hi), bw=hi - lo) for lo, hi in zip(edges[:-1], edges[1:])])
    join_ichans = [np.arange(i * nchan_band, (i + 1) * nchan_band) for i in range(nband)]
    join_truth = np.array(JOIN_TRUTH[:2 * nband])
    phases = ref.get_bin_centers(nbin)
    rng = np.random.default_rng(seed)
    clean = ref.gen_gaussian_portrait(code, np.append(truth, join_truth), alpha, phases, freqs, nu_ref, join_ichans, P_EXAMPLE)
    data = clean + SIGMA * rng.standard_normal(clean.shape)
    flags = np.ones(len(truth))
    flags[1] = 0.0
    flags[3::6] = 0                                             # fixloc
    init = np.where(flags != 0, truth * (1.0 + 0.003 * rng.standard_normal(len(truth))), truth)
    join_flags = np.ones(2 * nband)
    join_flags[0] = 0                                           # band 1: the phase reference
    join_init = join_truth + join_flags * np.tile([2e-4, 2e-5], nband) * rng.standard_normal(2 * nband)
    errs = np.full(clean.shape, SIGMA)
    return dict(seed=seed, code=code, nu_ref=nu_ref, truth=truth, alpha=alpha, freqs=freqs, phases=phases, data=data, flags=flags,
                init=init, errs=errs, join_ichans=join_ichans, join_truth=join_truth, join_init=join_init,
                join_flags=join_flags)


def solve_both(ref, c):
    """make_golden_ppgauss.solve_both for a joined fit: the stand-in's solve, then trf on the same objective; the
    same asserts.  Returns (stand-in result, trf result, self-scatter in sigma); the vectors carry the join parameters."""
    args = (c["code"], c["data"], c["init"], c["alpha"], c["errs"], c["flags"], False, c["phases"], c["freqs"], c["nu_ref"])
    kw = dict(join_params=[c["join_ichans"], c["join_init"], c["join_flags"]], P=P_EXAMPLE, quiet=True)
    a = ref.fit_gaussian_portrait(*args, **kw)
    true_min = ref.lm.minimize
    ref.lm.minimize = lambda fn, params, kws=None: mgg.minimize_trf(fn, params, kws)
    try:
        b = ref.fit_gaussian_portrait(*args, **kw)
    finally:
        ref.lm.minimize = true_min
    for r in (a, b):
        assert 0.9 < r.chi2 / r.dof < 1.1, r.chi2 / r.dof
    full_a, full_b = np.append(a.fitted_params, a.scattering_index), np.append(b.fitted_params, b.scattering_index)
    errs_a, errs_b = np.append(a.fit_errs, a.scattering_index_err), np.append(b.fit_errs, b.scattering_index_err)
    varied = errs_a > 0
    scatter = np.zeros(len(full_a))
    scatter[varied] = np.abs(full_a - full_b)[varied] / errs_a[varied]
    assert scatter.max() < 1e-4, scatter
    assert np.abs(errs_b[varied] / errs_a[varied] - 1.0).max() < 1e-5, errs_b[varied] / errs_a[varied] - 1.0
    n = len(c["init"])
    for idx, lo, hi in [(range(4, n, 6), 0.0, ref.wid_max), (range(6, n, 6), 0.0, np.inf)]:
        for i in idx:
            if errs_a[i] > 0:
                assert full_a[i] - lo > 5 * errs_a[i] and hi - full_a[i] > 5 * errs_a[i], (i, full_a[i], errs_a[i])
    return a, b, scatter


def fit_golden(ref, name, c):
    a, b, scatter = solve_both(ref, c)
    store = dict(code=np.array(c["code"]), nu_ref=c["nu_ref"], truth=c["truth"], freqs=c["freqs"], data=c["data"],
                 errs=c["errs"][:, 0], fit_flags=c["flags"], init_params=c["init"], scattering_index_in=c["alpha"], P=P_EXAMPLE,
                 seed=c["seed"],
                 join_truth=c["join_truth"], join_init=c["join_init"], join_flags=c["join_flags"],
                 fitted_params=a.fitted_params, fit_errs=a.fit_errs, chi2=a.chi2, dof=a.dof,
                 scattering_index=a.scattering_index, scattering_index_err=a.scattering_index_err,
                 trf_fitted_params=b.fitted_params, trf_fit_errs=b.fit_errs, trf_chi2=b.chi2, self_scatter=scatter)
    for i, ic in enumerate(c["join_ichans"]):
        store["join_ichans%d" % i] = ic
    mg.save("ppgauss_join_fit_" + name, **store)
    print("   ", name, "chi2/dof %.4f" % (a.chi2 / a.dof), "self-scatter max %.1e sigma" % scatter.max(),
          "| d chi2 %.1e" % (a.chi2 - b.chi2), "| join", a.fitted_params[-len(c["join_init"]):])
    return a


def first_case(ref, name, nband, nchan_band, nbin, seed):
    """The golden of the first seed from `seed` on whose two solves meet every assert of solve_both (MINPACK's stop at
    its default tolerances leaves some inputs further than 1e-4 sigma from the tight solve; such a seed would pin the
    optimiser, not the minimum)."""
    while True:
        c = join_case(ref, nband, nchan_band, nbin, seed)
        try:
            fit_golden(ref, name, c)
        except AssertionError as e:
            print("    %s: seed %d fails an assert of the two solves (%s ...), trying the next" % (name, seed, str(e)[:60]))
            seed += 1
            continue
        print("    %s: seed %d" % (name, seed))
        return c


# ---- the metafile branch of DataPortrait and make_gaussian_model ---------------------
def bunches_of(ref, c, zap=None):
    """The DataBunch load_data would return for every band of case c, its channels in descending order (a negative
    bandwidth, as many receivers record); zap = (band, channel of the band as stored) gets weight 0."""
    out = {}
    nbin = c["data"].shape[1]
    for i, ic in enumerate(c["join_ichans"]):
        ic = ic[::-1]
        nchan = len(ic)
        sub = c["data"][ic]
        w = np.ones(nchan)
        if zap is not None and zap[0] == i:
            w[zap[1]] = 0.0
        ok = np.flatnonzero(w > 0)
        freqs = c["freqs"][ic]
        snrs = np.array([ref.get_SNR(row) for row in sub])
        name = "band%d.npz" % (i + 1)
        out[name] = ref.DataBunch(
            nchan=nchan, nbin=nbin, nsub=1, npol=1, ok_ichans=[ok], ok_isubs=np.array([0]), DM=0.0, phases=c["phases"],
            prof=np.average(sub[ok], axis=0, weights=w[ok]), source="PSR_1234-5678", Ps=np.array([P_EXAMPLE]),
            freqs=freqs[None], bw=-abs(freqs[0] - freqs[1]) * nchan, nu0=freqs.mean(),
            masks=(w[:, None] * np.ones(nbin))[None, None], subints=sub[None, None].copy(), flux_prof=sub.mean(axis=1),
            noise_stds=np.full((1, 1, nchan), SIGMA), SNRs=snrs[None, None], weights=w[None])
    return out


def data_portrait(ref, refgauss, bunches, tmp, joinfile=None):
    meta = os.path.join(tmp, "bands.meta")
    with open(meta, "w") as fh:
        fh.write("".join(name + "\n" for name in bunches))
    ref.file_is_type = lambda f, t: True
    ref.load_data = lambda name, **kw: bunches[name]
    return refgauss.DataPortrait(meta, joinfile=joinfile, quiet=True)


def model_golden(ref, refgauss, c, tmp):
    np.float = float                # (NumPy 2 has none; the reference's joinfile reader would print "Bad join file.")
    store = {}
    # the index lists with a zapped channel: band 2's third channel as stored
    dz = data_portrait(ref, refgauss, bunches_of(ref, c, zap=(1, 2)), tmp)
    for i in range(dz.njoin):
        store["zap_join_ichans%d" % i], store["zap_join_ichanxs%d" % i] = dz.join_ichans[i], dz.join_ichanxs[i]
    store.update(zap_isort=dz.isort, zap_isortx=dz.isortx, zap_join_nchans=np.array(dz.join_nchans),
                 zap_join_nchanxs=np.array(dz.join_nchanxs), zap_join_params=dz.join_params, zap_freqsx=dz.freqsxs[0],
                 zap_band=1, zap_chan=2)
    # the whole route without one
    bunches = bunches_of(ref, c)
    for i, b in enumerate(bunches.values()):
        store["band%d_subints" % i], store["band%d_freqs" % i], store["band%d_SNRs" % i] = b.subints, b.freqs, b.SNRs
    dp = data_portrait(ref, refgauss, bunches, tmp)
    for i in range(dp.njoin):
        store["join_ichans%d" % i], store["join_ichanxs%d" % i] = dp.join_ichans[i], dp.join_ichanxs[i]
    store.update(isort=dp.isort, isortx=dp.isortx, join_params_init=dp.join_params.copy(), join_fit_flags=dp.join_fit_flags,
                 Ps=np.array(dp.Ps), nu0=dp.nu0, bw=dp.bw, freqs=dp.freqs, port_in=dp.port.copy(), noise_std=SIGMA)
    start = os.path.join(tmp, "start.gmodel")
    ref.write_model(start, "PSR_1234-5678", c["code"], c["nu_ref"], c["init"], c["flags"], c["alpha"], 0, quiet=True)
    store["start_gmodel"] = np.frombuffer(open(start, "rb").read(), dtype=np.uint8)
    passes = []
    check = refgauss.DataPortrait.check_convergence

    def recorded(self, *a, **k):
        cnv = check(self, *a, **k)
        passes.append([self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2, 1.0 if cnv else 0.0])
        return cnv
    refgauss.DataPortrait.check_convergence = recorded
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        dp.make_gaussian_model(modelfile=start, niter=1, writemodel=False, writeerrfile=False, quiet=True)
    finally:
        os.chdir(cwd)
        refgauss.DataPortrait.check_convergence = check
    passes = np.array(passes)
    # no pass decides its convergence on a near-tie
    assert np.all(np.abs(np.abs(passes[:, 0]) / passes[:, 1] - 1.0) > 0.05), passes
    assert np.all(np.abs(np.abs(passes[:, 2]) / passes[:, 3] - 1.0) > 0.05), passes
    joinfile = os.path.join(tmp, dp.model_name + ".join")
    text = open(joinfile, "rb").read()
    shutil.copy(joinfile, os.path.join(HERE, "ppgauss_join_model.join"))
    # what the reference reads back from its own file
    back = data_portrait(ref, refgauss, bunches, tmp, joinfile=joinfile)
    store.update(passes=passes, nu_fit=dp.nu_fit, model_params=dp.model_params, model_param_errs=dp.model_param_errs,
                 join_params=dp.join_params, join_param_errs=dp.join_param_errs, scattering_index=dp.scattering_index,
                 chi2=dp.chi2, dof=dp.dof, model=dp.model, port_out=dp.port, portx_out=dp.portx,
                 join_text=np.frombuffer(text, dtype=np.uint8), join_params_read=back.join_params)
    mg.save("ppgauss_join_model", **store)
    print("    model passes (phi, phierr, DM, DMerr, red_chi2, converged):\n", passes)
    print("    join parameters", dp.join_params, "read back", back.join_params)


def main():
    ref, refgauss, lm, tmp = mgg.import_ppgauss()
    rows_golden(ref)
    ca = first_case(ref, "2x8x128", 2, 8, 128, 901)
    cb = first_case(ref, "3x6x100", 3, 6, 100, 902)
    model_golden(ref, refgauss, ca, tmp)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
