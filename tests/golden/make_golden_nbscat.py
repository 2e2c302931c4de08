#!/usr/bin/env python3
"""Goldens of the narrowband scattering fit (pp_fit_phase_tau_batch, get_narrowband_TOAs(fit_scat=True)):
the TRUE reference's fit_portrait_full on ONE-channel portraits, fit_flags [1,0,0,1,0], freqs = nu_fits =
nu_outs = the channel's frequency -- exactly the fit the reference's narrowband path sketches and cannot run.

Build-container only (needs /root/reference); see make_golden.py for how the reference is imported.

    python tests/golden/make_golden_nbscat.py      # writes tests/golden/nbscat_*.npz

nbscat_fits.npz      24 problems from example.gmodel (unscattered template): nbin 256 / 100 / 1024, both log10_tau
                     settings, tau 0.004 .. 0.03 rot, every channel's S/N >= 30 (sigma 0.02; 0.1 at 1024 bins).  At
                     256 and 100 bins the tau = 0.004 cases start from a guess of 0 (linear) or 1 / nbin (log10); at
                     1024 bins the reference itself does not get home from there.  Reference outputs under three
                     variants: trust-ncg, Newton-CG, trust-ncg from a start displaced by +1e-3 rot in phi; and
                     f, grad f, Hess f at three fixed points per case.
nbscat_gettoas_{log10,lin}.npz   a 3 x 8 x 256 archive scattered as nu^-4 (subint 2 zapped, channels masked), the
                     reference's one-channel fit for every good (subint, channel) with the caller's guess recipe.

A guess of tau = 0 with linear tau cannot be given to the reference: its derivative code returns zeros at tau = 0
(the `if taus.sum()` branches, pptoaslib.py:251, 325, 341), the tau rows of its Hessian vanish and its covariance
inversion raises LinAlgError.  For those cases the reference starts from tau = 1 / nbin -- the rule log10_tau applies
to a zero guess -- while the stored guess, which the device gets, is 0: the optimum does not depend on the start.

The script asserts, for every case and variant: a return code the reference treats as success (1, 2, 4), the
injection recovered within 5 sigma, and the variants agreeing to < 1e-4 sigma.  No case may be left out downstream.
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import make_golden_gettoas as mgt  # noqa: E402
from tests import nbscat_ref as nr  # noqa: E402

GMODEL = os.path.join(mg.REF, "examples", "example.gmodel")
P_EXAMPLE = 1.0 / 345.67890123456789
VARIANTS = ("trust-ncg", "Newton-CG", "trust-ncg+1e-3")
FIELDS = nr.COLS


def unscattered_model(ref, freqs, nbin):
    name, code, nu_ref, ngauss, gparams, fit_flags, alpha, fit_alpha = ref.read_model(GMODEL, quiet=True)
    up = np.copy(gparams)
    up[1] = 0.0
    return ref.gen_gaussian_portrait(code, up, 0.0, ref.get_bin_centers(nbin), freqs, nu_ref)


def one_channel_fit(ref, prof, mprof, nu, P, sigma, x0, log10_tau, method):
    freqs = np.array([nu])
    r = ref.fit_portrait_full(prof[None], mprof[None], [x0[0], 0.0, 0.0, x0[1], 0.0], P, freqs, [nu] * 3, [nu] * 3,
                              np.array([sigma]), [1, 0, 0, 1, 0], [(None, None)] * 5, log10_tau, option=0,
                              sub_id=None, method=method, is_toa=True, quiet=True)
    return np.array([r.phi, r.phi_err, r.tau, r.tau_err, r.scales[0], r.scale_errs[0], r.snr, r.red_chi2,
                     r.covariance_matrix[0, 1], r.nfeval, r.return_code], dtype=np.float64)


def three_variants(ref, prof, mprof, nu, P, sigma, x0, log10_tau):
    return np.array([one_channel_fit(ref, prof, mprof, nu, P, sigma, x0, log10_tau, "trust-ncg"),
                     one_channel_fit(ref, prof, mprof, nu, P, sigma, x0, log10_tau, "Newton-CG"),
                     one_channel_fit(ref, prof, mprof, nu, P, sigma, [x0[0] + 1e-3, x0[1]], log10_tau, "trust-ncg")])


def check(out, phi_inj, tau_inj_param, what):
    """The three conditions every stored case meets."""
    for v in out:
        assert int(v[10]) in (1, 2, 4), (what, v[10])
        dphi = (v[0] - phi_inj + 0.5) % 1.0 - 0.5
        assert abs(dphi) < 5.0 * v[1], (what, "phi", dphi, v[1])
        assert abs(v[2] - tau_inj_param) < 5.0 * v[3], (what, "tau", v[2], tau_inj_param, v[3])
        assert v[6] >= 30.0, (what, "snr", v[6])
    for v in out[1:]:
        assert abs((v[0] - out[0][0] + 0.5) % 1.0 - 0.5) < 1e-4 * out[0][1], (what, "variants phi")
        assert abs(v[2] - out[0][2]) < 1e-4 * out[0][3], (what, "variants tau", abs(v[2] - out[0][2]) / out[0][3])


def reference_start(prof, mprof, sigma, guess_tau, log10_tau, nbin):
    """(phi, tau) the reference starts from: the grid phase at the guessed tau; a linear tau of 0 -> 1 / nbin."""
    X, p, Sd = nr.spectra(prof, mprof, sigma)
    phi0 = nr.seed_phase(X, p, 10.0 ** guess_tau if log10_tau else guess_tau)
    return [phi0, 1.0 / nbin if (not log10_tau and guess_tau == 0.0) else guess_tau]


def objective_points(ref, prof, mprof, nu, P, sigma, x0, log10_tau):
    nbin = len(prof)
    dFT, mFT = np.fft.rfft(prof[None], axis=-1), np.fft.rfft(mprof[None], axis=-1)
    dFT[:, 0] *= ref.F0_fact
    mFT[:, 0] *= ref.F0_fact
    freqs = np.array([nu])
    args = (dFT, mFT, np.array([sigma]) * np.sqrt(nbin / 2.0), P, freqs, nu, nu, nu,
            np.array([1, 0, 0, 1, 0], dtype=bool), log10_tau)
    dt = (0.03, -0.05) if log10_tau else (4e-4, -7e-4)
    pts = np.array([x0, [x0[0] + 1.3e-3, x0[1] + dt[0]], [x0[0] - 4.0e-4, x0[1] + dt[1]]])
    full = [[q[0], 0.0, 0.0, q[1], 0.0] for q in pts]
    f = np.array([ref.fit_portrait_full_function(q, *args) for q in full])
    g = np.array([ref.fit_portrait_full_function_deriv(q, *args)[[0, 3]] for q in full])
    h = np.array([ref.fit_portrait_full_function_2deriv(q, *args)[np.ix_([0, 3], [0, 3])] for q in full])
    return pts, f, g, h


def fit_level(ref):
    rng = np.random.default_rng(mg.SEED + 77)
    cases = []
    # (tau [rot], channel frequency [MHz], guess: a factor on the truth, or "zero")
    draws = [(0.004, 1200.0, "zero"), (0.01, 1400.0, 1.5), (0.02, 1600.0, 0.7), (0.03, 1800.0, 1.4)]
    for nbin in (256, 100, 1024):
        for log10_tau in (True, False):
            for tau, nu, gfac in draws:
                # (1024 bins: from tau = 1 / 1024 the reference itself ends in another valley, or at a point without a
                # covariance -- the grid phase is ~100 sigma off there.  Those two cases start near the truth.)
                if gfac == "zero" and nbin == 1024:
                    gfac = 1.5
                cases.append((nbin, log10_tau, tau, nu, gfac))
    rec = dict(nbin=[], log10_tau=[], tau_inj=[], phi_inj=[], nu=[], sigma=[], guess=[], ref_start=[], prof=[],
               mprof=[], out=[], pts=[], f=[], g=[], h=[])
    for nbin, log10_tau, tau, nu, gfac in cases:
        mprof = unscattered_model(ref, np.array([nu]), nbin)[0]
        # (1024 bins: at sigma = 0.02 the S/N is 2400 and the reference's exits scatter by more than 1e-4 of the
        # error bars that go with it)
        amp, sigma = 0.7, (0.1 if nbin == 1024 else 0.02)
        phi_inj = rng.uniform(-0.5, 0.5)
        k = np.arange(nbin // 2 + 1)
        prof = np.fft.irfft(amp * np.fft.rfft(mprof) * ref.scattering_portrait_FT(np.array([tau]), nbin)[0] *
                            np.exp(-2.0j * np.pi * k * phi_inj), nbin) + rng.normal(0.0, sigma, nbin)
        if gfac == "zero":
            guess_tau = np.log10(1.0 / nbin) if log10_tau else 0.0
        else:
            guess_tau = np.log10(gfac * tau) if log10_tau else gfac * tau
        x0 = reference_start(prof, mprof, sigma, guess_tau, log10_tau, nbin)
        out = three_variants(ref, prof, mprof, nu, P_EXAMPLE, sigma, x0, log10_tau)
        what = (nbin, log10_tau, tau, gfac)
        check(out, phi_inj, np.log10(tau) if log10_tau else tau, what)
        pts, f, g, h = objective_points(ref, prof, mprof, nu, P_EXAMPLE, sigma, x0, log10_tau)
        for key, val in dict(nbin=nbin, log10_tau=log10_tau, tau_inj=tau, phi_inj=phi_inj, nu=nu, sigma=sigma,
                             guess=guess_tau, ref_start=x0, prof=prof, mprof=mprof, out=out, pts=pts, f=f, g=g,
                             h=h).items():
            rec[key].append(val)
        print(what, "nfev", out[:, 9], "rc", out[:, 10], "dphi/sig %.1e" %
              (np.abs(out[1:, 0] - out[0, 0]).max() / out[0, 1]))
    arrays = {k: np.asarray(v) for k, v in rec.items() if k not in ("prof", "mprof")}
    for nbin in (256, 100, 1024):           # ragged rows: one array per row length
        sel = [i for i, c in enumerate(cases) if c[0] == nbin]
        arrays["prof_%d" % nbin] = np.array([rec["prof"][i] for i in sel])
        arrays["mprof_%d" % nbin] = np.array([rec["mprof"][i] for i in sel])
    mg.save("nbscat_fits", variants=np.array(VARIANTS), fields=np.array(FIELDS), P=P_EXAMPLE, **arrays)


def caller_level(ref, log10_tau, name):
    scat_guess = (45e-6, 1500.0, -4.0)
    data, arrays, scal = mgt.synth_archive(ref, seed=61, nsub=3, C=8, B=256, tau_us=30.0, sigma=0.05)
    nsub, nchan, nbin = 3, 8, 256
    out = {k: np.zeros((nsub, nchan)) for k in ("phis", "phi_errs", "taus", "tau_errs", "scales", "scale_errs",
                                                "channel_snrs", "red_chi2s", "phi_tau_cov", "TOA_fracs", "TOA_errs")}
    out["TOA_days"] = np.zeros((nsub, nchan), dtype=np.int64)
    out["nfevals"] = np.zeros((nsub, nchan), dtype=np.int64)
    out["rcs"] = np.zeros((nsub, nchan), dtype=np.int64)
    spread = []
    first_flags = None
    for isub in data.ok_isubs:
        P = data.Ps[isub]
        model = unscattered_model(ref, data.freqs[isub], nbin)
        for ichan in data.ok_ichans[isub]:
            nu = data.freqs[isub, ichan]
            prof, mprof, sigma = data.subints[isub, 0, ichan], model[ichan], data.noise_stds[isub, 0, ichan]
            guess = nr.tau_guesses(scat_guess, None, None, None, -4.0, [nu], P, nbin, log10_tau)[0]
            x0 = reference_start(prof, mprof, sigma, guess, log10_tau, nbin)
            v3 = three_variants(ref, prof, mprof, nu, P, sigma, x0, log10_tau)
            tau_inj = 30e-6 / P * (nu / 1500.0) ** -4.0
            check(v3, arrays["inj"][isub][0] + mg_phase_at(ref, arrays["inj"][isub], nu, P),
                  np.log10(tau_inj) if log10_tau else tau_inj, (name, isub, ichan))
            spread.append(v3)
            v = v3[0]
            for key, col in (("phis", 0), ("phi_errs", 1), ("taus", 2), ("tau_errs", 3), ("scales", 4),
                             ("scale_errs", 5), ("channel_snrs", 6), ("red_chi2s", 7), ("phi_tau_cov", 8),
                             ("nfevals", 9), ("rcs", 10)):
                out[key][isub, ichan] = v[col]
            toa = data.epochs[isub] + mgt.FakeMJD(0, (v[0] * P + data.backend_delay) / (3600 * 24.))
            out["TOA_days"][isub, ichan], out["TOA_fracs"][isub, ichan] = toa.d, toa.f
            out["TOA_errs"][isub, ichan] = v[1] * P * 1e6
            if first_flags is None:
                df = data.doppler_factors[isub]
                if log10_tau:
                    first_flags = {'scat_time': 10 ** v[2] * P / df * 1e6, 'log10_scat_time': v[2] + np.log10(P / df),
                                   'log10_scat_time_err': v[3]}
                else:
                    first_flags = {'scat_time': v[2] * P / df * 1e6, 'scat_time_err': v[3] * P / df * 1e6}
                first_flags['phi_tau_cov'] = v[8]
    names = sorted(list(first_flags) + ['be', 'fe', 'f', 'nbin', 'bw', 'subint', 'chan', 'tobs', 'tmplt', 'snr', 'gof'])
    mg.save(name, **arrays, **{"scal_" + k: np.asarray(v) for k, v in scal.items()},
            **{"out_" + k: v for k, v in out.items()}, out_variants=np.array(spread),
            out_ok_isubs=np.asarray(data.ok_isubs), out_toa0_flag_names=np.array(names),
            out_toa0_scat_names=np.array(sorted(first_flags)),
            out_toa0_scat_values=np.array([first_flags[k] for k in sorted(first_flags)]),
            kw_scat_guess=np.array(scat_guess), kw_log10_tau=log10_tau)


def mg_phase_at(ref, inj, nu, P):
    """The dispersive part of a channel's injected delay [rot] (synth_archive rotates by -(phi, DM, GM) about
    infinite frequency): phi_n = phi + Dconst DM nu^-2 / P + Dconst^2 GM nu^-4 / P."""
    return ref.Dconst * inj[1] * nu ** -2 / P + ref.Dconst ** 2 * inj[2] * nu ** -4 / P


def main():
    ref, tmp = mg.import_reference()
    fit_level(ref)
    caller_level(ref, True, "nbscat_gettoas_log10")
    caller_level(ref, False, "nbscat_gettoas_lin")
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
