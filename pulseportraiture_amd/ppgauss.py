"""ppgauss: Gaussian-component (.gmodel) templates fitted on the GPU.

`DataPortrait.make_gaussian_model`, `fit_profile`, `model_iteration`, `check_convergence`,
`write_model` and `write_errfile` reproduce the reference's (ppgauss.py:28-372): the initial
profile fit, the flag logic, the portrait fit, and the loop that measures the phase and DM left
between data and model, rotates the data by them and fits again.  A DataPortrait of several
bands (pplib.DataPortrait's metafile branch) is fitted jointly, the reference's "njoin"
branches: every band's phase offset and Delta-DM are parameters of the same fit, the data are
not rotated between iterations, and the join parameters are written beside the model.  Every pass
over the nchan x nbin portrait runs in HIP kernels through pulseportraiture_amd.engine: the
residual rows of all forward-difference parameter sets in one launch and their reduction to
the normal equations (pplib.fit_gaussian_portrait), the model portraits, the rotations and
the (phase, DM) fit of check_convergence.  The Levenberg-Marquardt driver itself -- a linear
solve in at most 100 unknowns per iteration -- is the host's (gaussfit.py).

Not available: the interactive component selector and every plot.  Components are either fitted automatically
(auto_gauss, the reference's own branch) or handed in (`init_params`, what the reference's
window would have returned before its profile fit).
"""
import time

import numpy as np

from . import gmodel
from .engine import default_engine
from .pplib import (default_model, fit_gaussian_portrait, fit_gaussian_profile, fit_phase_shift, fit_portrait,
                    gaussian_profile, get_noise, guess_fit_freq, scattering_alpha)
from .ppspline import DataPortrait as _NormalizingPortrait


def portrait_start(init_params, fixloc=False, fixwid=False, fixamp=False, fixscat=True, fiducial_gaussian=False):
    """(init_model_params, fit_flags) of a portrait fit from the profile fit's [DC, tau, (loc, wid,
    amp) x ngauss] (ppgauss.py:140-159): all slopes and spectral indices start at 0.0; fixscat,
    fixloc, fixwid and fixamp fix tau and the evolution of the locations, widths and amplitudes;
    fiducial_gaussian lets every location drift except the first component's."""
    init_params = np.asarray(init_params, dtype=np.float64)
    ngauss = (len(init_params) - 2) // 3
    comps = np.zeros([ngauss, 6])
    comps[:, 0::2] = np.reshape(init_params[2:], (ngauss, 3))
    init_model_params = np.array([init_params[0]] + [init_params[1]] + list(np.ravel(comps)))
    fit_flags = np.ones(len(init_model_params))
    fit_flags[1] *= not fixscat
    fit_flags[3::6] *= not fixloc
    fit_flags[5::6] *= not fixwid
    fit_flags[7::6] *= not fixamp
    if fiducial_gaussian:
        ifgauss = 0
        fit_flags[3::6] = 1
        fit_flags[3::6][ifgauss] = 0
    return init_model_params, fit_flags


class DataPortrait(_NormalizingPortrait):
    """The data a Gaussian-component model is fit to (built from arrays, like the parent; the
    parent's normalize_portrait is the reference's), with the reference's methods for modelling
    profile evolution with Gaussian components."""

    def _engine(self):
        return getattr(self, "engine", None) or default_engine()

    def fit_profile(self, profile, tau=0.0, fixscat=True, auto_gauss=0.0, profile_fit_flags=None, show=True,
                    init_params=None):
        """Fit Gaussian components to a profile (ppgauss.py:28-53) without a window.

        auto_gauss != 0.0: GaussianSelector's automatic branch (ppgauss.py:442-459) -- one
        component of that width [rot] and the profile's height, placed by fit_phase_shift, then
        fitted.  Otherwise init_params = [loc, wid, amp, ...] are the components a user would
        have drawn, and the profile fit refines them.  tau [bin] is the scattering timescale
        added to the Gaussians, and the initial value if fixscat=False."""
        profile = np.asarray(profile, dtype=np.float64)
        nbin = len(profile)
        errs = get_noise(profile)
        fit_scattering = not fixscat
        tauguess = tau
        if fit_scattering and tauguess == 0.0:
            tauguess = 0.1              # seems to break otherwise (ppgauss.py:415-416)
        start = [sorted(profile)[nbin // 10 + 1], tauguess]
        if auto_gauss:
            amp = profile.max()
            first_gauss = amp * gaussian_profile(nbin, 0.5, auto_gauss)
            loc = 0.5 + fit_phase_shift(profile, first_gauss, errs).phase
            start += [loc, auto_gauss, amp]
        else:
            comps = [] if init_params is None else list(np.ravel(init_params))
            if not comps or len(comps) % 3:
                raise ValueError("fit_profile: without auto_gauss, init_params must hold (loc, wid, amp) "
                                 "of every component")
            start += comps
        fgp = fit_gaussian_profile(profile, start, np.zeros(nbin) + errs, profile_fit_flags, fit_scattering,
                                   quiet=True, engine=self._engine())
        self.profile_start = np.array(start)
        self.init_params = fgp.fitted_params
        self.init_param_errs = fgp.fit_errs
        self.profile_fit = fgp
        self.ngauss = (len(self.init_params) - 2) // 3

    def make_gaussian_model(self, modelfile=None, ref_prof=(None, None), tau=0.0, fixloc=False, fixwid=False,
                            fixamp=False, fixscat=True, fixalpha=True, scattering_index=scattering_alpha,
                            model_code=default_model, niter=0, fiducial_gaussian=False, auto_gauss=0.0,
                            writemodel=False, outfile=None, writeerrfile=False, errfile=None, model_name=None,
                            residplot=None, quiet=False, init_gauss=None):
        """Fit a Gaussian-component model with independently evolving components
        (ppgauss.py:55-238; the arguments are the reference's).

        modelfile: a .gmodel whose parameters and flags start a new fit.  Without one the
        components come from a profile fit of the channels within ref_prof = (reference
        frequency, bandwidth) [MHz]: automatically (auto_gauss), or from init_gauss = [(loc,
        wid, amp), ...].  tau is a scattering timescale [bin]; niter the number of
        rotate-and-refit iterations after the initial fit.  residplot is not available."""
        if residplot:
            raise NotImplementedError("make_gaussian_model(residplot=...): plots are not available")
        if modelfile:
            if outfile is None:
                outfile = modelfile
            if errfile is None:
                errfile = outfile + "_errs"
            mdl = gmodel.read_gmodel(modelfile)
            self.model_name, self.model_code, self.nu_ref, self.ngauss = mdl["name"], mdl["code"], mdl["nu_ref"], mdl["ngauss"]
            self.init_model_params = np.array(mdl["params"], dtype=np.float64)
            self.fit_flags = np.array(mdl["fit_flags"], dtype=np.float64)
            self.scattering_index, self.fitalpha = mdl["alpha"], mdl["fit_alpha"]
            self.fixalpha = not self.fitalpha
            if model_name is not None:
                self.model_name = model_name
            self.init_model_params[1] *= self.nbin / self.Ps[0]         # [sec] -> [bin]
        else:
            self.model_code = model_code
            self.scattering_index = scattering_index
            self.fixalpha = fixalpha
            self.fitalpha = int(not self.fixalpha)
            if errfile is None and outfile is not None:
                errfile = outfile + "_errs"
            self.model_name = self.source if model_name is None else model_name
            # Fit the profile
            if not len(self.init_params):
                self.nu_ref, self.bw_ref = ref_prof
                if self.nu_ref is None:
                    self.nu_ref = self.nu0
                if self.bw_ref is None:
                    self.bw_ref = abs(self.bw)
                okinds = np.compress(np.less(self.nu_ref - (self.bw_ref / 2), self.freqs[0]) *
                                     np.greater(self.nu_ref + (self.bw_ref / 2), self.freqs[0]) *
                                     self.masks[0, 0].mean(axis=1), np.arange(self.nchan))
                if not len(okinds):
                    raise ValueError("no good channel within %g MHz of %g MHz" % (self.bw_ref / 2, self.nu_ref))
                profile = np.take(self.port, okinds, axis=0).mean(axis=0)       # an unweighted profile
                self.fit_profile(profile, tau=tau, fixscat=fixscat, auto_gauss=auto_gauss, profile_fit_flags=None,
                                 show=False, init_params=init_gauss)
            self.ngauss = (len(self.init_params) - 2) // 3
            self.init_model_params, self.fit_flags = portrait_start(self.init_params, fixloc, fixwid, fixamp, fixscat,
                                                                    fiducial_gaussian)
        # The noise...
        self.portx_noise = np.outer(self.noise_stdsxs, np.ones(self.nbin))
        self.nu_fit = guess_fit_freq(self.freqsxs[0], self.SNRsxs)
        # Here's the loop
        if niter < 0:
            niter = 0
        self.niter = niter
        self.itern = niter
        self.model_params = np.copy(self.init_model_params)
        self.total_time = 0.0
        self.start = time.time()
        print("Fitting Gaussian model portrait...")
        iterator = self.model_iteration(quiet)
        next(iterator)
        self.cnvrgnc = self.check_convergence(efac=1.0, quiet=quiet)
        self.convergence_history = [(self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2, self.cnvrgnc)]
        if writemodel:
            self.write_model(outfile=outfile, quiet=quiet)
        if writeerrfile:
            self.write_errfile(errfile=errfile, quiet=quiet)
        while self.niter and not self.cnvrgnc:
            if not quiet:
                print("\n...iteration %d..." % (self.itern - self.niter + 1))
            eng = self._engine()
            # (a joined fit carries the bands' offsets as parameters: its data stay where they are)
            for name, fr in (("port", self.freqs[0]), ("portx", self.freqsxs[0])) if not self.njoin else ():
                rot = eng.rotate_portraits(np.asarray(getattr(self, name))[None], fr, self.Ps[0], phi=self.phi, DM=self.DM,
                                           nu_DM=self.nu_fit)
                setattr(self, name, rot[0])
            if not quiet:
                print("Fitting Gaussian model portrait...")
            next(iterator)
            self.niter -= 1
            self.cnvrgnc = self.check_convergence(efac=1.0, quiet=quiet)
            self.convergence_history.append((self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2, self.cnvrgnc))
            # For safety, write model after each iteration
            if writemodel:
                self.write_model(outfile=outfile, quiet=quiet)
            if writeerrfile:
                self.write_errfile(errfile=errfile, quiet=quiet)
        if self.njoin:
            # data and model as they are without the bands' offsets (ppgauss.py:206-224)
            back = -np.asarray(self.join_params, dtype=np.float64)
            self.port = self._rotate_bands(self.port, self.join_ichans, self.freqs[0], back, self.nu_ref)
            self.portx = self._rotate_bands(self.portx, self.join_ichanxs, self.freqsxs[0], back, self.nu_ref)
            self.model = self._rotate_bands(self.model, self.join_ichans, self.freqs[0], back, self.nu_ref)
            self.model_masked = self.model * self.masks[0, 0]
            self.modelx = np.compress(self.masks[0, 0].mean(axis=1), self.model, axis=0)
        if not quiet:
            print("")
            print("Residuals mean: %.2e" % (self.portx - self.modelx).mean())
            print("Residuals std:  %.2e" % (self.portx - self.modelx).std())
            print("Data std:       %.2e\n" % np.median(self.noise_stdsxs))
            print("Total fit time: %.2f min" % (self.total_time / 60.0))
            print("Total time:     %.2f min\n" % ((time.time() - self.start) / 60.0))

    def model_iteration(self, quiet=False):
        """Iterate over a model fit (ppgauss.py:240-276)."""
        while True:
            start = time.time()
            eng = self._engine()
            fgp = fit_gaussian_portrait(self.model_code, self.portx, self.model_params, self.scattering_index,
                                        self.portx_noise, self.fit_flags, not self.fixalpha, self.phases,
                                        self.freqsxs[0], self.nu_ref, self.all_join_params, self.Ps[0], quiet=quiet,
                                        engine=eng)
            self.fitted_params, self.fit_errs, self.chi2, self.dof = fgp.fitted_params, fgp.fit_errs, fgp.chi2, fgp.dof
            self.scattering_index, self.scattering_index_err = fgp.scattering_index, fgp.scattering_index_err
            self.fgp = fgp
            if self.njoin:
                self.model_params = self.fitted_params[:-self.njoin * 2]
                self.model_param_errs = self.fit_errs[:-self.njoin * 2]
                self.join_params = self.fitted_params[-self.njoin * 2:]
                self.join_param_errs = self.fit_errs[-self.njoin * 2:]
                self.all_join_params[1] = self.join_params
                self.write_join_parameters()
            else:
                self.model_params = self.fitted_params[:]
                self.model_param_errs = self.fit_errs[:]
            mdl = dict(params=np.asarray(self.model_params, dtype=np.float64), code=self.model_code, nu_ref=self.nu_ref,
                       alpha=self.scattering_index, ngauss=self.ngauss)
            # (tau is in bins: a period of nbin makes it rotations)
            self.model = eng.gaussian_portrait(mdl, self.freqs[0], self.nbin, P=float(self.nbin))
            if self.njoin:
                # every band of the model rotated by its offsets (gen_gaussian_portrait's join_ichans, pplib.py:923-929)
                self.model = self._rotate_bands(self.model, self.join_ichans, self.freqs[0], self.join_params, self.nu_ref)
            self.model_masked = self.model * self.masks[0, 0]
            self.modelx = np.compress(self.masks[0, 0].mean(axis=1), self.model, axis=0)
            self.duration = time.time() - start
            self.total_time += self.duration
            yield

    def check_convergence(self, efac=1.0, quiet=False):
        """Check for convergence (ppgauss.py:278-334): whether the phase and DM in the data, as
        measured by the fitted model, are within the errors (times efac) of the measurements."""
        if self.njoin:
            # measured with the bands' offsets taken out of both
            back = -np.asarray(self.join_params, dtype=np.float64)
            portx = self._rotate_bands(self.portx, self.join_ichanxs, self.freqsxs[0], back, self.nu_ref)
            modelx = self._rotate_bands(self.modelx, self.join_ichanxs, self.freqsxs[0], back, self.nu_ref)
        else:
            portx, modelx = np.copy(self.portx), np.copy(self.modelx)
        # Currently, fit_phase_shift returns an unbounded phase
        phase_guess = fit_phase_shift(portx.mean(axis=0), modelx.mean(axis=0)).phase       # unweighted mean
        phase_guess %= 1
        if phase_guess >= 0.5:
            phase_guess -= 1.0
        DM_guess = 0.0
        fp = fit_portrait(portx, modelx, np.array([phase_guess, DM_guess]), self.Ps[0], self.freqsxs[0], self.nu_fit,
                          None, None, bounds=[(None, None), (None, None)], id=None, quiet=True)
        self.fp_results = fp
        self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2 = fp.phase, fp.phase_err, fp.DM, fp.DM_err, fp.red_chi2
        if not quiet:
            print("Iter %d:" % (self.itern - self.niter))
            print(" duration of %.2f min" % (self.duration / 60.))
            print(" phase offset of %.2e +/- %.2e [rot]" % (self.phi, self.phierr))
            print(" DM of %.6e +/- %.2e [cm**-3 pc]" % (self.DM, self.DMerr))
            print(" red. chi**2 of %.2f." % self.red_chi2)
        elif self.niter:
            print("Iter %d..." % (self.itern - self.niter + 1))
        if min(abs(self.phi), abs(1 - self.phi)) < abs(self.phierr) * efac:
            if abs(self.DM) < abs(self.DMerr) * efac:
                print("\nIteration converged.\n")
                return 1
        return 0

    def write_model(self, outfile=None, append=False, quiet=False):
        """Write the model parameters to file (ppgauss.py:336-354): locs of 1 or more are folded
        into [0, 1), the scattering timescale goes from bins to seconds."""
        if outfile is None:
            outfile = self.datafile + ".gmodel"
        model_params = np.copy(self.model_params)
        model_params[2::6] = np.where(model_params[2::6] >= 1.0, model_params[2::6] % 1, model_params[2::6])
        model_params[1] *= self.Ps[0] / self.nbin
        gmodel.write_gmodel(outfile, self.model_name, self.model_code, self.nu_ref, model_params, self.fit_flags,
                            self.scattering_index, self.fitalpha, append=append, quiet=quiet)

    def write_errfile(self, errfile=None, append=False, quiet=False):
        """Write the model parameter uncertainties to file (ppgauss.py:356-372)."""
        if errfile is None:
            errfile = self.datafile + ".gmodel_errs"
        model_param_errs = np.copy(self.model_param_errs)
        model_param_errs[1] *= self.Ps[0] / self.nbin
        gmodel.write_gmodel(errfile, self.model_name + "_errors", self.model_code, self.nu_ref, model_param_errs,
                            self.fit_flags, self.scattering_index_err, self.fitalpha, append=append, quiet=quiet)
