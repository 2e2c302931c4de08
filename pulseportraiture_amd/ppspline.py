"""ppspline: PCA + B-spline (.spl) templates made on the GPU.

`DataPortrait.make_spline_model` and `write_model` reproduce the reference's
(ppspline.py:34-232 with pplib.pca :1497-1534 and find_significant_eigvec
:1555-1619) for smooth=False; `make_smooth_spline_model` is its smooth=True, the
wavelet smoothing of pplib.smart_smooth on the device.  The passes over the nchan x nbin portrait --
weighted mean profile, centring, the covariance (or its dual, whichever is smaller),
the eigenvectors' statistics, projection, reconstruction and the model portraits --
run in HIP kernels through pulseportraiture_amd.engine.  Two third-party calls stay
on the host, as in the reference: numpy.linalg.eigh of the small symmetric matrix and
scipy.interpolate.splprep (FITPACK) on nchan points in at most ten dimensions.

One deliberate difference: `eigvec` is nbin x 10 -- the columns
find_significant_eigvec examines -- and `eigval` is the spectrum of the small
problem; the reference keeps all nbin columns, of which nothing past the tenth is
ever read.
"""
import pickle

import numpy as np
import scipy.interpolate as si

from . import pplib
from .archive import noise_kwargs
from .engine import default_engine

CHECK_MAX = 10      # find_significant_eigvec's check_max as make_spline_model calls it


def significant_eigvec(stats, nbin, check_max=CHECK_MAX, return_max=10, snr_cutoff=150.0,
                       check_crossings=True):
    """The decisions of find_significant_eigvec (pplib.py:1584-1615) for unsmoothed
    vectors, from the statistics Engine.pca_basis returns: stats[ivec] = (sum_{k>=1}
    |rfft(ev)_k|^2, get_noise(ev), max |ev|, count_crossings(|ev|, 0.1 max |ev|)).
    Returns (ieig, ev_snrs).

    The reference's check_acorr branch is not built: it sits in `elif ... and add_eigvec`
    with add_eigvec still False (pplib.py:1598), so it can never execute.  Without
    smoothing every noise eigenvector of a long profile passes the S/N cut and only the
    crossings test removes some of them; that is the reference's behaviour and is kept."""
    stats = np.asarray(stats, dtype=np.float64)
    ieig, snrs = [], []
    for ivec in range(min(max(check_max, return_max), len(stats))):
        add_eigvec = False
        ev_noise = stats[ivec, 1] * np.sqrt(nbin / 2.0)
        ev_snr = stats[ivec, 0] / ev_noise
        snrs.append(ev_snr)
        if ev_snr >= snr_cutoff:
            if check_crossings and ev_snr < 3 * snr_cutoff:
                if stats[ivec, 3] < int(0.02 * nbin):
                    add_eigvec = True
            else:
                add_eigvec = True
        if add_eigvec:
            ieig.append(ivec)
        if ivec + 1 == check_max:
            break
        if len(ieig) == return_max:
            break
    return np.array(ieig, dtype=int), np.array(snrs)


def fit_spline_curve(proj_port, pca_weights, freqs, bw, SNRs, noise_stds, k=3, sfac=1.0,
                     max_nbreak=None, quiet=False):
    """The B-spline curve through the projected profiles, parameterised by frequency
    (ppspline.py:135-155): si.splprep with the reference's arguments, the band flipped
    when bw < 0, and the refit under max_nbreak.  Returns (tck, u, fp, ier, msg)."""
    freqs = np.asarray(freqs, dtype=np.float64)
    nu_lo, nu_hi = freqs.min(), freqs.max()
    s = sfac * len(proj_port) * np.sum((SNRs * noise_stds) ** 2) / sum(SNRs) ** 2
    flip = -1 if bw < 0 else 1          # u in si.splprep has to be increasing
    (tck, u), fp, ier, msg = si.splprep(proj_port[::flip].T, w=pca_weights[::flip], u=freqs[::flip],
                                        ub=nu_lo, ue=nu_hi, k=k, task=0, s=s, t=None, full_output=1,
                                        nest=None, per=0, quiet=int(quiet))
    if max_nbreak is not None and len(np.unique(tck[0])) > max_nbreak:
        if max_nbreak < 2:
            print("max_nbreak not >= 2; setting max_nbreak = 2...")
            max_nbreak = 2
        if max_nbreak == 2:
            s = np.inf
        (tck, u), fp, ier, msg = si.splprep(proj_port[::flip].T, w=pca_weights[::flip], u=freqs[::flip],
                                            ub=nu_lo, ue=nu_hi, k=k, task=0, s=s, t=None, full_output=1,
                                            nest=max_nbreak + (k * 2), per=0, quiet=int(quiet))
    return tck, u, fp, ier, msg


class DataPortrait(pplib.DataPortrait):
    """The data a spline model is made from (built from arrays, like the parent), with
    the reference's methods for modelling profile evolution with a B-spline curve."""

    def normalize_portrait(self, method="rms", noise_method=None):
        """Normalize each channel's profile (pplib.py:357-382), with the reference's side
        effects: port, portx, norm_values, noise_stds[0,0], noise_stdsxs, flux_prof,
        flux_profx and the unnorm_* copies.  Norms and the noise of the normalised rows are
        measured on the device (Engine.channel_noise), with the estimator noise_method ('PS' or
        'fit'; None: archive's scope, else 'PS')."""
        kw = noise_kwargs(noise_method)
        if method not in ("mean", "max", "prof", "rms", "abs"):
            print("Unknown method for normalize_portrait(...), '%s'." % method)
            return
        eng = default_engine()
        weights = weightsx = None
        if method == "prof":
            weights = np.asarray(self.weights)[0]
            weightsx = np.asarray(self.weights)[np.asarray(self.weights) > 0]
        if self.noise_stds is None:
            self.noise_stds = np.zeros((self.nsub, self.npol, self.nchan))
            self.noise_stds[0, 0] = eng.channel_noise(self.port, **kw)[0]
            self.noise_stdsxs = self.noise_stds[0, 0, self.ok_ichans[0]]
        self.unnorm_noise_stds = np.copy(self.noise_stds)
        noise, norms = eng.channel_noise(self.port, norm=method,
                                         weights=None if weights is None else weights[None], **kw)
        self.port = self.port / norms[:, None]
        self.norm_values = norms
        self.noise_stds[0, 0] = noise
        self.flux_prof = self.port.mean(axis=1)
        self.unnorm_noise_stdsxs = np.copy(self.noise_stdsxs)
        noisex, normsx = eng.channel_noise(self.portx, norm=method,
                                           weights=None if weightsx is None else weightsx[None], **kw)
        self.portx = self.portx / normsx[:, None]
        self.noise_stdsxs = noisex
        self.flux_profx = self.portx.mean(axis=1)

    def unnormalize_portrait(self):
        """Undo normalize_portrait (pplib.py:384-398)."""
        if hasattr(self, 'unnorm_noise_stds'):
            self.port = (self.norm_values * self.port.transpose()).transpose()
            self.noise_stds = np.copy(self.unnorm_noise_stds)
            del self.unnorm_noise_stds
            self.flux_prof = self.port.mean(axis=1)
            self.portx = (self.norm_values[self.ok_ichans[0]] * self.portx.transpose()).transpose()
            self.noise_stdsxs = np.copy(self.unnorm_noise_stdsxs)
            del self.unnorm_noise_stdsxs
            self.flux_profx = self.portx.mean(axis=1)
            self.norm_values = np.ones(len(self.port))

    def make_spline_model(self, max_ncomp=10, smooth=True, snr_cutoff=150.0, rchi2_tol=0.1, k=3,
                          sfac=1.0, max_nbreak=None, model_name=None, quiet=False, **kwargs):
        """Make a model based on PCA and B-spline interpolation (ppspline.py:34-204).

        The arguments are the reference's.  smooth=True is refused here: callers pass smooth=False, or call
        make_smooth_spline_model for the smoothed model.  rchi2_tol only matters to the smoothing.  **kwargs:
        check_crossings (find_significant_eigvec's; default True) and engine (the Engine to run on; default
        the process-wide one)."""
        if smooth:
            raise NotImplementedError(
                "make_spline_model(smooth=True): the wavelet smoothing of the mean profile and the "
                "eigenvectors was pinned without PyWavelets and lives beside this method; call "
                "make_smooth_spline_model(...) (command: ppspline_smooth_run), or pass smooth=False")
        self._make_model(False, max_ncomp, snr_cutoff, rchi2_tol, k, sfac, max_nbreak, model_name, quiet, kwargs)

    def make_smooth_spline_model(self, max_ncomp=10, snr_cutoff=150.0, rchi2_tol=0.1, k=3, sfac=1.0,
                                 max_nbreak=None, model_name=None, quiet=False, **kwargs):
        """The reference's make_spline_model(smooth=True) (ppspline.py:34-204): the examined eigenvectors and the
        mean profile are wavelet-smoothed (pplib.smart_smooth, rchi2_tol) on the device; significance is decided
        from the smoothed vectors; projection, reconstruction and the model use the smoothed basis, and
        smooth_mean_prof / smooth_eigvec are set (write_model then writes those).  An odd nbin falls back to the
        unsmoothed model, as in the reference.  **kwargs: check_crossings, engine, and whatever else goes to
        smart_smooth (try_nlevels, threshtype)."""
        self._make_model(True, max_ncomp, snr_cutoff, rchi2_tol, k, sfac, max_nbreak, model_name, quiet, kwargs)

    def _make_model(self, smooth, max_ncomp, snr_cutoff, rchi2_tol, k, sfac, max_nbreak, model_name, quiet, kwargs):
        kwargs = dict(kwargs)
        eng = kwargs.pop("engine", None) or default_engine()
        check_crossings = kwargs.pop("check_crossings", True)
        port = self.portx
        if getattr(self, "noise_stdsxs", None) is None:
            self.noise_stdsxs = eng.channel_noise(port)[0]
        SNRs = np.asarray(self.SNRsxs, dtype=np.float64)
        pca_weights = SNRs / np.sum(SNRs)
        freqs = np.asarray(self.freqsxs[0], dtype=np.float64)
        nchanx, nbin = (int(v) for v in port.shape)
        if smooth and nbin % 2 != 0:
            print("nbin = %d is odd; cannot wavelet_smooth.\n" % nbin)
            smooth = False
        elif smooth and np.modf(np.log2(nbin))[0] != 0.0:
            print("nbin = %d is not a power of two; can only try wavelet_smooth to one level; recommend "
                  "resampling to a power-of-two number of phase bins.\n" % nbin)
        if not quiet:
            print("Performing principal component analysis on data with %d dimensions and %d "
                  "measurements..." % (nbin, nchanx))
        # pplib.pca: the covariance (or its dual) on the device, its eigen-solve on the host
        mean_prof, gram, fact = eng.pca_gram(port, pca_weights)
        eigval, vecs = np.linalg.eigh(gram)
        isort = np.argsort(eigval)[::-1]
        eigval, vecs = eigval[isort], vecs[:, isort]
        nvec = min(CHECK_MAX, len(eigval))
        eigvec, stats = eng.pca_basis(vecs[:, :nvec], eigval[:nvec])
        return_max = 10 if max_ncomp is None else min(max_ncomp, 10)
        basis, base_prof = eigvec, mean_prof        # what the projection and the model are built on
        if smooth:
            # find_significant_eigvec(return_smooth=True): the signal and the crossings of the SMOOTHED vectors,
            # the noise of the vectors themselves; then the mean profile (ppspline.py:91-102)
            raw = np.ascontiguousarray(eigvec.T[:nvec])
            sm, info = pplib.smart_smooth(raw, rchi2_tol=rchi2_tol, return_info=True, engine=eng, **kwargs)
            stats = pplib.smooth_stats(raw, sm, info)
        ieig, ev_snrs = significant_eigvec(stats, nbin, check_max=CHECK_MAX, return_max=return_max,
                                           snr_cutoff=snr_cutoff, check_crossings=check_crossings)
        if smooth:
            smooth_eigvec = np.zeros(eigvec.shape)
            if len(ieig):
                smooth_eigvec[:, ieig] = np.asarray(sm)[ieig].T
            smooth_mean_prof = np.asarray(pplib.smart_smooth(mean_prof, rchi2_tol=rchi2_tol, engine=eng))
            basis, base_prof = smooth_eigvec, smooth_mean_prof
        ncomp = len(ieig)
        nfreq = len(self.freqs[0])
        if ncomp == 0:          # the model is the constant average portrait
            proj_port = np.asarray(port)[:, :0]
            modelx = reconst_port = np.tile(base_prof, len(freqs)).reshape(len(freqs), nbin)
            model = np.tile(base_prof, nfreq).reshape(nfreq, nbin)
            (tck, u) = [np.array([]), np.array([]), 0], np.array([])
            fp, ier, msg = None, None, None
        else:
            if smooth:
                # (the resident basis is the unsmoothed one: nchan x nbin x ncomp products of the smoothed
                # columns, about the unsmoothed mean as reconstruct_portrait has it -- ppspline.py:119-124)
                delta_port = np.asarray(port, dtype=np.float64) - mean_prof
                proj_port = np.dot(delta_port, smooth_eigvec[:, ieig])
                reconst_port = np.dot(proj_port, smooth_eigvec[:, ieig].T) + mean_prof
            else:
                proj_port, reconst_port = eng.pca_project(ieig)
            tck, u, fp, ier, msg = fit_spline_curve(proj_port, pca_weights, freqs, self.bw, SNRs,
                                                    np.asarray(self.noise_stdsxs, dtype=np.float64),
                                                    k=k, sfac=sfac, max_nbreak=max_nbreak, quiet=quiet)
            if ier > 1:
                print("Something went wrong in si.splprep for %s:\n%s" % (self.source, msg))
            modelx = eng.spline_portrait(base_prof, basis[:, ieig], tck, freqs)
            model = eng.spline_portrait(base_prof, basis[:, ieig], tck, self.freqs[0])
        self.ieig = ieig
        self.ncomp = ncomp
        self.eigvec = eigvec
        self.eigval = eigval
        self.eigvec_stats = stats
        self.ev_snrs = ev_snrs
        self.mean_prof = mean_prof
        for name in ("smooth_mean_prof", "smooth_eigvec"):      # (a model made without smoothing carries neither)
            if hasattr(self, name):
                delattr(self, name)
        if smooth:
            self.smooth_mean_prof = smooth_mean_prof
            self.smooth_eigvec = smooth_eigvec
        self.proj_port = proj_port
        self.reconst_port = reconst_port
        self.tck, self.u, self.fp, self.ier, self.msg = tck, u, fp, ier, msg
        self.model_name = self.datafile + '.spl' if model_name is None else model_name
        self.model = model
        self.modelx = modelx
        self.model_masked = self.model * self.masks[0, 0]
        if not quiet:
            if proj_port.sum():
                print("B-spline interpolation model %s uses %d basis profile components and %d "
                      "breakpoints (%d B-splines with k=%d)." %
                      (self.model_name, ncomp, len(np.unique(self.tck[0])),
                       len(self.tck[0]) - self.tck[2] - 1, self.tck[2]))
            else:
                print("B-spline interpolation model %s uses 0 basis profile components; it returns "
                      "the average profile." % self.model_name)

    def write_model(self, outfile, quiet=False):
        """Write the model to outfile: the pickle (protocol 2) of [model_name, source,
        datafile, mean_prof, eigvec[:, ieig], tck] (ppspline.py:206-232), what
        splmodel.read_spline_model and the reference read back; the smoothed mean profile and
        eigenvectors where make_smooth_spline_model made them."""
        smooth = hasattr(self, "smooth_eigvec")
        basis, mean_prof = (self.smooth_eigvec, self.smooth_mean_prof) if smooth else (self.eigvec, self.mean_prof)
        eigvec = basis[:, self.ieig] if len(self.ieig) else basis[:, []]
        with open(outfile, "wb") as of:
            pickle.dump([self.model_name, self.source, self.datafile, mean_prof, eigvec, self.tck],
                        of, protocol=2)
        if not quiet:
            print("Wrote modelfile %s." % outfile)
