"""Command line of the fit residuals: `python -m pulseportraiture_amd.ppresid_run -d <datafiles> -m <model> [options]`
fits the archives as pptoas_run does (GetTOAs.get_TOAs), forms data minus fitted model of every fitted subint on the
device (GetTOAs.get_residuals) and writes one .npz archive per input: the input's fields with `subints` replaced by
the residuals.  --frame data (the default) keeps the rows where the data have them, so the output is an archive of the
same observation; --frame model stores the rows aligned with the template (dmc = 1), so that `ppscrunch_run -T` of it
is the mean residual in the template's frame: the profile evolution the template does not model."""
import argparse
import sys

import numpy as np

from . import archive
from .ppscrunch_run import output_name, write_archive

MODULE = "pulseportraiture_amd.ppresid_run"
FIT_KEYS = ("nu_refs", "DM0", "bary", "fit_DM", "fit_GM", "fit_scat", "log10_tau", "scat_guess", "fix_alpha", "method",
            "quiet", "seed")


def parser():
    ap = argparse.ArgumentParser(
        prog="python -m " + MODULE,
        description="Fit .npz archives with a wideband template and write the residuals, data minus fitted model, as "
                    ".npz archives (one GPU).")
    ap.add_argument("-d", "--datafiles", required=True, metavar="archive",
                    help="One .npz archive (the fields of a DataBunch) or a metafile listing archive filenames, one per line.")
    ap.add_argument("-m", "--modelfile", required=True, metavar="model",
                    help="Model file: a .gmodel (ppgauss) or a spline model (ppspline).")
    ap.add_argument("-e", "--ext", default="resid.npz", metavar="ext",
                    help="Output beside the input under this extension. [default=resid.npz]")
    ap.add_argument("--metafile", default=None, metavar="out.txt", help="Write the names of the output archives here.")
    ap.add_argument("--frame", choices=("data", "model"), default="data",
                    help="data: residual rows where the data have them, header unchanged; model: rows aligned with "
                         "the template, written as dedispersed (dmc = 1). [default=data]")
    ap.add_argument("--nu_ref", dest="nu_ref_DM", default=None, metavar="nu_ref",
                    help="Frequency [MHz] the fitted phases are referenced to; 'inf' for infinite frequency. "
                         "[default: zero-covariance frequency]")
    ap.add_argument("--DM", dest="DM0", default=None,
                    help="Nominal DM [cm**-3 pc] the DM offsets refer to. [default: each archive's DM]")
    ap.add_argument("--no_bary", dest="bary", action="store_false",
                    help="Do not Doppler-correct DMs, GMs, taus or nu_tau.")
    ap.add_argument("--fix_DM", dest="fit_DM", action="store_false", help="Do not fit for DM.")
    ap.add_argument("--fit_dt4", dest="fit_GM", action="store_true", help="Fit for delays that scale as nu**-4 (GM).")
    ap.add_argument("--fit_scat", action="store_true", help="Fit for scattering timescale and index.")
    ap.add_argument("--no_logscat", "--no_log10_tau", dest="log10_tau", action="store_false",
                    help="Fit the scattering timescale itself, not its log10.")
    ap.add_argument("--scat_guess", default=None, metavar="tau,freq,alpha",
                    help="Initial scattering timescale [s], its reference frequency [MHz] and index.")
    ap.add_argument("--fix_alpha", action="store_true", help="Fix the scattering index (with --fit_scat).")
    ap.add_argument("--seed", choices=("reference", "device"), default="reference",
                    help="Initial phase guess: the reference's (default) or the device's fast seed.")
    ap.add_argument("--psrchive", action="store_true", help="Not available: needs PSRCHIVE.")
    ap.add_argument("-T", "--tscrunch", action="store_true", help="Not available: needs PSRCHIVE.")
    ap.add_argument("--showplot", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--saveplot", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--quiet", action="store_true", help="Suppress output.")
    archive.add_noise_method_option(ap)
    return ap


def refusal(opts):
    """The message for an option this command cannot honour, or None."""
    if archive.noise_method_refusal(opts) is not None:
        return archive.noise_method_refusal(opts)
    if opts.psrchive:
        return "--psrchive needs PSRCHIVE, which this package does not use"
    if opts.tscrunch:
        return "-T/--tscrunch needs PSRCHIVE, which this package does not use: scrunch the archives with ppscrunch_run -T first"
    if opts.showplot or opts.saveplot:
        return "--showplot/--saveplot: plots are not available"
    return None


def get_toas_kwargs(opts):
    """get_TOAs keyword arguments of the parsed options: pptoas_run's mapping of the fit options."""
    from .pptoas_run import get_toas_kwargs as toas_kwargs
    ns = argparse.Namespace(nu_ref_tau=None, print_phase=False, print_flux=False, print_parangle=False, toa_flags="",
                            **vars(opts))
    kw = toas_kwargs(ns)
    return {k: kw[k] for k in FIT_KEYS}


def summary(res, nbin):
    """(fitted subints, overall reduced chi^2, its degrees of freedom, largest |residual| / sigma, its (subint, channel,
    bin)) of a get_residuals bunch.  The overall figure is the channels' sum of squares over the channels' summed
    nbin - 2; channels of sigma 0 (noiseless data) have no chi^2 and are left out of both figures."""
    rc2 = np.asarray(res.channel_red_chi2, dtype=np.float64)
    ok = np.isfinite(rc2)
    dof = int(ok.sum()) * (nbin - 2)
    red = float(rc2[ok].sum() * (nbin - 2) / dof) if dof else float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.abs(np.asarray(res.resid, dtype=np.float64)) / np.asarray(res.noise_stds, dtype=np.float64)[..., None]
    z[~ok] = -1.0
    z[~np.isfinite(z)] = -1.0
    where = tuple(int(v) for v in np.unravel_index(int(np.argmax(z)), z.shape))
    worst = float(z[where]) if z[where] >= 0 else float("nan")
    return len(res.ok_isubs), red, dof, worst, where


def main(argv=None):
    opts = parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    msg = refusal(opts)
    if msg is not None:
        print("ppresid_run: " + msg, file=sys.stderr)
        return 2
    with archive.noise_method_scope(opts.noise_method):
        from .pptoas import GetTOAs
        bunches = []
        for datafile in archive.named_datafiles(opts.datafiles):
            try:
                data, name = archive.load_bunch(datafile)
            except archive.LOAD_ERRORS + (TypeError, KeyError) as err:
                if not opts.quiet:
                    print("Cannot load_data(%s).  Skipping it." % datafile)
                    print(err)
                continue
            if data.npol != 1:
                print("ppresid_run: %s has %d polarisations; the fit is of total intensity: scrunch it with "
                      "ppscrunch_run -p first" % (name, data.npol), file=sys.stderr)
                return 2
            bunches.append((data, name))
        if not bunches:
            return 1
        gt = GetTOAs([b[0] for b in bunches], opts.modelfile, quiet=opts.quiet)
        gt.get_TOAs(**get_toas_kwargs(opts))
        eng = gt._engine(False)
        written = []
        for idatafile in gt.ok_idatafiles:
            data, name = bunches[idatafile]
            res = gt.get_residuals(data, frame=opts.frame)
            resid = res.resid
            out = archive.DataBunch(**{k: v for k, v in data.items()})
            if opts.frame == "model":
                out.dmc = 1
            elif data.dmc:
                # the fit is of the dispersed rows (a dedispersed archive is put back first): the residual goes
                # back to the state the header states
                resid = eng.rotate_portraits(resid, data.freqs, data.Ps, DM=float(data.DM), nu_DM=float(data.nu0))
            out.subints = np.asarray(resid)[:, None].astype(np.asarray(data.subints).dtype, copy=False)
            written.append(write_archive(output_name(name, opts.ext), out))
            if not opts.quiet:
                nfit, red, dof, worst, where = summary(res, data.nbin)
                print("%s: %d fitted subint(s), reduced chi2 %.6f (dof %d), largest |residual|/sigma %.3f at "
                      "(subint %d, channel %d, bin %d)" % ((written[-1], nfit, red, dof, worst) + where))
        if opts.metafile is not None:
            with open(opts.metafile, "w") as f:
                f.write("".join(name + "\n" for name in written))
        return 0 if written else 1


if __name__ == "__main__":
    sys.exit(main())
