"""Command line of ppgauss: `python -m pulseportraiture_amd.ppgauss_run -d <datafile> [options]`,
the options of the reference's `ppgauss.py` (ppgauss.py:667-743).

The input is one aligned, averaged portrait: an .npz archive (the fields of a DataBunch) or a
metafile naming one.  Its Gaussian components start from a model file (-I), from one automatically
placed component (--autogauss wid), or from components given with --gauss loc,wid,amp (repeatable)
-- the scripted equivalent of drawing them in the reference's window; the profile fit then refines
them.  The model is fitted on the device (DataPortrait.make_gaussian_model) and written as a
.gmodel (default datafile.gmodel) with its error file, which pptoas_run, ppzap_run -m and the
reference read.

Several observations from different bands (the reference's -M metafile and -j joinfile) are the
business of `python -m pulseportraiture_amd.ppgauss_join_run`, which shares this module's options
and its fit; here they stay refused."""
import argparse
import sys

import numpy as np

from .archive import (add_noise_method_option, load_archive_file, named_datafiles, noise_method_refusal,
                      noise_method_scope)
from .pplib import default_model

MODULE = "pulseportraiture_amd.ppgauss_run"


JOIN_MODULE = "pulseportraiture_amd.ppgauss_join_run"


def parser(joined=False):
    """The options of ppgauss_run; joined=True: of ppgauss_join_run, where -M and -j are the input
    and -d is not."""
    ap = argparse.ArgumentParser(
        prog="python -m " + (JOIN_MODULE if joined else MODULE),
        description="Generate a Gaussian-component model pulse portrait (the reference's ppgauss.py command line)" +
                    (" from several bands at once, each with a phase offset and a Delta-DM of its own." if joined else "."))
    ap.add_argument("-d", "--datafile", default=None, metavar="archive",
                    help="Not used here: python -m %s fits one archive." % MODULE if joined else
                         "One .npz archive (the fields of a DataBunch) from which to generate the Gaussian model, or "
                         "a metafile naming one.")
    ap.add_argument("-M", "--metafile", default=None, metavar="metafile",
                    help="List of .npz archive filenames, one per band (for instance every band's ppalign_run average), "
                         "from which to generate one Gaussian model." if joined else
                         "Not available here: python -m %s fits several observations from different bands." % JOIN_MODULE)
    ap.add_argument("-I", "--improve", dest="modelfile", default=None, metavar="modelfile",
                    help="Improve/iterate on a model given input data.  The argument to -I is a ppgauss-format "
                         "modelfile.  Use -o and -e to avoid overwriting and --niter to specify a number of iterations.  "
                         "Everything else should be specified in the modelfile.")
    ap.add_argument("-o", "--outfile", default=None, metavar="outfile",
                    help="Name of output model file name. [default=archive.gmodel]")
    ap.add_argument("-e", "--errfile", default=None, metavar="errfile",
                    help="Name of parameter error file name. [default=outfile_errs]")
    ap.add_argument("-j", "--joinfile", default=None, metavar="joinfile",
                    help="File of join parameters to start the alignment of the metafile's archives from, as written by "
                         "an earlier run; the fitted ones are appended to it. [default=model_name.join]" if joined else
                         "Not available here: join parameters to align the files of a metafile (python -m %s)." % JOIN_MODULE)
    ap.add_argument("-m", "--model_name", default=None, metavar="model_name",
                    help="Name given to model. [default=the archive's source name]")
    ap.add_argument("--nu_ref", default=None, metavar="nu_ref",
                    help="Reference frequency [MHz] for the Gaussian model; the initial profile to fit will be centered "
                         "on this freq. [default=the archive's center frequency]")
    ap.add_argument("--bw", dest="bw_ref", default=None, metavar="bw",
                    help="Used with --nu_ref; amount of bandwidth [MHz] centered on nu_ref to average for the initial "
                         "profile fit. [default=Full bandwidth]")
    ap.add_argument("--tau", default=0.0, metavar="tau",
                    help="Scattering timescale [sec] at nu_ref, assuming alpha=-4.0.  Not used with -I. [default=0]")
    ap.add_argument("--fitloc", dest="fixloc", action="store_false", default=True,
                    help="Do not fix locations of Gaussians across frequency (cf. --fgauss).  Not used with -I.")
    ap.add_argument("--fixwid", action="store_true", default=False,
                    help="Fix widths of Gaussians across frequency.  Not used with -I.")
    ap.add_argument("--fixamp", action="store_true", default=False,
                    help="Fix amplitudes of Gaussians across frequency.  Not used with -I.")
    ap.add_argument("--fitscat", dest="fixscat", action="store_false", default=True,
                    help="Fit scattering timescale to tau w.r.t nu_ref.  Not used with -I.")
    ap.add_argument("--fitalpha", dest="fixalpha", action="store_false", default=True,
                    help="Fit power-law index for the scattering law.  Implies --fitscat.")
    ap.add_argument("--mcode", dest="model_code", default=default_model, metavar="###",
                    help="Three-digit string specifying the evolutionary functions for each Gaussian parameter "
                         "(loc,wid,amp): 0 = power law, 1 = linear.  Not used with -I. [default=%s]" % default_model)
    ap.add_argument("--niter", default=0, metavar="int",
                    help="Number of iterations to loop for generating better model; exits before niter iterations if "
                         "internal convergence criteria are met. [default=0]")
    ap.add_argument("--fgauss", action="store_true", default=False,
                    help="Sets fitloc=True except for the first Gaussian component fitted in the initial profile fit, "
                         "i.e. sets a 'fiducial Gaussian'.  Not used with -I.")
    ap.add_argument("--autogauss", dest="auto_gauss", default=0.0, metavar="wid",
                    help="Automatically fit one Gaussian to initial profile with initial width [rot] given as the "
                         "argument.  Not used with -I.")
    ap.add_argument("--gauss", dest="gauss", action="append", default=[], metavar="loc,wid,amp",
                    help="A Gaussian component of the initial profile fit: location [rot], FWHM [rot] and amplitude.  "
                         "Repeat for every component.  Takes the place of the reference's interactive window.  Not "
                         "used with -I.")
    ap.add_argument("--norm", dest="normalize", default=None, metavar="normalize",
                    help="Normalize each channel's profile by either mean, max, mean profile, off-pulse noise, or "
                         "sqrt{vector modulus} ('mean', 'max', 'prof', 'rms', 'abs').")
    ap.add_argument("--figure", default=False, metavar="figurename", help="Not available: no plotting.")
    ap.add_argument("--verbose", dest="quiet", action="store_false", default=True, help="More to stdout.")
    add_noise_method_option(ap)
    return ap


def parse_gauss(specs):
    """[(loc, wid, amp), ...] of the --gauss arguments."""
    out = []
    for spec in specs:
        try:
            vals = [float(v) for v in spec.split(",")]
        except ValueError:
            vals = []
        if len(vals) != 3:
            raise ValueError("--gauss takes loc,wid,amp (three numbers), got '%s'" % spec)
        out.append(tuple(vals))
    return out


def refusal(opts, datafiles=None):
    """The message for a request this command cannot honour, or None."""
    if opts.metafile is not None:
        return ("-M/--metafile: fits of several observations from different bands (BETA in the reference) are not "
                "available here; give one archive with -d, or the metafile to python -m " + JOIN_MODULE)
    if opts.joinfile is not None:
        return "-j/--joinfile: joined multi-band fits are not available here, but with python -m " + JOIN_MODULE
    if opts.datafile is None:
        return "no archive: give one with -d"
    msg = fit_refusal(opts)
    if msg is not None:
        return msg
    if datafiles is not None and len(datafiles) != 1:
        return ("-d names a metafile of %d archives: joining several bands is not available here (python -m %s -M does "
                "it); give one archive" % (len(datafiles), JOIN_MODULE))
    return None


def fit_refusal(opts):
    """The message for a request about the fit itself that neither command honours, or None."""
    if noise_method_refusal(opts) is not None:
        return noise_method_refusal(opts)
    if opts.figure:
        return "--figure: plots are not available"
    if opts.normalize is not None and opts.normalize not in ("mean", "max", "prof", "rms", "abs"):
        return "Unknown normalization choice, '%s'." % opts.normalize
    if opts.modelfile is None and not float(opts.auto_gauss) and not opts.gauss:
        return ("no initial components: the reference would open a window here; give a model to improve (-I modelfile), "
                "let one component be placed automatically (--autogauss wid), or give the components (--gauss "
                "loc,wid,amp, once for each)")
    if opts.gauss:
        try:
            parse_gauss(opts.gauss)
        except ValueError as e:
            return str(e)
    return None


def load_bunch(datafile):
    """The DataBunch of an .npz archive, with the noise and S/N it lacks measured on the device
    (archive.load_archive_file: a file that cannot be read raises NumPy's own error)."""
    return load_archive_file(datafile)[0]


def load_portrait(datafile):
    """The DataPortrait of an .npz archive (load_bunch)."""
    from .ppgauss import DataPortrait
    return DataPortrait(load_bunch(datafile), quiet=True)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = parser().parse_args(argv)
    msg = refusal(opts)
    if msg is None:
        datafiles = named_datafiles(opts.datafile)
        msg = refusal(opts, datafiles)
    if msg is not None:
        print("ppgauss_run: " + msg, file=sys.stderr)
        return 2
    with noise_method_scope(opts.noise_method):
        return fit_and_write(load_portrait(datafiles[0]), opts, opts.datafile + ".gmodel")


def fit_and_write(dp, opts, default_outfile):
    """Fit the model the options ask for to the DataPortrait dp and write it (with its error
    file) to -o, or without -o and -I to default_outfile."""
    nu_ref = np.float64(opts.nu_ref) if opts.nu_ref else None
    bw_ref = np.float64(opts.bw_ref) if opts.bw_ref else None
    tau = np.float64(opts.tau)
    fixscat = opts.fixscat and opts.fixalpha            # (--fitalpha implies --fitscat)
    if opts.normalize is not None:
        dp.normalize_portrait(opts.normalize)
    outfile = opts.outfile
    if outfile is None and opts.modelfile is None:
        outfile = default_outfile
    if opts.modelfile is not None:
        dp.make_gaussian_model(modelfile=opts.modelfile, fixalpha=opts.fixalpha, model_code=opts.model_code,
                               niter=int(opts.niter), writemodel=True, outfile=outfile, writeerrfile=True,
                               errfile=opts.errfile, model_name=opts.model_name, quiet=opts.quiet)
    else:
        tau *= dp.nbin / dp.Ps[0]                       # [sec] -> [bin]
        dp.make_gaussian_model(modelfile=None, ref_prof=(nu_ref, bw_ref), tau=tau, fixloc=opts.fixloc, fixwid=opts.fixwid,
                               fixamp=opts.fixamp, fixscat=fixscat, fixalpha=opts.fixalpha, model_code=opts.model_code,
                               niter=int(opts.niter), fiducial_gaussian=opts.fgauss, auto_gauss=float(opts.auto_gauss),
                               writemodel=True, outfile=outfile, writeerrfile=True, errfile=opts.errfile,
                               model_name=opts.model_name, quiet=opts.quiet,
                               init_gauss=parse_gauss(opts.gauss) if opts.gauss else None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
