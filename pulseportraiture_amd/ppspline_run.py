"""Command line of ppspline: `python -m pulseportraiture_amd.ppspline_run -d <datafile> [options]`,
the options of the reference's `ppspline.py` (ppspline.py:288-338).

The input is one aligned, averaged portrait: an .npz archive (the fields of a DataBunch) or a
metafile naming one.  It is normalised with -N (default 'prof'), modelled with
DataPortrait.make_spline_model(smooth=False) on the device and written as a .spl pickle
(default datafile.spl) that pptoas_run, ppzap_run -m and the reference read."""
import argparse
import sys

from .archive import (add_noise_method_option, load_archive_file, named_datafiles, noise_method_refusal,
                      noise_method_scope)

MODULE = "pulseportraiture_amd.ppspline_run"
SMOOTH_MODULE = "pulseportraiture_amd.ppspline_smooth_run"


def parser(smooth=False):
    """The options of ppspline_run; smooth=True: those of ppspline_smooth_run (the same, -s and -T in effect)."""
    ap = argparse.ArgumentParser(
        prog="python -m " + (SMOOTH_MODULE if smooth else MODULE),
        description="Make a pulse portrait model using PCA & B-spline interpolation (the reference's "
                    "ppspline.py command line), " + ("with its wavelet smoothing (-s)." if smooth else "without smoothing."))
    ap.add_argument("-d", "--datafile", required=True, metavar="archive",
                    help="One .npz archive (the fields of a DataBunch) from which to make the model, or a "
                         "metafile naming one.  The data should be averaged and aligned.")
    ap.add_argument("-o", "--modelfile", default=None, metavar="modelfile",
                    help="Name for output model (pickle) file. [default=datafile.spl]")
    ap.add_argument("-l", "--model_name", default=None, metavar="model_name",
                    help="Optional name for model [default=datafile.spl].")
    ap.add_argument("-a", "--archive", default=None, metavar="archive", help="Not available: needs PSRCHIVE.")
    ap.add_argument("-N", "--norm", default="prof", metavar="normalization",
                    help="Normalize the input data by channel ('None', 'mean', 'max' (not recommended), 'rms' "
                         "(off-pulse noise), 'prof' (mean profile flux) [default], or 'abs' (sqrt{vector "
                         "modulus})).")
    ap.add_argument("-s", "--smooth", action="store_true",
                    help="Smooth the eigenvectors and mean profile [recommended]: what this command does, with or "
                         "without the flag." if smooth else
                         "Not available here (it was pinned without PyWavelets and lives in "
                         "ppspline_smooth_run): use that command.")
    ap.add_argument("-n", "--max_ncomp", default=10, metavar="max_ncomp",
                    help="Maximum number of principal components to use in PCA reconstruction of the data; "
                         "limited to a maximum of 10 by the B-spline representation.")
    ap.add_argument("-S", "--snr", dest="snr_cutoff", default=150.0, metavar="snr_cutoff",
                    help="S/N ratio cutoff for determining 'significant' eigenprofiles. [default=150.0]")
    ap.add_argument("-T", "--rchi2_tol", default=0.1, metavar="tolerance",
                    help="Tolerance parameter for smoothing.  Bigger value = more smoothing. [default=0.1]" if smooth
                    else "Tolerance of the smoothing [default=0.1]; it takes effect in ppspline_smooth_run.")
    ap.add_argument("-k", "--degree", dest="k", default=3, metavar="degree",
                    help="Degree of the spline.  Cubic splines (k=3) are recommended [default]. 1 <= k <= 5.")
    ap.add_argument("-f", "--sfac", default=1.0, metavar="smooth_factor",
                    help="To change the smoothness of the B-spline model, tweak this between 0.0 (interpolating "
                         "spline that passes through all data points) and a large number (guarantees maximum "
                         "two breakpoints = maximum smoothness).  Alternatively, use -t.")
    ap.add_argument("-t", "--knots", dest="max_nbreak", default=None, metavar="max_knots",
                    help="The maximum number of unique knots.")
    ap.add_argument("--plots", dest="make_plots", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--quiet", action="store_true", help="Suppresses output.")
    add_noise_method_option(ap)
    return ap


def refusal(opts, datafiles=None, smooth=False):
    """The message for a request this command cannot honour, or None."""
    if noise_method_refusal(opts) is not None:
        return noise_method_refusal(opts)
    if opts.smooth and not smooth:
        return ("-s/--smooth: the wavelet smoothing was pinned without PyWavelets and lives beside this "
                "command; run python -m %s (DataPortrait.make_smooth_spline_model) with the same "
                "options" % SMOOTH_MODULE)
    if opts.archive is not None:
        return "-a/--archive needs PSRCHIVE, which this package does not use"
    if opts.make_plots:
        return "--plots: plots are not available"
    if datafiles is not None and len(datafiles) != 1:
        return ("-d names a metafile of %d archives: joining several bands is not available; give one "
                "archive" % len(datafiles))
    return None


def load_portrait(datafile):
    """The DataPortrait of an .npz archive, with the noise and S/N it lacks measured on the device
    (archive.load_archive_file: a file that cannot be read raises NumPy's own error)."""
    from .ppspline import DataPortrait
    return DataPortrait(load_archive_file(datafile)[0], quiet=True)


def main(argv=None, smooth=False):
    """smooth=True: ppspline_smooth_run -- the same flow through make_smooth_spline_model."""
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = parser(smooth).parse_args(argv)
    msg = refusal(opts, smooth=smooth)
    if msg is None:
        datafiles = named_datafiles(opts.datafile)
        msg = refusal(opts, datafiles, smooth=smooth)
    if msg is not None:
        print(("ppspline_smooth_run: " if smooth else "ppspline_run: ") + msg, file=sys.stderr)
        return 2
    with noise_method_scope(opts.noise_method):
        datafile = datafiles[0]
        max_nbreak = None if opts.max_nbreak is None else int(opts.max_nbreak)
        dp = load_portrait(datafile)
        if opts.norm in ("mean", "max", "prof", "rms", "abs"):
            dp.normalize_portrait(opts.norm)
        kw = dict(max_ncomp=int(opts.max_ncomp), snr_cutoff=float(opts.snr_cutoff), rchi2_tol=float(opts.rchi2_tol),
                  k=int(opts.k), sfac=float(opts.sfac), max_nbreak=max_nbreak, model_name=opts.model_name, quiet=opts.quiet)
        if smooth:
            dp.make_smooth_spline_model(**kw)
        else:
            dp.make_spline_model(smooth=False, **kw)
        modelfile = opts.datafile + ".spl" if opts.modelfile is None else opts.modelfile
        dp.write_model(modelfile, quiet=opts.quiet)
        return 0


if __name__ == "__main__":
    sys.exit(main())
