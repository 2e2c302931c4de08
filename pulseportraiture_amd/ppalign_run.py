"""Command line of ppalign: `python -m pulseportraiture_amd.ppalign_run -M <metafile> [options]`,
the options of the reference's `ppalign.py` (ppalign.py:245-380).

The archives of the metafile (.npz archives of DataBunch fields) are aligned against an initial guess
and averaged on the GPU (ppalign.align_archives); the average is written as an .npz archive that
ppspline_run -d and pptoas_run read.  The initial guess is -I, a Gaussian of the FWHM given with -g,
or -- where the reference calls `psradd -T` -- the weighted mean of the dedispersed archives
(ppalign.average_guess, a stand-in).  One GPU: sharding the archives over ranks would change the
order of the sum, and with it the bytes of the result."""
import argparse
import sys

import numpy as np

from .archive import add_noise_method_option, noise_method_refusal, noise_method_scope

MODULE = "pulseportraiture_amd.ppalign_run"
BANNER = "\nppalign.py - Aligns and averages homogeneous archives by fitting DMs and phases\n"


def parser():
    ap = argparse.ArgumentParser(prog="python -m " + MODULE, usage="%(prog)s -M <metafile> [options]")
    ap.add_argument("-M", "--metafile", default=None, metavar="metafile", dest="metafile",
                    help="Metafile of archives to average together.")
    ap.add_argument("-I", "--init", default=None, metavar="initial_guess", dest="initial_guess",
                    help="Archive containing initial alignment guess.  psradd is used if -I is not used.  (Here: "
                         "the weighted mean of the dedispersed archives stands in for psradd.)")
    ap.add_argument("-g", "--width", default=None, metavar="fwhm", dest="fwhm",
                    help="Use a single Gaussian component of given FWHM to align archives.  Overides -I.")
    ap.add_argument("-D", "--no_DM", default=True, action="store_false", dest="fit_dm",
                    help="Align the subintegrations/archives with a fit for phase only.")
    ap.add_argument("-T", "--tscr", default=False, action="store_true", dest="tscrunch",
                    help="Tscrunch archives for the iterations.  Recommended unless there is reason to keep subint "
                         "resolution (may speed things up).  Not available: needs PSRCHIVE.")
    ap.add_argument("-p", "--poln", default=True, action="store_false", dest="pscrunch",
                    help="Output average Stokes portraits, not just total intensity.  Archives are internally "
                         "converted or skipped (if state == 'Intensity').")
    ap.add_argument("-C", "--cutoff", default=0.0, metavar="SNR_cutoff", dest="SNR_cutoff",
                    help="S/N ratio cutoff to apply to input archives. [default=0.0]  The S/N is the archive's "
                         "prof_SNR field where the .npz has one (PSRCHIVE's number cannot be reproduced), else "
                         "get_SNR of its dedispersed, fully scrunched profile.")
    ap.add_argument("-o", "--outfile", default=None, metavar="outfile", dest="outfile",
                    help="Name of averaged output archive. [default=metafile.algnd.npz]")
    ap.add_argument("-P", "--palign", default=False, action="store_true", dest="palign",
                    help="Passes -P to psradd if -I is not used. [default=False]  Not available: no psradd.")
    ap.add_argument("-N", "--norm", metavar="normalization", dest="norm", default=None,
                    help="Normalize the final averaged data by channel ('None' [default], 'mean', 'max' (not "
                         "recommended), 'prof', 'rms', or 'abs').")
    ap.add_argument("-s", "--smooth", default=False, action="store_true", dest="smooth",
                    help="Output a second averaged archive, smoothed with psrsmooth -W. [default=False]  Not "
                         "available: no psrsmooth.")
    ap.add_argument("-r", "--rot", default=0.0, metavar="phase", dest="rot_phase",
                    help="Additional rotation to add to averaged archive. [default=0.0]")
    ap.add_argument("--place", default=None, metavar="place", dest="place",
                    help="Roughly place pulse to be at the phase given.  Overrides --rot. [default=None]")
    ap.add_argument("--niter", metavar="int", dest="niter", default=1,
                    help="Number of iterations to complete. [default=1]")
    ap.add_argument("--verbose", action="store_false", dest="quiet", default=True, help="More to stdout.")
    return ap


def full_parser():
    """parser(), the reference's options, with the options that are this package's own."""
    ap = parser()
    add_noise_method_option(ap)
    return ap


def refusal(opts):
    """The message for an option this command cannot honour, or None."""
    if noise_method_refusal(opts) is not None:
        return noise_method_refusal(opts)
    if opts.tscrunch:
        return "-T/--tscr needs PSRCHIVE, which this package does not use: scrunch the archives with ppscrunch_run -T first"
    if opts.palign:
        return "-P/--palign goes to psradd -P, which this package does not use"
    if opts.smooth:
        return "-s/--smooth needs psrsmooth, which this package does not use"
    return None


def initial_guess(opts, datafiles):
    """The initial guess as align_archives takes it (ppalign.py:341-368)."""
    from . import ppalign
    from .archive import load_archive
    from .pplib import gaussian_profile
    if opts.initial_guess is None and opts.fwhm is None:
        return ppalign.average_guess(datafiles, quiet=opts.quiet)
    if opts.fwhm is not None:
        first, _ = load_archive(datafiles[0])
        return ppalign.constant_portrait(first, gaussian_profile(first.nbin, 0.5, float(opts.fwhm)))
    guess, _ = load_archive(opts.initial_guess)
    if guess.nchan == 1:       # a constant portrait of its average profile on the first archive's channels
        return ppalign.constant_portrait(datafiles[0], ppalign.scrunched_profile(guess))
    return guess


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = full_parser()
    opts = ap.parse_args(argv)
    if opts.metafile is None or not int(opts.niter):
        print(BANNER)
        ap.print_help()
        print("")
        return 0
    msg = refusal(opts)
    if msg is not None:
        print("ppalign_run: " + msg, file=sys.stderr)
        return 2
    with noise_method_scope(opts.noise_method):
        from . import ppalign
        from .archive import named_datafiles
        rot_phase = np.float64(opts.rot_phase)
        place = None
        if opts.place is not None:
            rot_phase, place = 0.0, np.float64(opts.place)
        datafiles = named_datafiles(opts.metafile)
        outfile = opts.metafile + ".algnd.npz" if opts.outfile is None else opts.outfile
        if not datafiles:
            print("ppalign_run: %s names no archive" % opts.metafile, file=sys.stderr)
            return 1
        try:
            guess = initial_guess(opts, datafiles)
        except RuntimeError as err:         # (the archive the guess is made from cannot be loaded)
            print("ppalign_run: no initial guess: %s" % err, file=sys.stderr)
            return 1
        ppalign.align_archives(datafiles, guess, fit_dm=opts.fit_dm, tscrunch=False, pscrunch=opts.pscrunch,
                               SNR_cutoff=float(opts.SNR_cutoff), outfile=outfile, norm=opts.norm, rot_phase=rot_phase,
                               place=place, niter=int(opts.niter), quiet=opts.quiet)
        return 0


if __name__ == "__main__":
    sys.exit(main())
