"""Command line of joined ppgauss fits: `python -m pulseportraiture_amd.ppgauss_join_run -M <metafile>
[-j joinfile] [options]`, the reference's `ppgauss.py -M ... -j ...` (ppgauss.py:667-743).

The metafile lists one .npz archive per band -- every band's ppalign_run average, or any archive of
one subint -- with the same number of bins.  One Gaussian-component model is fitted to all of them
at once on the device; every band gets a phase offset and a Delta-DM of its own as parameters of
the same fit (band 1 is the phase reference), so that a wideband template can span receivers no
single observation ties together.  The options, the starting components (-I, --autogauss, --gauss)
and the fit are ppgauss_run's.  Written: the .gmodel (default metafile.gmodel) with its error file,
and the join parameters, appended to the joinfile (default <model name>.join in the working
directory); a joinfile given with -j also provides the parameters to start from."""
import sys

from . import ppgauss_run
from .archive import named_datafiles, noise_method_scope

MODULE = ppgauss_run.JOIN_MODULE
MAX_BANDS = 16          # Engine.GAUSS_FIT_MAX_JOIN


def parser():
    return ppgauss_run.parser(joined=True)


def refusal(opts, datafiles=None):
    """The message for a request this command cannot honour, or None."""
    if opts.metafile is None:
        return "no metafile: give the list of the bands' archives with -M/--metafile"
    if opts.datafile is not None:
        return "-d/--datafile: one archive is fitted by python -m %s; here the archives come with -M" % ppgauss_run.MODULE
    msg = ppgauss_run.fit_refusal(opts)
    if msg is not None:
        return msg
    if datafiles is not None and not 1 <= len(datafiles) <= MAX_BANDS:
        return "-M names %d archives: 1..%d bands are joined" % (len(datafiles), MAX_BANDS)
    return None


def load_portrait(datafiles, joinfile=None, metafile=None):
    """The joined DataPortrait of the bands' .npz archives."""
    from .ppgauss import DataPortrait
    return DataPortrait([ppgauss_run.load_bunch(f) for f in datafiles], joinfile=joinfile, quiet=True, metafile=metafile)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = parser().parse_args(argv)
    msg = refusal(opts)
    if msg is None:
        datafiles = [f.strip() for f in named_datafiles(opts.metafile)]
        msg = refusal(opts, datafiles)
    if msg is not None:
        print("ppgauss_join_run: " + msg, file=sys.stderr)
        return 2
    with noise_method_scope(opts.noise_method):
        try:
            dp = load_portrait(datafiles, opts.joinfile, opts.metafile)
        except (ValueError, OSError) as e:
            print("ppgauss_join_run: %s" % e, file=sys.stderr)
            return 2
        return ppgauss_run.fit_and_write(dp, opts, opts.metafile + ".gmodel")


if __name__ == "__main__":
    sys.exit(main())
