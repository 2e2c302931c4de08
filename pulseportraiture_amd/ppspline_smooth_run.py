"""Command line of ppspline with the reference's wavelet smoothing:
`python -m pulseportraiture_amd.ppspline_smooth_run -d <datafile> [options]`, the options of ppspline_run
(the reference's `ppspline.py -s`, ppspline.py:288-338).

The eigenvectors and the mean profile are smoothed on the device (pplib.smart_smooth; -T is its tolerance) and
the .spl model is built from the smoothed basis (DataPortrait.make_smooth_spline_model)."""
import sys

from . import ppspline_run


def parser():
    return ppspline_run.parser(smooth=True)


def refusal(opts, datafiles=None):
    return ppspline_run.refusal(opts, datafiles, smooth=True)


def main(argv=None):
    return ppspline_run.main(argv, smooth=True)


if __name__ == "__main__":
    sys.exit(main())
