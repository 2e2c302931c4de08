"""ppzap: flag noisy channels (the reference's ppzap.py).

get_zap_channels runs the iterative median / sigma clip of every good subint on the
device (Engine.zap_median); when the DataBunch carries no noise_stds, the channel noise
is measured there too (Engine.channel_noise).  print_paz_cmds writes the reference's
paz commands byte for byte.  The command line is pulseportraiture_amd.ppzap_run."""
import sys

import numpy as np

from .archive import noise_kwargs
from .engine import default_engine


def _good_mask(data, isubs):
    good = np.zeros((len(isubs), int(data.nchan)), dtype=np.uint8)
    for j, isub in enumerate(isubs):
        good[j, np.asarray(data.ok_ichans[isub], dtype=int)] = 1
    return good


def get_zap_channels(data, nstd=3, noise_method=None):
    """Proposed channels to zap by the median algorithm (ppzap.py:18-47): in every good
    subint, channels whose noise is more than nstd standard deviations above the median
    of the good channels' noise are flagged and removed, until a round flags none.

    data is a DataBunch; its noise_stds[isub, 0] are used, or the power-spectrum noise
    of its portraits measured on the device when it has none -- with the estimator in force
    (archive.noise_method_scope), else 'PS'.  noise_stds that the bunch carries are the
    caller's and are clipped as they are, whatever is in force: ppzap_run puts the noise of
    the NORMALISED rows there, which a second measurement here would undo.  Only an
    explicit noise_method ('PS' or 'fit') measures anew over them.  Returns one sorted list
    of channel indices per entry of data.ok_isubs, in that order."""
    isubs = np.asarray(data.ok_isubs, dtype=int)
    if not len(isubs):
        return []
    eng = default_engine()
    if data.noise_stds is not None and noise_method is None:
        noise = np.asarray(data.noise_stds, dtype=np.float64)[isubs, 0]
    else:
        noise = eng.channel_noise(np.asarray(data.subints)[isubs, 0], **noise_kwargs(noise_method))[0]
    zap = eng.zap_median(noise, _good_mask(data, isubs), nstd)
    return [[int(n) for n in np.nonzero(row)[0]] for row in zap]


def print_paz_cmds(datafiles, zap_list, all_subs=False, modify=True, outfile=None, quiet=False):
    """Print paz commands for a list of datafiles and a zap list (ppzap.py:49-99).

    zap_list[iarch][isub] holds the channel indices to zap; isub is the position in
    that archive's list (what paz -w is given).  all_subs=True zaps each listed
    channel in every subint; modify=True modifies the archives (paz -m), otherwise
    the commands write a .zap copy (paz -e zap).  outfile=None prints to stdout,
    otherwise the commands are appended to outfile.  quiet=True suppresses the
    "Nothing to zap." and "Wrote ..." messages, as in the reference."""
    if not len(datafiles) or not len(zap_list):
        if not quiet:
            print("Nothing to zap.")
            return None
    out = open(outfile, "a") if outfile is not None else sys.stdout
    try:
        paz_outfile = None
        for iarch, datafile in enumerate(datafiles):
            count = 0
            for isub in range(len(zap_list[iarch])):
                count += len(zap_list[iarch][isub])
            if count:
                if modify:
                    paz_outfile = datafile
                else:
                    ii = datafile[::-1].find(".")
                    if ii < 0:
                        paz_outfile = datafile + ".zap"
                    else:
                        paz_outfile = datafile[:-ii] + "zap"
                    print("paz -e zap %s" % datafile, file=out)
            last_line = ""
            for isub, bad_ichans in enumerate(zap_list[iarch]):
                for bad_ichan in bad_ichans:
                    if not all_subs:
                        print("paz -m -I -z %d -w %d %s" % (bad_ichan, isub, paz_outfile), file=out)
                    else:
                        line = "paz -m -z %d %s" % (bad_ichan, paz_outfile)
                        if line != last_line:
                            print(line, file=out)
                        last_line = line
    finally:
        if outfile is not None:
            out.close()
    if outfile is not None and not quiet:
        print("Wrote %s." % outfile)
