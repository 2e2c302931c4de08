"""Command line of ppzap: `python -m pulseportraiture_amd.ppzap_run -d <datafiles> [options]`,
the options of the reference's `ppzap.py` plus --gpus and --backend (with -m only).

Two methods, as in the reference.  The noise method (the default) measures the channel
noise of every good subint on the device -- after normalising it with -N -- and clips
it there (ppzap.py:200-241).  The model method (-m) fits TOAs with GetTOAs and flags
channels by their reduced chi^2 and S/N (get_channels_to_zap, ppzap.py:169-199); with
--gpus N > 1 the fit is sharded over N ranks started like pptoas_run's, and rank 0
prints."""
import argparse
import contextlib
import os
import sys

import numpy as np

from .archive import (LOAD_ERRORS, add_noise_method_option, list_datafiles, load_bunch, noise_kwargs, noise_method_refusal,
                      noise_method_scope)
from .pptoas_run import PG_TIMEOUT_S, _backend, launch

MODULE = "pulseportraiture_amd.ppzap_run"


def parser():
    ap = argparse.ArgumentParser(
        prog="python -m " + MODULE,
        description="Identify bad channels to zap (the reference's ppzap.py command line).  Archives "
                    "that cannot be loaded are skipped; each zap list is paired with the archive it "
                    "came from (the reference's noise method pairs them with the full list of "
                    "archives, which shifts them after a skipped one).")
    ap.add_argument("-d", "--datafiles", required=True, metavar="archive",
                    help="One .npz archive (the fields of a DataBunch) or a metafile listing archive "
                         "filenames, one per line, to examine.  Files should NOT be dedispersed.")
    ap.add_argument("-n", "--num_std", dest="nstd", default=5.0, metavar="num_std",
                    help="Channels with noise levels greater than num_std standard deviations away from "
                         "the median value will be flagged.  This process is iterated until there are "
                         "zero flagged channels.  This is the default method for ppzap, but is ignored "
                         "if -m is provided.")
    ap.add_argument("-N", "--norm", default=None, metavar="normalization",
                    choices=("mean", "max", "prof", "rms", "abs"),
                    help="Used only with -n, this will normalize the data before proceeding.  "
                         "Normalization method is one of 'mean', 'max', 'prof', 'rms', or 'abs'.")
    ap.add_argument("-m", "--modelfile", default=None, metavar="model",
                    help="Model file: a .gmodel (ppgauss) or a spline model (ppspline), with the same "
                         "nbin as the datafile(s).")
    ap.add_argument("-T", "--tscrunch", action="store_true", help="Not available: needs PSRCHIVE.")
    ap.add_argument("-S", "--SNR-threshold", dest="SNR_threshold", default=8.0, metavar="S/N",
                    help="Set a TOA signal-to-noise ratio threshold for flagging low S/N channels; this is "
                         "used in combination with the number of channels fit to ensure a wideband TOA "
                         "S/N greater than SNR_threshold [default=8.0].")
    ap.add_argument("-R", "--rchi2-threshold", dest="rchi2_threshold", default=1.3, metavar="red_chi2",
                    help="Set a reduced chi-squared threshold for flagging bad channels [default=1.3].")
    ap.add_argument("-o", "--outfile", default=None, metavar="outfile",
                    help="Name of output paz command file. Will append. [default=stdout]")
    ap.add_argument("--modify", action="store_true", help="paz commands will modify original datafiles.")
    ap.add_argument("--hist", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--quiet", action="store_true", help="Suppress output.")
    ap.add_argument("--gpus", type=int, default=1,
                    help="With -m: ranks to shard the TOA fit over (the output is that of one rank).")
    ap.add_argument("--backend", choices=("auto", "nccl", "gloo"), default=None,
                    help="With -m and --gpus > 1: process-group backend; auto = nccl when every rank has "
                         "a GPU of its own, gloo when ranks share one. [default=auto]")
    add_noise_method_option(ap)
    return ap


def refusal(opts):
    """The message for an option this command cannot honour, or None."""
    if noise_method_refusal(opts) is not None:
        return noise_method_refusal(opts)
    if opts.tscrunch:
        return "-T/--tscrunch needs PSRCHIVE, which this package does not use: scrunch the archives with ppscrunch_run -T first"
    if opts.hist:
        return "--hist: plots are not available"
    if opts.gpus < 1:
        return "--gpus must be at least 1"
    if opts.modelfile is None and (opts.gpus > 1 or opts.backend is not None):
        return "the noise method runs on one GPU: --gpus and --backend go with -m"
    return None


def _summary(nzap, nchan, what, opts):
    """The reference's closing line, or (no channel examined, where the reference divides by
    zero) a message and exit code 1."""
    if not nchan:
        print("ppzap_run: no channel to examine in %s" % opts.datafiles, file=sys.stderr)
        return 1
    if not opts.quiet:
        print("ppzap.py found %d channels to zap out of a total %d channels%s (=%.2f%%) in %s." %
              (nzap, nchan, what, 100 * float(nzap) / nchan, opts.datafiles))
    return 0


def noise_method(opts):
    """ppzap.py:200-241, with each zap list paired with its own archive."""
    from .engine import default_engine
    from .ppzap import get_zap_channels, print_paz_cmds
    nstd = float(opts.nstd)
    nchan, names, zap_channels = 0, [], []
    for datafile in list_datafiles(opts.datafiles):
        try:
            data, _ = load_bunch(datafile)
        except LOAD_ERRORS:
            if not opts.quiet:
                print("Cannot load_data(%s).  Skipping it." % datafile)
            continue
        nchan += int(sum(len(c) for c in data.ok_ichans))
        isubs = np.asarray(data.ok_isubs, dtype=int)
        # (an estimator in force is measured whatever the archive stores)
        if (opts.norm is not None or noise_kwargs()) and len(isubs):
            noise = np.zeros((data.nsub, 1, data.nchan)) if data.noise_stds is None else \
                np.array(data.noise_stds, dtype=np.float64)
            noise[isubs, 0] = default_engine().channel_noise(
                np.asarray(data.subints)[isubs, 0], norm=opts.norm,
                weights=np.asarray(data.weights)[isubs], **noise_kwargs())[0]
            data.noise_stds = noise
        names.append(datafile)
        zap_channels.append(get_zap_channels(data, nstd=nstd))
    print_paz_cmds(names, zap_channels, all_subs=False, modify=opts.modify, outfile=opts.outfile,
                   quiet=opts.quiet)
    return _summary(sum(len(z) for zc in zap_channels for z in zc), nchan, "", opts)


@contextlib.contextmanager
def _stdout_to_stderr():
    """File descriptor 1 pointed at stderr: the process-group backend prints its connection
    banner there (gloo: "[Gloo] Rank ... is connected ..."), and stdout carries only what one
    rank would print."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def model_method(opts):
    """ppzap.py:169-199 on one rank or sharded over WORLD_SIZE ranks (rank 0 prints)."""
    from datetime import timedelta
    from .ppzap import print_paz_cmds
    from .pptoas import GetTOAs
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist = None
    try:
        with _stdout_to_stderr() if world > 1 else contextlib.nullcontext():
            if world > 1:
                import torch
                import torch.distributed as dist
                backend = _backend(opts.backend or "auto", world)
                if backend == "nccl":
                    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
                dist.init_process_group(backend, timeout=timedelta(seconds=PG_TIMEOUT_S))
            gt = GetTOAs(list_datafiles(opts.datafiles), opts.modelfile, quiet=True)
            gt.get_TOAs(quiet=True, distributed=world > 1)
        if rank != 0:
            return 0
        gt.get_channels_to_zap(SNR_threshold=float(opts.SNR_threshold),
                               rchi2_threshold=float(opts.rchi2_threshold), iterate=True, show=False)
        ok_datafiles = [gt.datafiles[i] for i in gt.ok_idatafiles]
        print_paz_cmds(ok_datafiles, gt.zap_channels, all_subs=False, modify=opts.modify,
                       outfile=opts.outfile, quiet=opts.quiet)
        nchan = sum(len(c) for arch in gt.channel_red_chi2s for c in arch)
        nzap = sum(len(z) for arch in gt.zap_channels for z in arch)
        rc = _summary(nzap, nchan, " fit", opts)
        sys.stdout.flush()
        return rc
    finally:
        if dist is not None:
            with _stdout_to_stderr():
                dist.destroy_process_group()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = parser().parse_args(argv)
    msg = refusal(opts)
    if msg is not None:
        print("ppzap_run: " + msg, file=sys.stderr)
        return 2
    if opts.modelfile is None:
        with noise_method_scope(opts.noise_method):
            return noise_method(opts)
    if opts.gpus > 1 and "RANK" not in os.environ:
        # (before torch is imported or a GPU is touched: the ranks are a child process)
        return launch(opts.gpus, argv, module=MODULE)
    with noise_method_scope(opts.noise_method):
        return model_method(opts)


if __name__ == "__main__":
    sys.exit(main())
