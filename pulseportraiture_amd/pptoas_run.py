"""Command line of the TOA driver: `python -m pulseportraiture_amd.pptoas_run -d <datafiles>
-m <model> [options]`, the options of the reference's `pptoas.py` plus --gpus, --seed and
--backend.

With --gpus N > 1 (and no RANK in the environment) the command starts its N ranks itself:
`python -m torch.distributed.run ... -m pulseportraiture_amd.pptoas_run <same args>` as a
CHILD process (launch), before torch is imported or any GPU is touched.  Each rank then
runs get_TOAs(distributed=True) and rank 0 writes the TOAs."""
import argparse
import os
import signal
import socket
import subprocess
import sys
import threading
import time

from .archive import add_noise_method_option, noise_method_refusal, noise_method_scope

MODULE = "pulseportraiture_amd.pptoas_run"
GRACE_S = 10.0
PG_TIMEOUT_S = 1800.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _children():
    """{pid: ppid} of every live (not zombie) process, from /proc."""
    out = {}
    for name in os.listdir("/proc"):
        if not name.isdigit():
            continue
        try:
            with open("/proc/%s/stat" % name) as f:
                stat = f.read()
        except OSError:
            continue
        fields = stat[stat.rindex(")") + 2:].split()
        if fields[0] != "Z":
            out[int(name)] = int(fields[1])
    return out


def _descendants(pid):
    table, found, todo = _children(), set(), [pid]
    while todo:
        p = todo.pop()
        for c, pp in table.items():
            if pp == p and c not in found:
                found.add(c)
                todo.append(c)
    return found


def _kill(pids, sig):
    for p in pids:
        try:
            os.kill(p, sig)
        except OSError:
            pass


def launch(nproc, argv, module=MODULE, grace=GRACE_S, env=None):
    """Run `module` with `argv` on `nproc` local ranks under torch.distributed.run, in a
    CHILD process of its own session (never an exec).  SIGINT / SIGTERM received here are
    forwarded as SIGTERM to the child's process group; when the child has ended (or been
    told to), what is left of it and of its ranks -- which torch.distributed.run starts
    in sessions of their own -- gets `grace` seconds and then SIGKILL.  Returns the child's
    exit code (128 + signal for a child killed by a signal)."""
    env = dict(os.environ if env is None else env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = os.pathsep.join([root] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this driver
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(nproc)),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "-m", module] + list(argv)
    proc = subprocess.Popen(cmd, env=env, start_new_session=True)
    stop = []

    def forward(signum, frame):
        stop.append(signum)
        try:
            os.killpg(proc.pid, signal.SIGTERM)
        except OSError:
            pass
    old = {}
    if threading.current_thread() is threading.main_thread():
        old = {s: signal.signal(s, forward) for s in (signal.SIGINT, signal.SIGTERM)}
    seen = set()
    try:
        while proc.poll() is None:
            seen |= _descendants(proc.pid)
            try:
                proc.wait(timeout=0.5)
            except subprocess.TimeoutExpired:
                pass
    finally:
        if proc.poll() is None:                 # (an exception here: end the child as a signal would)
            forward(signal.SIGTERM, None)
        deadline = time.time() + grace
        while proc.poll() is None and time.time() < deadline:
            time.sleep(0.1)
        left = lambda: [p for p in seen if p in _children()]    # noqa: E731
        while left() and time.time() < deadline:
            time.sleep(0.1)
        if proc.poll() is None:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except OSError:
                pass
        _kill(left(), signal.SIGKILL)
        rc = proc.wait()
        for s, h in old.items():
            signal.signal(s, h)
    return rc if rc >= 0 else 128 - rc


def parser():
    ap = argparse.ArgumentParser(
        prog="python -m " + MODULE,
        description="Measure wideband TOAs and DMs (the reference's pptoas.py command line) on one "
                    "or more GPUs.")
    ap.add_argument("-d", "--datafiles", required=True, metavar="archive",
                    help="One .npz archive (the fields of a DataBunch) or a metafile listing archive "
                         "filenames, one per line.")
    ap.add_argument("-m", "--modelfile", required=True, metavar="model",
                    help="Model file: a .gmodel (ppgauss) or a spline model (ppspline).")
    ap.add_argument("-o", "--outfile", metavar="timfile", default=None,
                    help="Output .tim file; appended to. [default=stdout]")
    ap.add_argument("--narrowband", action="store_true", help="Make narrowband TOAs instead (one GPU).")
    ap.add_argument("--psrchive", action="store_true", help="Not available: needs PSRCHIVE.")
    ap.add_argument("--errfile", default=None, help="Not available: needs the 'princeton' format.")
    ap.add_argument("-T", "--tscrunch", action="store_true", help="Not available: needs PSRCHIVE.")
    ap.add_argument("-f", "--format", default=None,
                    help="Output format: 'ipta' (the default and the only one available).")
    ap.add_argument("--nu_ref", dest="nu_ref_DM", default=None, metavar="nu_ref",
                    help="Topocentric frequency [MHz] the TOAs are referenced to; 'inf' for infinite "
                         "frequency (written as 0.0). [default: zero-covariance frequency]")
    ap.add_argument("--DM", dest="DM0", default=None,
                    help="Nominal DM [cm**-3 pc] the DM offsets refer to. [default: each archive's DM]")
    ap.add_argument("--no_bary", dest="bary", action="store_false",
                    help="Do not Doppler-correct DMs, GMs, taus or nu_tau.")
    ap.add_argument("--one_DM", action="store_true",
                    help="Write one DM per archive on its TOA lines: its mean DM offset plus its DM0, that "
                         "offset's error, and the flag DM_mean.  (What the reference intends; its own "
                         "pptoas.py raises NameError here.)")
    ap.add_argument("--fix_DM", dest="fit_DM", action="store_false", help="Do not fit for DM.")
    ap.add_argument("--fit_dt4", dest="fit_GM", action="store_true",
                    help="Fit for delays that scale as nu**-4 (GM).")
    ap.add_argument("--fit_scat", action="store_true",
                    help="Fit for scattering timescale and index (with --narrowband: a timescale per channel).")
    ap.add_argument("--no_logscat", "--no_log10_tau", dest="log10_tau", action="store_false",
                    help="Fit the scattering timescale itself, not its log10.")
    ap.add_argument("--scat_guess", default=None, metavar="tau,freq,alpha",
                    help="Initial scattering timescale [s], its reference frequency [MHz] and index.")
    ap.add_argument("--fix_alpha", action="store_true", help="Fix the scattering index (with --fit_scat).")
    ap.add_argument("--nu_tau", dest="nu_ref_tau", default=None, metavar="nu_ref_tau",
                    help="Frequency [MHz] the scattering times are referenced to. [default: zero-covariance "
                         "frequency]")
    ap.add_argument("--print_phase", action="store_true", help="Add the fitted phase (-phs) to each TOA.")
    ap.add_argument("--print_flux", action="store_true", help="Add a flux density estimate to each TOA.")
    ap.add_argument("--print_parangle", action="store_true", help="Add the parallactic angle to each TOA.")
    ap.add_argument("--flags", dest="toa_flags", default="", metavar="k,v,...",
                    help="Flag/value pairs written to every TOA, e.g. pta,NANOGrav,version,0.1")
    ap.add_argument("--snr_cut", dest="snr_cutoff", default=0.0, type=float, metavar="S/N",
                    help="Write only TOAs with at least this S/N.")
    ap.add_argument("--showplot", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--saveplot", action="store_true", help="Not available: no plotting.")
    ap.add_argument("--quiet", action="store_true", help="Only the TOAs are written to stdout.")
    ap.add_argument("--gpus", type=int, default=1,
                    help="Ranks to shard the archives (or, with fewer archives, the subints) over.")
    ap.add_argument("--seed", choices=("reference", "device"), default="reference",
                    help="Initial phase guess: the reference's (default) or the device's fast seed.")
    ap.add_argument("--backend", choices=("auto", "nccl", "gloo"), default="auto",
                    help="Process-group backend for --gpus > 1: auto = nccl when every rank has a GPU of "
                         "its own, gloo when ranks share one.")
    add_noise_method_option(ap)
    return ap


def refusal(opts):
    """The message for an option this command cannot honour, or None."""
    if noise_method_refusal(opts) is not None:
        return noise_method_refusal(opts)
    if opts.psrchive:
        return "--psrchive needs PSRCHIVE, which this package does not use"
    if opts.tscrunch:
        return "-T/--tscrunch needs PSRCHIVE, which this package does not use: scrunch the archives with ppscrunch_run -T first"
    if opts.showplot or opts.saveplot:
        return "--showplot/--saveplot: plots are not available"
    if opts.format is not None and opts.format.lower() == "princeton":
        return "-f princeton: the reference has no writer for it (write_princeton_TOAs); use the IPTA format"
    if opts.format is not None and opts.format.lower() != "ipta":
        return "-f %s: unknown format (only 'ipta')" % opts.format
    if opts.errfile is not None:
        return "--errfile goes with the 'princeton' format, which is not available"
    if opts.narrowband and opts.gpus > 1:
        return "--narrowband runs on one GPU: drop --gpus"
    if opts.gpus < 1:
        return "--gpus must be at least 1"
    return None


def get_toas_kwargs(opts):
    """get_TOAs keyword arguments of the parsed options (the reference's mapping)."""
    import numpy as np
    nu_ref_DM = opts.nu_ref_DM
    nu_refs = None
    if nu_ref_DM:
        nu_ref_DM = np.inf if nu_ref_DM == "inf" else np.float64(nu_ref_DM)
        nu_refs = (nu_ref_DM, None)
    if opts.nu_ref_tau:
        nu_refs = (nu_ref_DM if nu_ref_DM else None, np.float64(opts.nu_ref_tau))
    DM0 = np.float64(opts.DM0) if opts.DM0 else None
    scat_guess = [float(s.upper()) for s in opts.scat_guess.split(",")] if opts.scat_guess else None
    items = opts.toa_flags.split(",")
    flags = dict(zip(items[::2], items[1::2])) if opts.toa_flags else {}
    return dict(nu_refs=nu_refs, DM0=DM0, bary=opts.bary, fit_DM=opts.fit_DM, fit_GM=opts.fit_GM,
                fit_scat=opts.fit_scat, log10_tau=opts.log10_tau, scat_guess=scat_guess,
                fix_alpha=opts.fix_alpha, print_phase=opts.print_phase, print_flux=opts.print_flux,
                print_parangle=opts.print_parangle, addtnl_toa_flags=flags, method='trust-ncg',
                quiet=opts.quiet, seed=opts.seed)


def get_narrowband_kwargs(opts):
    """get_narrowband_TOAs keyword arguments of the parsed options."""
    kw = get_toas_kwargs(opts)
    return {k: kw[k] for k in ("fit_scat", "log10_tau", "scat_guess", "print_phase", "print_flux",
                               "print_parangle", "addtnl_toa_flags", "method", "quiet")}


def one_DM_toas(gt):
    """TOA_list with every TOA's DM replaced by its archive's mean DM offset plus DM0, its
    error by that offset's error, and the flag DM_mean (TOA_list holds the archives' TOAs in
    order, len(ok_isubs) each)."""
    toas, k = [], 0
    for ia, ok in enumerate(gt.ok_isubs):
        for toa in gt.TOA_list[k:k + len(ok)]:
            toa.DM = gt.DeltaDM_means[ia] + gt.DM0s[ia]
            toa.DM_error = gt.DeltaDM_errs[ia]
            toa.flags['DM_mean'] = True
            toas.append(toa)
        k += len(ok)
    return toas


def _backend(choice, world):
    import torch
    if choice != "auto":
        return choice
    return "nccl" if torch.cuda.device_count() >= world else "gloo"


def run(opts):
    """One rank's (or the single process's) work; returns the exit code."""
    from datetime import timedelta
    from .pptoas import GetTOAs, write_TOAs
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        backend = _backend(opts.backend, world)
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
        dist.init_process_group(backend, timeout=timedelta(seconds=PG_TIMEOUT_S))
    try:
        with noise_method_scope(opts.noise_method):
            gt = GetTOAs(opts.datafiles, opts.modelfile, quiet=opts.quiet)
            if opts.narrowband:
                gt.get_narrowband_TOAs(**get_narrowband_kwargs(opts))
            else:
                gt.get_TOAs(distributed=world > 1, **get_toas_kwargs(opts))
        if rank == 0:
            toas = one_DM_toas(gt) if (opts.one_DM and not opts.narrowband) else gt.TOA_list
            write_TOAs(toas, inf_is_zero=True, SNR_cutoff=opts.snr_cutoff, outfile=opts.outfile, append=True)
            sys.stdout.flush()
    finally:
        if dist is not None:
            dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = parser().parse_args(argv)
    msg = refusal(opts)
    if msg is not None:
        print("pptoas_run: " + msg, file=sys.stderr)
        return 2
    if opts.gpus > 1 and "RANK" not in os.environ:
        # (before torch is imported or a GPU is touched: the ranks are a child process)
        return launch(opts.gpus, argv)
    return run(opts)


if __name__ == "__main__":
    sys.exit(main())
