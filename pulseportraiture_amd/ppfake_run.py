"""Command line of make_fake_pulsar: `python -m pulseportraiture_amd.ppfake_run -m <model.gmodel> -e <pulsar.par>
-o 'fake-%d.npz' [options]`.

The reference has no command for this; the options are the parameter block of its examples/example.py, which
simulates archives with known phases and Delta-DMs, aligns them, builds a template and measures TOAs.  Every file
is one call of pplib.make_fake_pulsar: the portraits are formed on the GPU and written as .npz archives that
ppalign_run, ppspline_run, ppgauss_run, ppzap_run and pptoas_run read.  The injected Delta-DMs are printed, one
line per file."""
import argparse
import sys

MODULE = "pulseportraiture_amd.ppfake_run"
BANNER = "\nppfake_run - Simulates archives from a Gaussian-component model and an ephemeris\n"


def _floats(text):
    return [float(v) for v in str(text).split(",") if v.strip()]


def parser():
    ap = argparse.ArgumentParser(prog="python -m " + MODULE,
                                 usage="%(prog)s -m <model.gmodel> -e <pulsar.par> -o <'name-%%d.npz'> [options]")
    ap.add_argument("-m", "--modelfile", default=None, metavar="model", help="Gaussian-component model file (.gmodel).")
    ap.add_argument("-e", "--ephemeris", default=None, metavar="parfile",
                    help="Ephemeris (.par): PSR or PSRJ, F0 or P0, PEPOCH and DM are read; there is no predictor, "
                         "every subint's period is 1 / F0.")
    ap.add_argument("-o", "--outfile", default="fake-%d.npz", metavar="outfile",
                    help="Output .npz archive; with --nfiles > 1 it must hold one %%d, the file's number from 1. "
                         "[default=fake-%%d.npz]")
    ap.add_argument("--nfiles", type=int, default=1, metavar="int", help="Number of files (epochs). [default=1]")
    ap.add_argument("--days", type=float, default=20.0, metavar="days", help="Days between files. [default=20]")
    ap.add_argument("--MJD0", type=float, default=None, metavar="MJD",
                    help="Start day of the first file. [default: the ephemeris' PEPOCH]")
    ap.add_argument("--nsub", type=int, default=1, metavar="int", help="Subintegrations per file. [default=1]")
    ap.add_argument("--npol", type=int, default=1, metavar="int",
                    help="Polarisations (the same model, noise of their own). [default=1]")
    ap.add_argument("--nchan", type=int, default=64, metavar="int", help="Frequency channels. [default=64]")
    ap.add_argument("--nbin", type=int, default=512, metavar="int", help="Phase bins. [default=512]")
    ap.add_argument("--nu0", type=float, default=1500.0, metavar="MHz", help="Centre of the band. [default=1500]")
    ap.add_argument("--bw", type=float, default=800.0, metavar="MHz", help="Bandwidth. [default=800]")
    ap.add_argument("--tsub", type=float, default=60.0, metavar="sec", help="Length of a subintegration. [default=60]")
    ap.add_argument("--phase", type=float, default=0.0, metavar="rot",
                    help="Delay of every subint [rot], with respect to nu0. [default=0]")
    ap.add_argument("--dDM", default=None, metavar="v[,v...]",
                    help="Injected Delta-DM [cm**-3 pc]: one per file, or one for all. [default=0]")
    ap.add_argument("--dDM_mean", type=float, default=None, metavar="DM",
                    help="Draw one Delta-DM per file from a normal distribution with this mean...")
    ap.add_argument("--dDM_std", type=float, default=None, metavar="DM", help="...and this standard deviation.")
    ap.add_argument("--noise_std", type=float, default=1.0, metavar="flux",
                    help="Noise level of every channel, per subintegration. [default=1]")
    ap.add_argument("--scale", type=float, default=1.0, metavar="factor", help="Scaling of the model's amplitudes. [default=1]")
    ap.add_argument("--dedispersed", action="store_true", help="Store the archives dedispersed.")
    ap.add_argument("--t_scat", type=float, default=0.0, metavar="sec",
                    help="Scattering timescale at nu0; a model with a TAU of its own keeps it. [default=0]")
    ap.add_argument("--alpha", type=float, default=None, metavar="index", help="Scattering index. [default=-4.0]")
    ap.add_argument("--scint", action="store_true", help="Add random scintillation.")
    ap.add_argument("--xs", default=None, metavar="x[,x...]",
                    help="Powers of a DM(nu) law; see add_DM_nu.  Write a list that begins with a minus sign as --xs=-2,-4.")
    ap.add_argument("--Cs", default=None, metavar="C[,C...]", help="Coefficients of the DM(nu) law. [default: ones]")
    ap.add_argument("--nu_DM", default="inf", metavar="MHz", help="Frequency the DM refers to, with --xs. [default=inf]")
    ap.add_argument("--seed", type=int, default=None, metavar="int",
                    help="Seed of the Delta-DM and scintillation draws and of the noise; file k uses seed + k. "
                         "[default: drawn and printed]")
    ap.add_argument("--f64", action="store_true", help="Write float64 portraits. [default: float32]")
    ap.add_argument("--metafile", default=None, metavar="list.txt", help="Write the list of files the other commands take.")
    ap.add_argument("--quiet", action="store_true", help="Only the injected Delta-DMs go to stdout.")
    return ap


def refusal(opts):
    """The message for options this command cannot honour, or None."""
    if opts.nfiles < 1:
        return "--nfiles must be at least 1"
    if min(opts.nsub, opts.npol, opts.nchan) < 1:
        return "--nsub, --npol and --nchan must be at least 1"
    nbin = opts.nbin
    pow2 = nbin >= 32 and nbin <= 8192 and nbin & (nbin - 1) == 0
    if not (pow2 or (nbin >= 8 and nbin <= 4096 and nbin % 2 == 0)):
        return "--nbin %d: a power of two in [32, 8192] or an even number in [8, 4096]" % nbin
    if opts.nfiles > 1:
        try:
            names = set(opts.outfile % k for k in range(1, opts.nfiles + 1))
        except TypeError:
            names = set()
        if len(names) != opts.nfiles:
            return "-o %s: with --nfiles %d the name must hold one %%d" % (opts.outfile, opts.nfiles)
    if (opts.dDM_mean is None) != (opts.dDM_std is None):
        return "--dDM_mean and --dDM_std go together"
    if opts.dDM is not None and opts.dDM_mean is not None:
        return "--dDM and --dDM_mean/--dDM_std exclude each other"
    if opts.dDM_std is not None and opts.dDM_std < 0.0:
        return "--dDM_std must not be negative"
    try:
        if opts.dDM is not None and len(_floats(opts.dDM)) not in (1, opts.nfiles):
            return "--dDM: one value, or one per file (%d)" % opts.nfiles
        for name in ("xs", "Cs"):
            if getattr(opts, name) is not None:
                _floats(getattr(opts, name))
        float(opts.nu_DM)
    except ValueError:
        return "--dDM, --xs, --Cs and --nu_DM take numbers"
    if opts.Cs is not None and opts.xs is None:
        return "--Cs goes with --xs"
    if opts.noise_std < 0.0 or opts.noise_std != opts.noise_std:
        return "--noise_std must not be negative"
    return None


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = parser()
    opts = ap.parse_args(argv)
    if opts.modelfile is None or opts.ephemeris is None:
        print(BANNER)
        ap.print_help()
        print("")
        return 0
    msg = refusal(opts)
    if msg is not None:
        print("ppfake_run: " + msg, file=sys.stderr)
        return 2
    import numpy as np
    from . import parfile, pplib
    from .pptoas import MJD
    try:
        par = parfile.psr_par(opts.ephemeris)
    except (OSError, ValueError) as err:
        print("ppfake_run: %s" % err, file=sys.stderr)
        return 1
    seed = opts.seed
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0] >> np.uint64(2))
        if not opts.quiet:
            print("seed = %d" % seed)
    if opts.dDM_mean is not None:
        dDMs = np.random.default_rng(seed).normal(opts.dDM_mean, opts.dDM_std, opts.nfiles)
    else:
        dDMs = np.ones(opts.nfiles) * (_floats(opts.dDM) if opts.dDM is not None else [0.0])
    MJD0 = float(par.PEPOCH) if opts.MJD0 is None else opts.MJD0
    names = []
    for ifile in range(opts.nfiles):
        name = opts.outfile % (ifile + 1) if "%" in opts.outfile else opts.outfile
        pplib.make_fake_pulsar(
            opts.modelfile, opts.ephemeris, outfile=name, nsub=opts.nsub, npol=opts.npol, nchan=opts.nchan,
            nbin=opts.nbin, nu0=opts.nu0, bw=opts.bw, tsub=opts.tsub, phase=opts.phase, dDM=dDMs[ifile],
            start_MJD=MJD(MJD0 + ifile * opts.days), noise_stds=opts.noise_std, scales=opts.scale,
            dedispersed=opts.dedispersed, t_scat=opts.t_scat,
            alpha=pplib.scattering_alpha if opts.alpha is None else opts.alpha, scint=opts.scint,
            xs=None if opts.xs is None else _floats(opts.xs), Cs=None if opts.Cs is None else _floats(opts.Cs),
            nu_DM=float(opts.nu_DM), quiet=opts.quiet or ifile > 0, seed=seed + ifile + 1,
            dtype=np.float64 if opts.f64 else np.float32)
        names.append(name if name.endswith(".npz") else name + ".npz")
        print("%s  dDM = % .6e" % (names[-1], dDMs[ifile]))
    if opts.metafile is not None:
        with open(opts.metafile, "w") as f:
            f.write("\n".join(names) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
