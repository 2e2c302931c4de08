"""Command line of the archive operations: `python -m pulseportraiture_amd.ppscrunch_run -d <datafiles> [options]`,
the package's `pam`: scrunch .npz archives in time (-T / --setnsub N), frequency (-F / --setnchn N) and polarisation
(-p), dedisperse (-D) or dededisperse them, on the device (pulseportraiture_amd.scrunch), and write them as .npz
archives every command here reads.  The operations run in load_data's order: (de)dedisperse, time, polarisation,
frequency.  There is no baseline removal and no bscrunch."""
import argparse
import os
import sys

from . import archive

MODULE = "pulseportraiture_amd.ppscrunch_run"


def parser():
    ap = argparse.ArgumentParser(
        prog="python -m " + MODULE,
        description="Scrunch .npz archives in time, frequency and polarisation on the GPU (PSRCHIVE's pam for the "
                    "archives of this package).  Archives that cannot be loaded are skipped.")
    ap.add_argument("-d", "--datafiles", required=True, metavar="archive",
                    help="One .npz archive (the fields of a DataBunch) or a metafile listing archive filenames, one per line.")
    ap.add_argument("-T", "--tscrunch", action="store_true", help="Add all subints (one subint out).")
    ap.add_argument("--setnsub", type=int, default=None, metavar="N", help="Add subints into N contiguous groups.")
    ap.add_argument("-F", "--fscrunch", action="store_true", help="Add all channels (one channel out).")
    ap.add_argument("--setnchn", type=int, default=None, metavar="N", help="Add channels into N contiguous groups.")
    ap.add_argument("-p", "--pscrunch", action="store_true", help="Total intensity only.")
    ap.add_argument("-D", "--dedisperse", action="store_true", help="Dedisperse about the centre frequency.")
    ap.add_argument("--dededisperse", action="store_true", help="Put the dispersion delay back.")
    ap.add_argument("-e", "--ext", default="scr.npz", metavar="ext",
                    help="Output beside the input under this extension. [default=scr.npz]")
    ap.add_argument("-o", "--outfile", default=None, metavar="outfile", help="Name of the output archive (one archive only).")
    ap.add_argument("--metafile", default=None, metavar="out.txt", help="Write the names of the output archives here.")
    ap.add_argument("--quiet", action="store_true", help="Suppress output.")
    archive.add_noise_method_option(ap)
    return ap


def refusal(opts):
    """The message for a combination this command cannot honour, or None."""
    if archive.noise_method_refusal(opts) is not None:
        return archive.noise_method_refusal(opts)
    if opts.tscrunch and opts.setnsub is not None:
        return "-T and --setnsub exclude each other"
    if opts.fscrunch and opts.setnchn is not None:
        return "-F and --setnchn exclude each other"
    if opts.dedisperse and opts.dededisperse:
        return "-D and --dededisperse exclude each other"
    if (opts.setnsub is not None and opts.setnsub < 1) or (opts.setnchn is not None and opts.setnchn < 1):
        return "--setnsub and --setnchn take a positive number"
    return None


def output_name(datafile, ext):
    """<datafile without its last extension>.<ext>, beside the input."""
    return os.path.splitext(str(datafile))[0] + "." + str(ext).lstrip(".")


def write_archive(outfile, data):
    """The DataBunch as an .npz archive.load_bunch and archive.load_archive read back: the fields of data_from_arrays
    (noise_stds and SNRs among them) plus state; epochs as float days.  Not prof_SNR: that was the S/N of the archive
    before it was scrunched."""
    names = archive.ARRAY_FIELDS + archive.SCALAR_FIELDS + archive.EXTRA_FIELDS
    return archive.write_archive(outfile, {k: data.get(k) for k in names if k != "prof_SNR"})


def scrunched(data, opts, engine=None):
    """The operations `opts` asks for, in load_data's order."""
    from . import scrunch as sc
    if opts.dedisperse:
        data = sc.dedisperse(data, engine=engine)
    if opts.dededisperse:
        data = sc.dededisperse(data, engine=engine)
    if opts.tscrunch or opts.setnsub is not None:
        data = sc.tscrunch(data, nsub=opts.setnsub, engine=engine)
    if opts.pscrunch:
        data = sc.pscrunch(data, engine=engine)
    if opts.fscrunch or opts.setnchn is not None:
        data = sc.fscrunch(data, nchan=opts.setnchn, engine=engine)
    return data


def main(argv=None):
    opts = parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    msg = refusal(opts)
    if msg is not None:
        print("ppscrunch_run: " + msg, file=sys.stderr)
        return 2
    with archive.noise_method_scope(opts.noise_method):
        from .engine import default_engine
        from .scrunch import state_of
        datafiles = archive.named_datafiles(opts.datafiles)
        if opts.outfile is not None and len(datafiles) != 1:
            print("ppscrunch_run: -o names one output, %s names %d archives" % (opts.datafiles, len(datafiles)), file=sys.stderr)
            return 2
        eng = default_engine()
        written = []
        for datafile in datafiles:
            try:
                data, _ = archive.load_archive(datafile, eng)
            except RuntimeError as err:
                if not opts.quiet:
                    print("Cannot load_data(%s).  Skipping it." % datafile)
                    print(err)
                continue
            try:
                data.state = state_of(data)
                data = scrunched(data, opts, eng)
            except ValueError as err:            # (more groups asked for than the archive has members)
                if not opts.quiet:
                    print("%s: %s.  Skipping it." % (datafile, err))
                continue
            out = write_archive(opts.outfile or output_name(datafile, opts.ext), data)
            written.append(out)
            if not opts.quiet:
                print("Unloaded %s: %d subint(s) x %d pol x %d channel(s) x %d bins." % (out, data.nsub, data.npol, data.nchan, data.nbin))
        if opts.metafile is not None:
            with open(opts.metafile, "w") as f:
                f.write("".join(name + "\n" for name in written))
        return 0 if written else 1


if __name__ == "__main__":
    sys.exit(main())
