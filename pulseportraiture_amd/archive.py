"""The package's archives: `.npz` files holding the fields of the DataBunch the reference's load_data returns
(pplib.py:2650-2814), and the metafiles that list them.  PSRFITS I/O needs PSRCHIVE, which is outside this package.

The format is stated once, in ARRAY_FIELDS, SCALAR_FIELDS and EXTRA_FIELDS; `load_bunch` (as stored) and `load_archive`
(noise and S/N measured on the device where the file lacks them; `load_archive_file` is the same with NumPy's own
errors) read it, `write_archive` writes it.  This module
stands below every command and every library module that touches an archive: it imports none of them.
"""
import contextlib
import zipfile

import numpy as np

from ._lib import NOISE_METHODS as _NOISE_METHODS
from .pplib import DataBunch, default_engine, get_bin_centers

# ---- the format: the arguments of data_from_arrays ... ----
# arrays, one entry (or row) per subint; epochs are stored as float days
ARRAY_FIELDS = ("subints", "freqs", "Ps", "epochs", "weights", "noise_stds", "SNRs", "doppler_factors", "subtimes",
                "parallactic_angles")
# the header, stored as 0-d arrays
SCALAR_FIELDS = ("DM", "dmc", "backend_delay", "telescope", "telescope_code", "backend", "frontend", "source", "bw",
                 "nu0")
# ... and what an archive may carry beside them: its own S/N (e.g. PSRCHIVE's) and its polarisation state
# ('Intensity', 'Stokes' or 'Coherence'), attached to the loaded bunch
EXTRA_FIELDS = ("prof_SNR", "state")
# read back as Python scalars; bw and nu0 stay the 0-d arrays they are stored as (in a bunch built without them they
# are NumPy scalars too: data_from_arrays derives them from freqs)
_UNWRAPPED = tuple(k for k in SCALAR_FIELDS if k not in ("bw", "nu0")) + EXTRA_FIELDS

# what loading an archive that is missing, not an .npz of DataBunch fields, or damaged (BadZipFile: cut short) raises
LOAD_ERRORS = (RuntimeError, OSError, ValueError, zipfile.BadZipFile)


# ---------------------------------------------------------------------------
# epochs: integer day + fraction of a day (PSRCHIVE's MJD keeps day, seconds
# and fractional seconds; a float64 fraction resolves 1e-16 d = 9 ps)
# ---------------------------------------------------------------------------
class MJD(object):
    def __init__(self, day=0, frac=0.0):
        if isinstance(day, MJD):
            day, frac = day._day, day._frac
        elif not isinstance(day, (int, np.integer)):
            whole = np.floor(day)
            day, frac = int(whole), float(day - whole) + float(frac)
        carry = np.floor(frac)
        self._day = int(day) + int(carry)
        self._frac = float(frac - carry)

    def intday(self):
        return self._day

    def fracday(self):
        return self._frac

    def in_days(self):
        return self._day + self._frac

    def __add__(self, other):
        other = other if isinstance(other, MJD) else MJD(other)
        return MJD(self._day + other._day, self._frac + other._frac)

    __radd__ = __add__

    def __sub__(self, other):
        other = other if isinstance(other, MJD) else MJD(other)
        return MJD(self._day - other._day, self._frac - other._frac)

    def __repr__(self):
        return "MJD(%d%s)" % (self._day, ("%.15f" % self._frac)[1:])


def data_from_arrays(subints, freqs, Ps, epochs, weights=None, noise_stds=None,
                     SNRs=None, DM=0.0, dmc=0, doppler_factors=None,
                     backend_delay=0.0, telescope="GBT", telescope_code="1",
                     backend="GUPPI", frontend="Rcvr", bw=None, nu0=None,
                     subtimes=None, parallactic_angles=None, source="noname",
                     filename="arrays"):
    """Build the DataBunch `load_data` would return (pplib.py:2650-2814) from
    arrays: subints[nsub,npol,nchan,nbin], freqs[nsub,nchan], Ps[nsub], epochs
    (MJD objects or floats).  Zero-weight channels are excluded like the
    reference does (pplib.py:2755-2757); noise defaults to the power-spectrum
    estimate per channel (get_noise_PS), computed on the device."""
    subints = np.asarray(subints)
    if subints.ndim == 3:
        subints = subints[:, None]
    nsub, npol, nchan, nbin = subints.shape
    freqs = np.broadcast_to(np.asarray(freqs, dtype=np.float64), (nsub, nchan)).copy()
    weights = np.ones((nsub, nchan)) if weights is None else \
        np.asarray(weights, dtype=np.float64)
    ok_ichans = [np.where(weights[i] > 0)[0] for i in range(nsub)]
    ok_isubs = np.array([i for i in range(nsub) if len(ok_ichans[i])], dtype=int)
    if SNRs is None:
        SNRs = np.ones((nsub, npol, nchan))
    epochs = [e if isinstance(e, MJD) else MJD(e) for e in epochs]
    Ps = np.asarray(Ps, dtype=np.float64)
    if doppler_factors is None:
        doppler_factors = np.ones(nsub)
    if subtimes is None:
        subtimes = np.zeros(nsub)
    if parallactic_angles is None:
        parallactic_angles = np.zeros(nsub)
    if bw is None:
        bw = (freqs[0].max() - freqs[0].min()) * nchan / max(nchan - 1, 1)
    if nu0 is None:
        nu0 = freqs[0].mean()
    return DataBunch(
        subints=subints, freqs=freqs, weights=weights, noise_stds=noise_stds,
        SNRs=np.asarray(SNRs, dtype=np.float64), Ps=Ps, epochs=epochs,
        ok_isubs=ok_isubs, ok_ichans=ok_ichans, DM=DM, dmc=dmc,
        doppler_factors=np.asarray(doppler_factors, dtype=np.float64), nbin=nbin,
        nchan=nchan, nsub=nsub, npol=npol, phases=get_bin_centers(nbin),
        backend_delay=backend_delay, telescope=telescope,
        telescope_code=telescope_code, backend=backend, frontend=frontend, bw=bw,
        nu0=nu0, subtimes=np.asarray(subtimes, dtype=np.float64),
        integration_length=float(np.sum(subtimes)),
        parallactic_angles=np.asarray(parallactic_angles, dtype=np.float64),
        source=source, filename=filename, masks=(weights > 0)[:, None, :, None])


# ---------------------------------------------------------------------------
# metafiles
# ---------------------------------------------------------------------------
def list_datafiles(datafiles):
    """The archives named by -d: the lines of a metafile when -d names a text file (the
    reference asks `file` whether it is ASCII, pplib.py:3015-3031), else -d itself."""
    try:
        with open(datafiles, "rb") as f:
            head = f.read(1 << 16)
    except OSError:
        return [datafiles]
    try:
        if b"\0" in head:
            return [datafiles]
        head.decode("utf-8")
    except UnicodeDecodeError:
        return [datafiles]
    with open(datafiles) as f:
        return [line.rstrip("\n") for line in f]


def named_datafiles(datafiles):
    """list_datafiles without its blank lines."""
    return [f for f in list_datafiles(datafiles) if f.strip()]


# ---------------------------------------------------------------------------
# reading
# ---------------------------------------------------------------------------
def _read(datafile):
    """(DataBunch, name, whether it came with SNRs) of a DataBunch -- the same object -- or of an .npz archive."""
    if isinstance(datafile, dict):
        return datafile, datafile.get("filename", "arrays"), True
    if not str(datafile).endswith(".npz"):
        raise RuntimeError("Cannot load_data(%s): PSRFITS archives need PSRCHIVE; pass a "
                           "DataBunch (data_from_arrays) or an .npz of its fields." % datafile)
    with np.load(datafile, allow_pickle=True) as z:
        kw = {k: z[k] for k in z.files}
    for k in _UNWRAPPED:
        if k in kw:
            kw[k] = kw[k].item()
    extras = {k: kw.pop(k) for k in EXTRA_FIELDS if k in kw}
    kw.setdefault("filename", str(datafile))
    data = data_from_arrays(**kw)
    data.update(extras)
    return data, str(datafile), "SNRs" in kw


def load_bunch(datafile):
    """(DataBunch, name) of an archive as it is stored, nothing measured: a DataBunch, handed back as it is, or an
    .npz of its fields.  RuntimeError for any other name; whatever NumPy raises for an .npz it cannot read."""
    return _read(datafile)[:2]


# ---------------------------------------------------------------------------
# the noise estimator
# ---------------------------------------------------------------------------
# pplib.get_noise's methods (pplib.py:2206-2225).  The reference has one module constant; here every function that
# measures noise takes noise_method=None, and None means whatever noise_method_scope has put in force -- nothing,
# unless a command line said --noise_method: today's power-spectrum estimate wherever the archive stores no value.
NOISE_METHODS = _NOISE_METHODS
_IN_FORCE = [None]


def add_noise_method_option(ap):
    """--noise_method for a command's parser (its value is checked by noise_method_refusal, through the command's
    own refusal())."""
    ap.add_argument("--noise_method", default=None, metavar="{PS,fit}",
                    help="Noise estimator: 'PS', the mean of the top quarter of the power spectrum, or 'fit', the "
                         "mean above a fitted noise-floor harmonic (get_noise_fit).  Given, it is measured anew "
                         "even where the archive stores noise_stds and SNRs. [default: stored values, else 'PS']")


def noise_method_refusal(opts):
    """The message for a --noise_method that is no estimator, or None."""
    value = getattr(opts, "noise_method", None)
    if value is not None and value not in NOISE_METHODS:
        return "--noise_method %s: unknown estimator (one of %s)" % (value, ", ".join(NOISE_METHODS))
    return None


@contextlib.contextmanager
def noise_method_scope(method):
    """Inside the block, every noise_method=None means `method` (None: no change).  The one place a command line's
    --noise_method is applied: the commands run their work inside it.  The setting is the process's, as the
    reference's module constant is: the commands are single-threaded, and a library caller with threads passes
    noise_method to the functions instead."""
    if method is not None and method not in NOISE_METHODS:
        raise ValueError("noise method must be one of %s, not %r" % (", ".join(NOISE_METHODS), method))
    before = _IN_FORCE[0]
    if method is not None:
        _IN_FORCE[0] = method
    try:
        yield
    finally:
        _IN_FORCE[0] = before


def noise_method_in_force(noise_method=None):
    """The estimator a function called with noise_method should use: its argument, else the scope's, else None
    (stored values where there are any, 'PS' where something has to be measured)."""
    if noise_method is not None and noise_method not in NOISE_METHODS:
        raise ValueError("noise method must be one of %s, not %r" % (", ".join(NOISE_METHODS), noise_method))
    return noise_method if noise_method is not None else _IN_FORCE[0]


def noise_kwargs(noise_method=None):
    """Engine.channel_noise / channel_snrs keywords of the estimator in force: none at all for None."""
    method = noise_method_in_force(noise_method)
    return {} if method is None else {"method": method}


def measure(eng, data, noise_stds=True, SNRs=True, noise_method=None):
    """data.noise_stds and data.SNRs [nsub,npol,nchan] measured from its subints (NumPy or a device tensor) on the
    device: get_noise and get_SNR of every row, shaped like subints without its last axis.  A row of zeros has no
    noise to divide by: its S/N is NaN (scrunch.measured makes it 0).  noise_method: 'PS' or 'fit' (None: the
    scope's, else 'PS')."""
    sub = data.subints if hasattr(data.subints, "is_cuda") else np.asarray(data.subints)
    rows = sub.reshape(-1, sub.shape[-1])
    shape = tuple(int(n) for n in sub.shape[:-1])
    kw = noise_kwargs(noise_method)
    if noise_stds:
        data.noise_stds = eng.channel_noise(rows, **kw)[0].reshape(shape)
    if SNRs:
        data.SNRs = eng.channel_snrs(rows, **kw).reshape(shape)
    return data


def _completed(read, engine, noise_method=None):
    """(DataBunch, name) of what _read returned, the noise and S/N per channel that the archive lacks measured --
    or, with an estimator in force, all of them measured with it: stored values of another estimator would
    otherwise win silently."""
    data, name, has_snrs = read
    forced = noise_method_in_force(noise_method) is not None
    return measure(engine or default_engine(), data, forced or data.noise_stds is None,
                   forced or not has_snrs or data.SNRs is None, noise_method), name


def load_archive(datafile, engine=None, noise_method=None):
    """(DataBunch, name) of an archive ready to be worked on: load_bunch, with the noise and S/N per channel that the
    archive lacks measured on the device (noise_method given, or in force: all of them, with that estimator).
    RuntimeError: it cannot be loaded."""
    try:
        read = _read(datafile)
    except LOAD_ERRORS + (TypeError, KeyError) as err:
        raise RuntimeError("Cannot load_data(%s): %s" % (datafile, err))
    return _completed(read, engine, noise_method)


def load_archive_file(datafile, engine=None, noise_method=None):
    """load_archive for the commands that fit one file and report what reading it raised: NumPy is asked to open the
    file whatever its name, so one that is missing or is no .npz inside raises NumPy's own error, and only a file that
    NumPy can open but whose name is not an .npz's raises load_bunch's RuntimeError."""
    if not str(datafile).endswith(".npz"):
        with np.load(datafile, allow_pickle=True):
            pass
    return _completed(_read(datafile), engine, noise_method)


def good_channel_counts(datafile, tscrunch=False):
    """Good-channel counts of an archive's good subints, from its weights alone (the
    portraits are not read); [] for an archive get_TOAs cannot load.  tscrunch: of the one
    subint the archive is scrunched to -- the channels whose summed weight is positive."""
    if isinstance(datafile, dict):
        if tscrunch:
            n = int((np.nansum(np.asarray(datafile["weights"], dtype=np.float64), axis=0) > 0).sum())
            return [n] if n else []
        return [len(datafile["ok_ichans"][i]) for i in datafile["ok_isubs"]]
    if not str(datafile).endswith(".npz"):
        return []
    with np.load(datafile, allow_pickle=True) as z:
        if "weights" in z.files and tscrunch:
            counts = (np.nansum(np.atleast_2d(np.asarray(z["weights"], dtype=np.float64)), axis=0) > 0).sum()
        elif "weights" in z.files:
            counts = (np.asarray(z["weights"], dtype=np.float64) > 0).sum(axis=-1)
        else:               # (data_from_arrays: every channel of every subint is good)
            with z.zip.open("subints.npy") as f:
                version = np.lib.format.read_magic(f)
                read = np.lib.format.read_array_header_1_0 if version == (1, 0) else \
                    np.lib.format.read_array_header_2_0
                shape = read(f)[0]
            counts = np.full(1 if tscrunch else shape[0], shape[-2])
    return [int(c) for c in np.atleast_1d(counts) if c > 0]


# ---------------------------------------------------------------------------
# writing
# ---------------------------------------------------------------------------
def write_archive(outfile, fields):
    """Write `fields` -- a mapping from the names above to their values, those that are None left out -- as an .npz
    archive: epochs (MJD objects or floats) as float days, subints on the device brought to the host.  Returns the
    name of the file written."""
    fields = {k: v for k, v in fields.items() if v is not None}
    fields["epochs"] = np.array([e.in_days() if hasattr(e, "in_days") else float(e) for e in fields["epochs"]])
    if hasattr(fields["subints"], "is_cuda"):
        fields["subints"] = fields["subints"].cpu().numpy()
    np.savez(outfile, **fields)
    # (np.savez appends .npz to a name without it)
    return outfile if str(outfile).endswith(".npz") else str(outfile) + ".npz"
