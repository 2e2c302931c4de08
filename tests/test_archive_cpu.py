"""The archive module without a GPU: what write_archive writes reads back field for field, the loaders close the
file, refuse what is not an .npz and report a damaged one as their callers expect, and the module stands below the
rest of the package.  The fields are the module's own tuples: no list of them is kept here."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from pulseportraiture_amd import archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_ENGINE = object()        # (an archive that lacks nothing is not measured: the engine is never asked)


def _fields(seed=11):
    """Every field of the format for 2 subints x 2 pol x 4 channels x 16 bins with one zero weight, none of them at
    the value data_from_arrays would fill in."""
    rng = np.random.default_rng(seed)
    weights = np.ones((2, 4))
    weights[1, 2] = 0.0
    base = archive.data_from_arrays(rng.standard_normal((2, 2, 4, 16)), np.linspace(1200.0, 1500.0, 4), [0.003, 0.0031],
                                    [archive.MJD(56000, 0.25), archive.MJD(56001, 0.5)], weights)
    fields = {}
    for k in archive.ARRAY_FIELDS:
        v = base[k]
        if v is None:                                                   # one value per row
            v = rng.uniform(0.5, 2.0, size=base.subints.shape[:-1])
        elif isinstance(v, np.ndarray) and np.all(v == v.flat[0]):      # a default of zeros or ones
            v = rng.uniform(0.5, 2.0, size=v.shape)
        fields[k] = v
    for k in archive.SCALAR_FIELDS:
        v = base[k]
        fields[k] = k + "_x" if isinstance(v, str) else 1 if isinstance(v, int) else float(rng.uniform(1.0, 2.0))
    fields.update(zip(archive.EXTRA_FIELDS, (31.5, "Coherence")))
    return fields


def _days(v):
    return [e.in_days() for e in v]


def test_what_write_archive_writes_reads_back(tmp_path):
    fields = _fields()
    names = archive.ARRAY_FIELDS + archive.SCALAR_FIELDS + archive.EXTRA_FIELDS
    assert sorted(fields) == sorted(names) and not any(v is None for v in fields.values())
    name = archive.write_archive(str(tmp_path / "a"), fields)
    assert name == str(tmp_path / "a.npz") and archive.write_archive(name, dict(fields, weights=None)) == name
    with np.load(name, allow_pickle=True) as z:
        assert sorted(z.files) == sorted(set(names) - {"weights"})       # (None: left out)
    name = archive.write_archive(name, fields)
    with np.load(name, allow_pickle=True) as z:
        assert sorted(z.files) == sorted(names)
    for data, fname in (archive.load_bunch(name), archive.load_archive(name, NO_ENGINE)):
        assert fname == name and data.filename == name
        for k in archive.ARRAY_FIELDS:
            if hasattr(fields[k][0], "in_days"):
                assert _days(data[k]) == _days(fields[k]), k            # (float days: exact for these epochs)
            else:
                assert np.array_equal(data[k], fields[k]) and data[k].dtype == np.asarray(fields[k]).dtype, k
        for k in archive.SCALAR_FIELDS + archive.EXTRA_FIELDS:
            assert data[k] == fields[k] and getattr(data, k) == fields[k], k
        assert (data.nsub, data.npol, data.nchan, data.nbin) == (2, 2, 4, 16)
        assert list(data.ok_isubs) == [0, 1] and [list(c) for c in data.ok_ichans] == [[0, 1, 2, 3], [0, 1, 3]]
    # a bunch is handed back as it is
    assert archive.load_bunch(data)[0] is data and archive.load_archive(data, NO_ENGINE)[0] is data


def test_the_loaders_close_the_file(tmp_path, monkeypatch):
    fields = _fields()
    name = archive.write_archive(str(tmp_path / "a.npz"), fields)
    opened, np_load = [], np.load

    def recording_load(*args, **kwargs):
        opened.append(np_load(*args, **kwargs))
        return opened[-1]

    monkeypatch.setattr(np, "load", recording_load)
    first = archive.load_bunch(name)[0]
    archive.load_archive(name, NO_ENGINE)
    archive.good_channel_counts(name)
    monkeypatch.undo()
    assert len(opened) == 3
    for z in opened:                                                   # NpzFile.close was reached
        assert (z.zip is None or z.zip.fp is None) and (z.fid is None or z.fid.closed)
    assert np.array_equal(first.subints, fields["subints"])            # (read before the file was closed)
    other = archive.write_archive(str(tmp_path / "b.npz"), dict(fields, subints=2.0 * fields["subints"]))
    os.replace(other, name)
    with np.load(name) as z:
        assert np.array_equal(z["subints"], 2.0 * fields["subints"])
    assert np.array_equal(archive.load_bunch(name)[0].subints, 2.0 * fields["subints"])


def test_a_name_that_is_no_npz_is_refused_by_both_loaders(tmp_path):
    (tmp_path / "a.fits").write_bytes(b"SIMPLE  =                    T")
    for name in (str(tmp_path / "a.fits"), str(tmp_path / "absent.fits")):
        for load in (archive.load_bunch, lambda f: archive.load_archive(f, NO_ENGINE)):
            with pytest.raises(RuntimeError, match="PSRFITS archives need PSRCHIVE"):
                load(name)
        assert archive.good_channel_counts(name) == []


def test_a_truncated_npz(tmp_path):
    """load_archive reports it as the RuntimeError its callers skip on; load_bunch lets NumPy's own error through,
    which get_TOAs does not skip on and the ppzap noise method (LOAD_ERRORS) does."""
    whole = archive.write_archive(str(tmp_path / "whole.npz"), _fields())
    with open(whole, "rb") as f:
        content = f.read()
    name = str(tmp_path / "cut.npz")
    with open(name, "wb") as f:
        f.write(content[:len(content) // 2])
    with pytest.raises(RuntimeError, match=r"^Cannot load_data\(%s\): " % name.replace(".", r"\.")):
        archive.load_archive(name, NO_ENGINE)
    with pytest.raises(archive.LOAD_ERRORS) as err:
        archive.load_bunch(name)
    assert not isinstance(err.value, RuntimeError)
    with pytest.raises(type(err.value)):                                # the same error, as it was
        archive.load_archive_file(name, NO_ENGINE)
    # ... and a missing one
    with pytest.raises(OSError):
        archive.load_bunch(str(tmp_path / "absent.npz"))
    with pytest.raises(RuntimeError):
        archive.load_archive(str(tmp_path / "absent.npz"), NO_ENGINE)


def test_load_archive_file_asks_numpy_whatever_the_name(tmp_path):
    """What ppgauss_run.load_bunch and ppspline_run.load_portrait raised when they opened the file themselves first:
    NumPy's error for a file that is missing or is no .npz inside, the RuntimeError for one that is, under another
    name."""
    whole = archive.write_archive(str(tmp_path / "whole.npz"), _fields())
    assert np.array_equal(archive.load_archive_file(whole, NO_ENGINE)[0].subints, _fields()["subints"])
    for absent in (str(tmp_path / "absent.npz"), str(tmp_path / "absent.fits")):
        with pytest.raises(FileNotFoundError):
            archive.load_archive_file(absent, NO_ENGINE)
    (tmp_path / "a.fits").write_bytes(b"SIMPLE  =                    T")
    with pytest.raises(pickle.UnpicklingError):                         # (np.load's last resort)
        archive.load_archive_file(str(tmp_path / "a.fits"), NO_ENGINE)
    os.replace(whole, str(tmp_path / "whole.dat"))
    with pytest.raises(RuntimeError, match="PSRFITS archives need PSRCHIVE"):
        archive.load_archive_file(str(tmp_path / "whole.dat"), NO_ENGINE)


def test_a_joined_fit_reports_a_missing_band_in_one_line(tmp_path, capsys, monkeypatch):
    from pulseportraiture_amd import ppgauss_join_run
    monkeypatch.chdir(tmp_path)
    (tmp_path / "bands.txt").write_text("missing_band.fits\n")
    assert ppgauss_join_run.main(["-M", "bands.txt", "--autogauss", "0.05"]) == 2
    assert capsys.readouterr().err == ("ppgauss_join_run: [Errno 2] No such file or directory: "
                                       "'missing_band.fits'\n")


def test_an_archive_that_lacks_noise_or_snrs_is_measured_by_load_archive_only(tmp_path):
    class Engine(object):
        calls = []

        def channel_noise(self, rows):
            self.calls.append(("noise", rows.shape))
            return (np.full(len(rows), 3.0),)

        def channel_snrs(self, rows):
            self.calls.append(("snrs", rows.shape))
            return np.full(len(rows), 7.0)

    fields = _fields()
    bare = dict(fields, noise_stds=None, SNRs=None)
    name = archive.write_archive(str(tmp_path / "bare.npz"), bare)
    stored = archive.load_bunch(name)[0]
    assert stored.noise_stds is None and np.array_equal(stored.SNRs, np.ones((2, 2, 4)))    # (data_from_arrays)
    eng = Engine()
    data = archive.load_archive(name, eng)[0]
    assert eng.calls == [("noise", (16, 16)), ("snrs", (16, 16))]
    assert np.array_equal(data.noise_stds, np.full((2, 2, 4), 3.0))
    assert np.array_equal(data.SNRs, np.full((2, 2, 4), 7.0))
    # a bunch that came with S/N keeps them; its noise alone is measured
    del eng.calls[:]
    stored.SNRs = fields["SNRs"]
    assert archive.load_archive(stored, eng)[0] is stored and eng.calls == [("noise", (16, 16))]
    assert stored.SNRs is fields["SNRs"] and np.array_equal(stored.noise_stds, np.full((2, 2, 4), 3.0))


def test_metafiles(tmp_path):
    meta = tmp_path / "meta.txt"
    meta.write_text("a.npz\n\n  \n b.npz \n")
    assert archive.list_datafiles(str(meta)) == ["a.npz", "", "  ", " b.npz "]
    assert archive.named_datafiles(str(meta)) == ["a.npz", " b.npz "]
    name = archive.write_archive(str(tmp_path / "a.npz"), _fields())
    assert archive.list_datafiles(name) == [name] == archive.named_datafiles(name)
    assert archive.list_datafiles(str(tmp_path / "absent")) == [str(tmp_path / "absent")]


def _modules_loaded_by(module):
    code = "import sys, pulseportraiture_amd.%s; print('\\n'.join(sorted(sys.modules)))" % module
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, env=dict(os.environ, PYTHONPATH=ROOT),
                         stdout=subprocess.PIPE, universal_newlines=True).stdout.split()
    return [m[len("pulseportraiture_amd."):] for m in out if m.startswith("pulseportraiture_amd.")]


def test_the_archive_module_stands_below_the_rest():
    ours = _modules_loaded_by("archive")
    assert "archive" in ours and "pplib" in ours
    assert not [m for m in ours if m in ("pptoas", "ppalign", "scrunch", "engine") or m.endswith("_run")], ours


@pytest.mark.parametrize("module", ["ppalign", "scrunch", "pplib"])
def test_library_modules_load_no_command_line(module):
    ours = _modules_loaded_by(module)
    assert module in ours and not [m for m in ours if m.endswith("_run")], ours
