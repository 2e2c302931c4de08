"""ppalign without a GPU: the command line's options against the reference's parser (tests/golden/
ppalign_options.txt, written by make_golden_ppalign.py from the reference's OptionParser), its refusals, the channel
selection of the archive walk, and the output archive's round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_options_and_defaults_are_the_references():
    from pulseportraiture_amd.ppalign_run import parser
    kinds = {"_StoreAction": "store", "_StoreTrueAction": "store_true", "_StoreFalseAction": "store_false"}
    ours = {}
    for a in parser()._actions:
        if a.dest != "help":
            ours[",".join(a.option_strings)] = (a.dest, kinds[type(a).__name__], repr(a.default))
    theirs = {}
    for line in open(os.path.join(GOLDEN, "ppalign_options.txt")):
        flags, dest, action, default = line.rstrip("\n").split("\t")
        theirs[flags] = (dest, action, default)
    assert len(theirs) == 15
    assert ours == theirs


@pytest.mark.parametrize("flag,word", [("-T", "PSRCHIVE"), ("-P", "psradd"), ("-s", "psrsmooth")])
def test_refusals_exit_2_with_a_message(flag, word):
    p = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.ppalign_run", "-M", "list.txt", flag], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and p.stdout == ""
    assert p.stderr.startswith("ppalign_run: ") and word in p.stderr and len(p.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("args", [[], ["--niter", "0", "-M", "list.txt"]])
def test_without_a_metafile_or_iterations_the_banner_and_help(args):
    p = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.ppalign_run"] + args, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    assert p.stdout.startswith("\nppalign.py - Aligns and averages homogeneous archives by fitting DMs and phases\n")
    assert "--place" in p.stdout and "prof_SNR" in p.stdout and "stands in for psradd" in p.stdout


def test_channel_selection():
    """same_freqs: intersect1d of the subint's and the template's good channels; otherwise the nearest template channel
    of every good data channel (the first of two equally near, as np.argmin), ppalign.py:161-172 -- and of the data
    channels of one subint that share a template row only the last is added (NumPy's buffered +=, :204-208)."""
    from pulseportraiture_amd.ppalign import last_of_each_row, nearest_channels, select_channels
    from pulseportraiture_amd.pplib import DataBunch
    mf = np.array([1100.0, 1200.0, 1300.0, 1400.0])
    df = np.array([[1090.0, 1149.0, 1150.0, 1151.0, 1290.0, 1500.0]])
    d = DataBunch(freqs=df, ok_ichans=[np.array([0, 1, 2, 3, 5])])
    ich, mich = select_channels(d, 0, mf, np.array([0, 1, 3]), same_freqs=False)
    assert list(ich) == [0, 1, 2, 3, 5] and list(mich) == [0, 0, 0, 1, 3]
    assert list(nearest_channels(mf, df[0])) == [0, 0, 0, 1, 2, 3]
    assert list(last_of_each_row(ich, mich)) == [2, 3, 5]
    d = DataBunch(freqs=np.tile(mf, (1, 1)), ok_ichans=[np.array([0, 2, 3])])
    ich, mich = select_channels(d, 0, mf, np.array([0, 1, 3]), same_freqs=True)
    assert list(ich) == [0, 3] and list(mich) == [0, 3]


def test_gaussian_profile_is_the_references():
    from pulseportraiture_amd.pplib import gaussian_profile
    g = np.load(os.path.join(GOLDEN, "ppalign_guesses.npz"))
    assert np.array_equal(gaussian_profile(256, 0.5, 0.05), g["g005_256"])
    assert np.array_equal(gaussian_profile(1000, 0.5, 0.05), g["g005_1000"])
    assert np.array_equal(gaussian_profile(256, 0.3, 0.0001), g["place_delta_256"])
    assert not gaussian_profile(64, 0.5, 0.0).any()


def test_the_output_archive_round_trips(tmp_path):
    from pulseportraiture_amd.ppalign import write_archive
    from pulseportraiture_amd.archive import load_bunch as _load
    from pulseportraiture_amd.pptoas import data_from_arrays
    rng = np.random.default_rng(3)
    port = rng.standard_normal((4, 6, 32))
    totw = np.array([2.0, 0.0, 1.5, -1.0, 3.0, 0.0])
    guess = data_from_arrays(rng.standard_normal((2, 1, 6, 32)), np.linspace(1200.0, 1700.0, 6), [0.003, 0.0031],
                             [56000.25, 56001.5], DM=12.5, dmc=1, telescope="Arecibo", nu0=1450.0, bw=600.0)
    name = write_archive(str(tmp_path / "out"), port, totw, guess)
    assert name.endswith("out.npz")
    d, _ = _load(name)
    assert d.DM == 0.0 and d.dmc == 0 and d.telescope == "Arecibo" and d.nu0 == 1450.0 and d.bw == 600.0
    assert d.subints.shape == (1, 4, 6, 32) and np.array_equal(d.subints[0], port)
    assert list(d.weights[0]) == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    assert np.array_equal(d.freqs[0], guess.freqs[0]) and d.Ps[0] == 0.003 and d.epochs[0].in_days() == 56000.25
    assert list(d.ok_ichans[0]) == [0, 2, 4]


def test_channel_selection_against_the_golden():
    """The good channels and their nearest template channels of every subint of ppalign_mapped.npz, as the
    reference's expressions gave them (ppalign.py:166-172)."""
    from pulseportraiture_amd.ppalign import select_channels
    from pulseportraiture_amd.pplib import DataBunch
    g = np.load(os.path.join(GOLDEN, "ppalign_mapped.npz"))
    mf = g["guess.fits__freqs"][0]
    nsel = 0
    for name in ("m0.fits", "m1.fits"):
        w, freqs = g[name + "__weights"], g[name + "__freqs"]
        d = DataBunch(freqs=freqs, ok_ichans=[np.where(w[i] > 0)[0] for i in range(len(w))])
        for isub in range(len(w)):
            ich, mich = select_channels(d, isub, mf, np.arange(len(mf)), same_freqs=False)
            assert np.array_equal(ich, g["%s__ichans_%d" % (name, isub)])
            assert np.array_equal(mich, g["%s__model_ichans_%d" % (name, isub)])
            nsel += 1
            assert len(set(mich.tolist())) < len(mich)          # several data channels share a template row
    assert nsel == 4


def _lists(weights, chan_map, nchan_model):
    """pp_align_lists: (off, pairs[npairs, 2]) -- the library's host code only, no device."""
    import ctypes as C
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    w = np.ascontiguousarray(weights, dtype=np.float64)
    nsub, nchan = w.shape
    cm = None if chan_map is None else np.ascontiguousarray(chan_map, dtype=np.int32)
    off = np.full(nchan_model + 1, -7, dtype=np.int32)
    pairs = np.full(2 * nsub * nchan, -7, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    n = lib.pp_align_lists(nsub, nchan, nchan_model, w.ctypes.data_as(C.POINTER(C.c_double)),
                           None if cm is None else cm.ctypes.data_as(ip), off.ctypes.data_as(ip), pairs.ctypes.data_as(ip))
    if n < 0:
        return n, _lib.last_error()
    assert (pairs[2 * n:] == -7).all()
    return off, pairs[:2 * n].reshape(n, 2)


def test_the_contribution_lists():
    """The CSR lists pp_align_add walks: every accumulator row's (subint, data channel) pairs by subint, then channel;
    rows of weight 0 or NaN left out, negative weights kept; rows nothing lands on are empty; against a plain loop."""
    rng = np.random.default_rng(5)
    for nsub, nchan, nmodel, mapped in ((3, 7, 5, True), (1, 1, 1, False), (4, 6, 6, False), (5, 40, 3, True), (2, 9, 12, True)):
        w = rng.uniform(-1.0, 3.0, (nsub, nchan))
        w[rng.random((nsub, nchan)) < 0.2] = 0.0
        w[rng.random((nsub, nchan)) < 0.1] = np.nan
        w[0, 0] = -0.5
        cm = rng.integers(0, nmodel, (nsub, nchan)) if mapped else None
        if mapped and nmodel > 2:
            cm[cm == 1] = 0                     # a row nothing lands on
        off, pairs = _lists(w, cm, nmodel)
        want = [[] for _ in range(nmodel)]
        for i in range(nsub):
            for n in range(nchan):
                if w[i, n] != 0.0 and not np.isnan(w[i, n]):
                    want[n if cm is None else cm[i, n]].append((i, n))
        assert off[0] == 0 and list(np.diff(off)) == [len(r) for r in want]
        assert [tuple(p) for p in pairs] == [p for r in want for p in r]
        if mapped and nmodel > 2:
            assert off[1] == off[2]
    assert (0, 0) in [tuple(p) for p in _lists(np.array([[-0.5, 0.0, np.nan]]), None, 3)[1]]
    off, pairs = _lists(np.zeros((2, 3)), None, 3)
    assert list(off) == [0, 0, 0, 0] and len(pairs) == 0


def test_the_contribution_lists_refuse_a_map_outside_the_accumulator():
    for bad in (5, -1, 2 ** 30):
        rc, msg = _lists(np.ones((2, 3)), [[0, 1, 2], [4, bad, 0]], 5)
        assert rc == -1 and "chan_map[1][1]" in msg
    rc, msg = _lists(np.ones((2, 3)), None, 5)
    assert rc == -1 and "without a channel map" in msg
