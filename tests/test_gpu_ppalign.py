"""The device-resident alignment accumulator (pp_align_begin / pp_align_add / pp_align_finish; Engine.align_begin /
align_add / align_finish) against a NumPy restatement of the reference's accumulation (ppalign.py:202-212), its
bitwise promises, and its refusals.

Bars.  The accumulator is held to what tests/test_gpu_parity.py holds the one-call kernel (pp_align_accumulate) to,
relative to the largest sample of the expected portrait: 5e-10 when a subint with DM = 15 at a few ms is among the
inputs (thousands of turns: NumPy's own k * phi rounds at ~1e-16 k phi), and without that subint the rounding-level
bar of the row length's route -- 2e-13 for the tuned power-of-two plans (test_align_accumulate_matches_oracle), 2e-12
for the chirp-z route of every other even length (test_align_accumulate_at_any_even_nbin_matches_oracle).  The bars
were fixed before the first run; every measured figure is printed beside its bar.

Where several data channels map to one accumulator row, every one of them is added (the CSR lists of the entry
point), which is what the restatement does with np.add.at."""
import numpy as np
import pytest

from tests.gpu_support import eng, run_module  # noqa: F401

pytestmark = pytest.mark.gpu

NBINS = [32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 100, 1000]
NSUB, NCHAN, NCHAN_MODEL = 3, 7, 5
MAPS = {
    # data channel -> accumulator row, per subint
    "identity": None,
    "many_to_one": np.array([[0, 0, 1, 2, 3, 4, 4], [0, 1, 1, 2, 3, 3, 4], [4, 3, 2, 2, 1, 0, 0]], dtype=np.int32),
    "row_never_hit": np.array([[0, 0, 1, 1, 2, 4, 4], [0, 1, 1, 2, 2, 4, 4], [0, 0, 0, 1, 2, 2, 4]], dtype=np.int32),
}


def _pow2(nbin):
    return nbin & (nbin - 1) == 0


def _inputs(nbin, npol, nchan, dtype, big_dm, seed=0):
    """nsub x npol x nchan x nbin rows: a Gaussian pulse per channel plus white noise, the polarisations scaled
    differently; per-subint phase, DM and reference frequency with DM = 0 and nu_ref = inf among them; a zero, a NaN
    and a negative weight."""
    rng = np.random.default_rng(1000 * nbin + 10 * npol + nchan + seed)
    x = (np.arange(nbin) + 0.5) / nbin
    freqs = np.linspace(1200.0, 1700.0, nchan)
    prof = np.exp(-0.5 * ((x[None, :] - 0.5 - 0.02 * np.arange(nchan)[:, None] / nchan) / 0.03) ** 2)
    ports = np.empty((NSUB, npol, nchan, nbin))
    for i in range(NSUB):
        for ip in range(npol):
            ports[i, ip] = prof * rng.uniform(0.5, 2.0) * (1.0 if ip == 0 else rng.uniform(-0.5, 0.5)) \
                + 0.1 * rng.standard_normal((nchan, nbin))
    ports = ports.astype(dtype)
    Ps = rng.uniform(0.002, 0.005, NSUB)
    phases = rng.uniform(-0.5, 0.5, NSUB)
    DMs = np.array([0.0, 15.0 if big_dm else 3e-3, -2e-3])
    nu_refs = np.array([1400.0, np.inf, 1234.5])
    w = rng.uniform(0.5, 3.0, (NSUB, nchan))
    w[0, 1] = 0.0
    w[1, 2] = np.nan
    w[2, 0] = -0.75
    return ports, freqs, Ps, phases, DMs, nu_refs, w


def _restated(ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, nchan_model, rot_phase):
    """ppalign.py:202-212 and :220-221 over the oracle's rotate_data."""
    from oracle import pptoas_oracle as orc
    nsub, npol, nchan, nbin = ports.shape
    aligned = np.zeros((npol, nchan_model, nbin))
    totw = np.zeros(nchan_model)
    for i in range(nsub):
        ichans = np.where((w[i] != 0.0) & ~np.isnan(w[i]))[0]
        model_ichans = ichans if cmap is None else cmap[i][ichans]
        weights = np.outer(w[i][ichans], np.ones(nbin))
        for ipol in range(npol):
            np.add.at(aligned[ipol], model_ichans, weights * orc.rotate_data(
                ports[i, ipol][ichans].astype(np.float64), phases[i], DMs[i], Ps[i], freqs[ichans], nu_refs[i]))
        np.add.at(totw, model_ichans, w[i][ichans])
    for ipol in range(npol):
        aligned[ipol, np.where(totw > 0)[0]] /= totw[np.where(totw > 0)[0], None]
    if rot_phase:
        aligned = orc.rotate_data(aligned, rot_phase)
    return aligned, totw


def _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, nchan_model, rot_phase=0.0, to_slot=-1):
    npol, nbin = (1 if len(ports.shape) == 3 else int(ports.shape[1])), int(ports.shape[-1])
    eng.align_begin(npol, nchan_model, nbin)
    eng.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, cmap)
    return eng.align_finish(rot_phase, to_slot)


@pytest.mark.parametrize("mapping", sorted(MAPS))
@pytest.mark.parametrize("nbin", NBINS)
def test_accumulator_matches_the_restated_reference(eng, nbin, mapping):
    cmap = MAPS[mapping]
    nchan = NCHAN_MODEL if cmap is None else NCHAN
    fine = 2e-13 if _pow2(nbin) else 2e-12
    for npol in (1, 4):
        for dtype in (np.float64, np.float32):
            for big_dm, bar in ((True, 5e-10), (False, fine)):
                args = _inputs(nbin, npol, nchan, dtype, big_dm)
                for rot in (0.0, 0.37):
                    al, tw = _accumulate(eng, *args, cmap, NCHAN_MODEL, rot)
                    oal, otw = _restated(*args, cmap, NCHAN_MODEL, rot)
                    dev = np.abs(al - oal).max() / np.abs(oal).max()
                    print("nbin %5d %-13s npol %d %-7s bigDM %d rot %.2f: dev %.3e bar %.1e" %
                          (nbin, mapping, npol, np.dtype(dtype).name, big_dm, rot, dev, bar))
                    np.testing.assert_allclose(tw, otw, rtol=1e-15, atol=0)
                    assert dev <= bar, (npol, dtype, big_dm, rot, dev, bar)
                    if mapping == "row_never_hit":
                        assert otw[3] == 0.0 and not al[:, 3].any()


@pytest.mark.parametrize("nbin", NBINS)
def test_accumulator_matches_the_one_call_kernel(eng, nbin):
    """One polarisation, identity map: the sum Engine.align_accumulate forms in one call, divided the same way."""
    fine = 2e-13 if _pow2(nbin) else 2e-12
    for dtype in (np.float64, np.float32):
        ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 1, NCHAN_MODEL, dtype, False)
        al, tw = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, None, NCHAN_MODEL)
        one, otw = eng.align_accumulate(ports[:, 0], freqs, Ps, phases, DMs, nu_refs, w)
        good = otw > 0
        one[good] /= otw[good, None]
        dev = np.abs(al[0] - one).max() / np.abs(one).max()
        print("nbin %5d %-7s: dev %.3e bar %.1e" % (nbin, np.dtype(dtype).name, dev, fine))
        np.testing.assert_allclose(tw, otw, rtol=1e-15, atol=0)
        assert dev <= fine


@pytest.mark.parametrize("nbin", [256, 1000])
def test_bits_do_not_depend_on_how_the_subints_are_cut(eng, nbin):
    """Three subints in one add, the same subints in three adds, and a device tensor: the same bytes."""
    import torch
    cmap = MAPS["many_to_one"]
    for dtype in (np.float64, np.float32):
        ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 4, NCHAN, dtype, False)
        al, tw = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, NCHAN_MODEL, 0.1)
        eng.align_begin(4, NCHAN_MODEL, nbin)
        for i in range(NSUB):
            eng.align_add(ports[i:i + 1], freqs, Ps[i:i + 1], phases[i:i + 1], DMs[i:i + 1], nu_refs[i:i + 1],
                          w[i:i + 1], cmap[i:i + 1])
        al3, tw3 = eng.align_finish(0.1)
        assert al3.tobytes() == al.tobytes() and tw3.tobytes() == tw.tobytes()
        ald, twd = _accumulate(eng, torch.from_numpy(ports).cuda(), freqs, Ps, phases, DMs, nu_refs, w, cmap,
                               NCHAN_MODEL, 0.1)
        assert ald.tobytes() == al.tobytes() and twd.tobytes() == tw.tobytes()


def test_a_host_input_cut_into_runs_gives_the_same_bits(eng):
    """A work-memory budget of a little more than one subint sends a host input through in several runs."""
    nbin = 256
    ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 4, NCHAN, np.float64, False)
    cmap = MAPS["row_never_hit"]
    al, tw = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, NCHAN_MODEL)
    with eng.options(max_work_bytes=1.4 * ports[0].nbytes):
        al2, tw2 = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, NCHAN_MODEL)
    assert al2.tobytes() == al.tobytes() and tw2.tobytes() == tw.tobytes()


@pytest.mark.parametrize("nbin", [256, 100])
def test_stokes_polarisation_0_equals_the_one_polarisation_run(eng, nbin):
    ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 4, NCHAN, np.float64, False)
    cmap = MAPS["many_to_one"]
    al4, tw4 = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, cmap, NCHAN_MODEL, 0.37)
    for ipol in (0, 2):
        al1, tw1 = _accumulate(eng, np.ascontiguousarray(ports[:, ipol]), freqs, Ps, phases, DMs, nu_refs, w, cmap,
                               NCHAN_MODEL, 0.37)
        assert al1[0].tobytes() == al4[ipol].tobytes() and tw1.tobytes() == tw4.tobytes()


@pytest.mark.parametrize("nbin", [256, 1000])
def test_finish_into_a_slot_equals_set_model_of_the_returned_portrait(eng, nbin):
    """finish(to_slot=0) leaves the template set_model of the returned polarisation 0 would: the slot's channel
    means and a fit against it give the same bytes.  Two finishes give the same bytes; a zero rot_phase changes none."""
    ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 4, NCHAN_MODEL, np.float64, False)
    al, tw = _accumulate(eng, ports, freqs, Ps, phases, DMs, nu_refs, w, None, NCHAN_MODEL, 0.0, to_slot=0)
    x0 = np.zeros((NSUB, 5))
    errs = np.full((NSUB, NCHAN_MODEL), 0.1)

    def fit():
        r = eng.fit_batch(np.ascontiguousarray(ports[:, 0]), freqs, Ps, x0, errs=errs, seed_ns=nbin)
        return eng.model_means(0, NCHAN_MODEL, nbin).tobytes() + r["params"].tobytes() + r["scales"].tobytes()

    from_device = fit()
    again, tw_again = eng.align_finish(0.0, to_slot=-1)
    assert again.tobytes() == al.tobytes() and tw_again.tobytes() == tw.tobytes()
    eng.set_model(al[0])
    assert fit() == from_device
    turned, _ = eng.align_finish(0.25)
    assert np.abs(turned - al).max() > 1e-3 * np.abs(al).max()
    back, _ = eng.align_finish(0.0)
    assert back.tobytes() == al.tobytes()


def test_misuse_is_refused_not_faulted():
    """add or finish before begin, another row length, and a channel map that points outside the accumulator (checked
    on the host; nothing is launched) raise EngineError; the accumulator is untouched by a refused call."""
    from pulseportraiture_amd.engine import Engine, EngineError
    e = Engine(0)
    try:
        nbin = 64
        ports, freqs, Ps, phases, DMs, nu_refs, w = _inputs(nbin, 1, NCHAN, np.float64, False)
        cmap = MAPS["many_to_one"]
        with pytest.raises(EngineError, match="begin"):
            e.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, cmap)
        with pytest.raises(EngineError, match="begin"):
            e.align_finish()
        e.align_begin(1, NCHAN_MODEL, nbin)
        e.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, cmap)
        al, tw = e.align_finish()
        with pytest.raises(EngineError, match="bin"):
            e.align_add(np.zeros((NSUB, 1, NCHAN, 128)), freqs, Ps, phases, DMs, nu_refs, w, cmap)
        with pytest.raises(EngineError, match="accumulator"):
            e.align_add(np.zeros((NSUB, 4, NCHAN, nbin)), freqs, Ps, phases, DMs, nu_refs, w, cmap)
        with pytest.raises(EngineError, match="channel map"):
            e.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, None)       # 7 channels onto 5 rows
        for bad in (NCHAN_MODEL, -1, 2 ** 30):
            cm = cmap.copy()
            cm[2, 6] = bad
            with pytest.raises(EngineError, match="chan_map"):
                e.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, cm)
        with pytest.raises(EngineError, match="nbin"):
            e.align_begin(1, NCHAN_MODEL, 1001)
        with pytest.raises(EngineError, match="begin"):      # (a refused begin leaves no accumulator)
            e.align_finish()
        e.align_begin(1, NCHAN_MODEL, nbin)
        e.align_add(ports, freqs, Ps, phases, DMs, nu_refs, w, cmap)
        al2, tw2 = e.align_finish()
        assert al2.tobytes() == al.tobytes() and tw2.tobytes() == tw.tobytes()
    finally:
        e.close()


# =====================================================================================================
# align_archives against the TRUE reference (tests/golden/ppalign_*.npz, from make_golden_ppalign.py)
# =====================================================================================================
import json      # noqa: E402
import os        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# golden file of the cases -> golden file of their archives
CASE_FILES = {"ppalign_same": "ppalign_same", "ppalign_same_norms": "ppalign_same", "ppalign_mapped": "ppalign_mapped",
              "ppalign_stokes": "ppalign_stokes", "ppalign_nbin1000": "ppalign_nbin1000"}
_G = {}


def _golden(name):
    if name not in _G:
        _G[name] = np.load(os.path.join(GOLDEN, name + ".npz"))
    return _G[name]


def _cases():
    out = []
    for fname in sorted(CASE_FILES):
        meta = json.loads(str(_golden(fname)["meta"]))["cases"]
        out += [(fname, c) for c in meta if not c.startswith("_")]
    return out


def _archive_fields(g, name):
    """The arguments of data_from_arrays for archive `name` of golden g, with what load_data measured."""
    sub = g[name + "__subints"].astype(np.float64)
    return dict(subints=sub, freqs=g[name + "__freqs"], Ps=g[name + "__Ps"], epochs=55000.0 + np.arange(len(sub)),
                weights=g[name + "__weights"], noise_stds=g[name + "__noise_stds"], SNRs=g[name + "__SNRs"],
                DM=0.0, dmc=0, nu0=1500.0, bw=800.0, filename=name)


def _bunch(g, name):
    from pulseportraiture_amd.pptoas import data_from_arrays
    d = data_from_arrays(**_archive_fields(g, name))
    d.prof_SNR = float(g[name + "__prof_SNR"])
    return d


def _datafiles(g):
    """The list align_archives walks: DataBunches, and the name of the archive that cannot be loaded."""
    return [_bunch(g, str(n)) if str(n) + "__subints" in g.files else str(n) for n in g["archive_names"]]


def _lines(text):
    """The iteration and skip messages of a run's stdout."""
    return [ln for ln in text.splitlines() if ln.startswith("Doing iteration") or "Skipping it" in ln]


@pytest.mark.parametrize("fname,case", _cases())
def test_align_archives_matches_the_reference(fname, case, capsys):
    """Every golden case at the tolerance the golden itself measured: atol = max(10 x ref_self_dev, 1e-12) x peak
    (ref_self_dev: the reference against itself on reordered input; it is below 3e-15 in every case, so the bar is
    1e-12 of the peak throughout).

    Measured on an MI355X: all 25 cases pass, 3e-16 ... 5e-14 of the peak (same channels, mapped channels, Stokes and
    nbin = 1000; every norm, rot_phase, place, niter 2, phase-only; the largest are the cases normalised by 'rms' and
    'max' after two iterations).  With the fit's default Taylor model the two nbin = 1000 cases sat at 7e-11 and 2e-9;
    align_archives fits with every evaluation a pass over the cross-spectrum (option "taylor" 0) for that reason."""
    from pulseportraiture_amd.ppalign import align_archives
    gc, g = _golden(fname), _golden(CASE_FILES[fname])
    meta = json.loads(str(gc["meta"]))["cases"][case]
    want, want_w = gc[case + "_amps"], gc[case + "_weights"]
    capsys.readouterr()
    got, totw = align_archives(_datafiles(g), _bunch(g, "guess.fits"), **meta["kwargs"])
    text = capsys.readouterr().out
    peak = np.abs(want).max()
    rel = max(10.0 * float(gc[case + "_self_dev"]), 1e-12)
    dev = np.abs(got - want).max() / peak
    with capsys.disabled():
        print("\n%-20s %-24s dev %.3e of the peak, bar %.1e" % (fname, case, dev, rel))
    assert got.shape == want.shape
    np.testing.assert_array_equal((totw > 0).astype(float), want_w)
    assert _lines(text) == _lines(meta["stdout"])
    assert dev <= rel, (dev, rel)


# =====================================================================================================
# the command line, in child processes
# =====================================================================================================
def _npz_fields(g, name):
    return {k: v for k, v in _archive_fields(g, name).items() if k != "filename"}


def _write_archives(g, tmp):
    """The golden's archives as .npz files and their metafile; returns the metafile's name."""
    names = []
    for n in g["archive_names"]:
        n = str(n)
        stem = n.replace(".fits", ".npz")
        names.append(stem)
        if n + "__subints" in g.files:
            np.savez(os.path.join(tmp, stem), prof_SNR=float(g[n + "__prof_SNR"]), **_npz_fields(g, n))
    np.savez(os.path.join(tmp, "init.npz"), **_npz_fields(g, "guess.fits"))
    with open(os.path.join(tmp, "list.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return "list.txt"


def test_ppalign_run_equals_the_golden(tmp_path):
    from pulseportraiture_amd.archive import load_bunch as _load
    g, gc = _golden("ppalign_same"), _golden("ppalign_same_norms")
    meta = _write_archives(g, str(tmp_path))
    out = run_module("ppalign_run", ["-M", meta, "-I", "init.npz", "--niter", "2", "-N", "prof", "-C", "10", "-o", "out.npz"],
                     tmp_path, 300)
    assert _lines(out) == ["Doing iteration 1...", "Doing iteration 2..."]
    d, _ = _load(str(tmp_path / "out.npz"))
    want = gc["norm_prof_niter2_amps"]
    rel = max(10.0 * float(gc["norm_prof_niter2_self_dev"]), 1e-12)
    dev = np.abs(d.subints[0] - want).max() / np.abs(want).max()
    print("ppalign_run: dev %.3e of the peak, bar %.1e" % (dev, rel))
    assert d.DM == 0.0 and d.dmc == 0 and d.subints.shape == (1,) + want.shape
    np.testing.assert_array_equal(d.weights[0], gc["norm_prof_niter2_weights"])
    assert dev <= rel


def test_ppalign_run_with_a_gaussian_guess_and_with_none(tmp_path):
    """-g 0.05 and neither -I nor -g run and write their default and named archives; with neither, the first template
    is the weighted mean of the dedispersed subints, formed here in NumPy."""
    from oracle import pptoas_oracle as orc
    from pulseportraiture_amd import ppalign
    from pulseportraiture_amd.archive import load_bunch as _load
    g = _golden("ppalign_mapped")
    meta = _write_archives(g, str(tmp_path))
    run_module("ppalign_run", ["-M", meta, "-g", "0.05", "-o", "gauss.npz"], tmp_path, 300)
    run_module("ppalign_run", ["-M", meta], tmp_path, 300)
    for name in ("gauss.npz", "list.txt.algnd.npz"):
        d, _ = _load(str(tmp_path / name))
        assert d.subints.shape == (1, 1, 24, 128) and np.isfinite(d.subints).all() and d.subints.any()
    # the stand-in for psradd -T: header DMs of 0.3 and -0.2 to dedisperse by, other channels to the nearest
    files = [_bunch(g, str(n)) for n in g["archive_names"]]
    files[0].DM, files[1].DM = 0.3, -0.2
    guess = ppalign.average_guess(files)
    mf = files[0].freqs[0]
    num, den = np.zeros((24, 128)), np.zeros(24)
    for d in files:
        for i in range(d.nsub):
            rot = orc.rotate_data(d.subints[i, 0], 0.0, d.DM, d.Ps[i], d.freqs[i], d.nu0)
            for n in range(d.nchan):
                m = int(np.argmin(abs(mf - d.freqs[i, n])))
                num[m] += d.weights[i, n] * rot[n]
                den[m] += d.weights[i, n]
    want = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], 0.0)
    np.testing.assert_allclose(guess.subints[0, 0], want, rtol=0, atol=2e-13 * np.abs(want).max())
    np.testing.assert_array_equal(guess.weights[0], (den > 0).astype(float))


def test_the_chain_from_archives_to_toas(tmp_path):
    """ppalign_run -> ppspline_run -d -> pptoas_run -m at 3 archives x 2 x 16 x 256: one TOA per subint, and the
    difference of the DMs injected into two archives comes back within 5 sigma of the reported errors."""
    from oracle import pptoas_oracle as orc
    from tests.synth_host import model_portrait, P_EXAMPLE
    rng = np.random.default_rng(7)
    freqs, model = model_portrait(16, 256)
    dDMs = [6e-4, -6e-4, 0.0]
    names = []
    for ia, dDM in enumerate(dDMs):
        sub = np.empty((2, 1, 16, 256))
        for i in range(2):
            sub[i, 0] = orc.rotate_data(model, -rng.uniform(-0.2, 0.2), -dDM, P_EXAMPLE, freqs, 1500.0) \
                + 0.02 * model.max() * rng.standard_normal(model.shape)
        names.append("arch%d.npz" % ia)
        np.savez(str(tmp_path / names[-1]), subints=sub, freqs=np.tile(freqs, (2, 1)), Ps=np.full(2, P_EXAMPLE),
                 epochs=56000.0 + ia + 0.01 * np.arange(2), weights=np.ones((2, 16)), DM=0.0, dmc=0, nu0=1500.0, bw=800.0)
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    run_module("ppalign_run", ["-M", "list.txt", "--niter", "2", "-o", "avg.npz"], tmp_path, 300)
    run_module("ppspline_run", ["-d", "avg.npz", "-o", "t.spl", "--quiet"], tmp_path, 300)
    out = run_module("pptoas_run", ["-d", "list.txt", "-m", "t.spl", "--quiet"], tmp_path, 300)
    toas = [ln for ln in out.splitlines() if "-pp_dm " in ln]
    assert len(toas) == 6, out

    def flag(ln, key):
        parts = ln.split()
        return float(parts[parts.index(key) + 1])

    dm = np.array([flag(ln, "-pp_dm") for ln in toas]).reshape(3, 2)
    dme = np.array([flag(ln, "-pp_dme") for ln in toas]).reshape(3, 2)
    diff = dm[0].mean() - dm[1].mean()
    sigma = 0.5 * np.sqrt((dme[0] ** 2).sum() + (dme[1] ** 2).sum())
    print("chain: DM difference %.3e (injected %.3e), sigma %.1e" % (diff, dDMs[0] - dDMs[1], sigma))
    assert abs(diff - (dDMs[0] - dDMs[1])) < 5.0 * sigma
