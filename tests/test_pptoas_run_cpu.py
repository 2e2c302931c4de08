"""get_TOAs(distributed=True) and the pptoas_run command line without a GPU: the shard
plan, the fit-flag carry between shards, rank 0's assembly over gloo with a stubbed device
stage, a failing rank, the option mapping, and the launcher's clean-up."""
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from pulseportraiture_amd import archive, pptoas, pptoas_run
from pulseportraiture_amd.dist import shard_range
from tests.gpu_support import kill_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "example.gmodel")


# ---------------------------------------------------------------------------
# shard plan and flag carry
# ---------------------------------------------------------------------------
def test_shard_plan_fits_every_good_subint_once():
    rng = np.random.default_rng(3)
    for narch in range(10):
        for nsub_max in range(14):
            noks = [int(v) for v in rng.integers(0, nsub_max + 1, size=narch)]
            for world in range(1, 5):
                seen = {}
                for rank in range(world):
                    mode, lo, hi = pptoas.shard_plan(narch, rank, world)
                    assert mode == ("archives" if narch >= world else "subints")
                    if mode == "subints":
                        assert (lo, hi) == (0, narch)
                    for ia in range(lo, hi):
                        j0, j1 = pptoas.shard_subints(mode, noks[ia], rank, world)
                        assert 0 <= j0 <= j1 <= noks[ia]
                        for j in range(j0, j1):
                            seen[(ia, j)] = seen.get((ia, j), 0) + 1
                want = {(ia, j): 1 for ia in range(narch) for j in range(noks[ia])}
                assert seen == want, (narch, noks, world)


def _flags_sharded(nchans, fit_flags, world):
    """Shard by shard with the carry-in each rank computes from what precedes it."""
    out = []
    for rank in range(world):
        lo, hi = shard_range(len(nchans), rank, world)
        carry = pptoas.subint_fit_flags(nchans[:lo], fit_flags)[1]
        out += pptoas.subint_fit_flags(nchans[lo:hi], fit_flags, carry)[0]
    return out


def test_flag_carry_between_shards_equals_the_whole_run():
    rng = np.random.default_rng(11)
    for fit_DM in (0, 1):
        for fit_GM in (0, 1):
            fit_flags = [1, fit_DM, fit_GM, 0, 0]
            for _ in range(200):
                n = int(rng.integers(0, 12))
                nchans = [int(v) for v in rng.choice([1, 2, 32], size=n)]
                whole = pptoas.subint_fit_flags(nchans, fit_flags)[0]
                for world in range(1, 5):
                    assert _flags_sharded(nchans, fit_flags, world) == whole
    # a two-channel subint first in its shard right after a one-channel one: phase only, from the carry
    nchans = [32, 1, 2, 32]
    whole = pptoas.subint_fit_flags(nchans, [1, 1, 1, 0, 0])[0]
    assert whole[2] == (1, 0, 0, 0, 0)
    assert shard_range(4, 1, 2)[0] == 2
    assert _flags_sharded(nchans, [1, 1, 1, 0, 0], 2) == whole
    # ... which a shard that ignored its carry-in would get wrong
    assert pptoas.subint_fit_flags(nchans[2:], [1, 1, 1, 0, 0])[0][0] == (1, 1, 0, 0, 0)


def test_good_channel_counts_read_weights_only(tmp_path):
    w = np.ones((4, 6))
    w[0, 1:] = 0
    w[1] = 0
    w[3, :4] = 0
    f = tmp_path / "a.npz"
    np.savez(f, subints=np.zeros((4, 1, 6, 8)), weights=w)
    assert archive.good_channel_counts(str(f)) == [1, 6, 2]
    g = tmp_path / "b.npz"
    np.savez(g, subints=np.zeros((3, 1, 5, 8)))
    assert archive.good_channel_counts(str(g)) == [5, 5, 5]
    assert archive.good_channel_counts(str(tmp_path / "x.fits")) == []


# ---------------------------------------------------------------------------
# assembly over gloo with a stubbed device stage
# ---------------------------------------------------------------------------
def _archives(spec):
    """DataBunches: spec is a list of per-archive lists of good-channel counts (0 = zapped subint)."""
    out = []
    nchan, nbin = 32, 16
    for ia, counts in enumerate(spec):
        nsub = len(counts)
        rng = np.random.default_rng(100 + ia)
        w = np.zeros((nsub, nchan))
        for i, c in enumerate(counts):
            w[i, np.sort(rng.choice(nchan, size=c, replace=False))] = 1.0
        freqs = np.linspace(1100.0, 1900.0, nchan)
        epochs = [pptoas.MJD(58000 + ia, 0.1 * i + 0.01) for i in range(nsub)]
        out.append(pptoas.data_from_arrays(
            rng.normal(size=(nsub, 1, nchan, nbin)), freqs, np.full(nsub, 0.003 + 1e-4 * ia), epochs,
            weights=w, noise_stds=np.ones((nsub, 1, nchan)), SNRs=np.full((nsub, 1, nchan), 10.0),
            DM=30.0 + ia, doppler_factors=1.0 + 1e-4 * np.arange(nsub), backend_delay=1e-6,
            subtimes=np.full(nsub, 10.0), filename="arch%d.fits" % ia))
    return out


class _StubGetTOAs(pptoas.GetTOAs):
    """get_TOAs with the device stage replaced: the 'fit' of a subint is a fixed function of
    (archive name, subint, flags), so its answer does not depend on the batch."""
    fail_rank = None

    def _engine(self, distributed):
        return None

    def _load_template(self, eng, slot, freqs_row, nbin, P, unscattered=False):
        pass

    def _archive_fit(self, eng, d, a, opt):
        if self.fail_rank is not None:
            import torch.distributed as tdist
            if tdist.is_initialized() and tdist.get_rank() == self.fail_rank:
                raise FloatingPointError("stub fit failed on purpose")
        nok, nchan = len(a.isubs), d.nchan
        res = dict(params=np.zeros((nok, 5)), param_errs=np.zeros((nok, 5)), cov=np.zeros((nok, 5, 5)),
                   nu_refs=np.zeros((nok, 3)), nfeval=np.zeros(nok, dtype=np.int32),
                   return_code=np.zeros(nok, dtype=np.int32), scales=np.zeros((nok, nchan)),
                   scale_errs=np.zeros((nok, nchan)), snr=np.zeros(nok), channel_snrs=np.zeros((nok, nchan)),
                   red_chi2=np.zeros(nok))
        for j, isub in enumerate(a.isubs):
            seed = [sum(map(ord, d.filename)), int(isub)] + list(a.flags_per[j])
            r = np.random.default_rng(seed)
            fl = np.asarray(a.flags_per[j], dtype=float)
            res["params"][j] = r.normal(size=5) * fl + [0, d.DM, 0, 0, 0]
            res["param_errs"][j] = r.uniform(1e-4, 1e-3, size=5) * fl
            m = r.normal(size=(5, 5))
            res["cov"][j] = m @ m.T
            res["nu_refs"][j] = r.uniform(1200, 1800, size=3)
            res["nfeval"][j], res["return_code"][j] = r.integers(3, 30), r.integers(0, 4)
            res["scales"][j] = r.uniform(0.5, 2, size=nchan)
            res["scale_errs"][j] = r.uniform(0.01, 0.1, size=nchan)
            res["snr"][j] = r.uniform(5, 50)
            res["channel_snrs"][j] = r.uniform(1, 5, size=nchan)
            res["red_chi2"][j] = r.uniform(0.8, 1.2)
        res["duration"] = 0.25 * nok
        means = {sl: np.linspace(0.1, 0.2, nchan) for sl in set(a.slots.values())}
        return res, res["duration"], means


_KW = dict(quiet=True, seed="device", fit_GM=True, print_flux=True, print_phase=True,
           nu_refs=(1500.0, None), addtnl_toa_flags={"pta": "X"})
_LISTS = ("obs", "doppler_fs", "nu0s", "nu_fits", "nu_refs", "ok_idatafiles", "ok_isubs", "MJDs", "Ps", "phis",
          "phi_errs", "TOA_errs", "DM0s", "DMs", "DM_errs", "DeltaDM_means", "DeltaDM_errs", "GMs", "GM_errs",
          "taus", "tau_errs", "alphas", "alpha_errs", "scales", "scale_errs", "snrs", "channel_snrs",
          "profile_fluxes", "profile_flux_errs", "fluxes", "flux_errs", "flux_freqs", "red_chi2s", "covariances",
          "nfevals", "rcs", "order")


def _snapshot(gt):
    out = {k: [np.asarray(v).tolist() if not isinstance(v, dict) else dict(v) for v in getattr(gt, k)]
           for k in _LISTS}
    out["TOAs"] = [[repr(t) for t in a] for a in gt.TOAs]
    out["epochs"] = [[repr(e) for e in a] for a in gt.epochs]
    out["fit_durations"] = list(gt.fit_durations)
    out["lines"] = [pptoas.toa_string(t) for t in gt.TOA_list]
    return out


def _worker(rank, world, port, spec, kw, fail_rank, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gt = _StubGetTOAs(_archives(spec), MODEL, quiet=True)
        gt.fail_rank = fail_rank
        try:
            gt.get_TOAs(distributed=True, **kw)
            q.put((rank, "ok", _snapshot(gt)))
        except Exception as err:
            q.put((rank, type(err).__name__, str(err)))
    finally:
        dist.destroy_process_group()


def _run_world(spec, world, kw, fail_rank=None, timeout=120):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, spec, kw, fail_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(world):
            rank, status, body = q.get(timeout=timeout)
            got[rank] = (status, body)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    return got


def _one_process(spec, kw):
    gt = _StubGetTOAs(_archives(spec), MODEL, quiet=True)
    gt.get_TOAs(**kw)
    return _snapshot(gt)


# archive mode (>= world archives; a skipped archive with no good subints among them) and subint mode
# (fewer archives than ranks; ragged shards, a slice that is empty on the last rank, one- and two-channel
# subints so that the flag carry crosses shard boundaries)
_ARCHIVE_SPEC = [[32, 1], [2, 32, 2, 32], [0, 0], [5, 2, 7], [1, 2, 3, 32, 0]]
_SUBINT_SPEC = [[32, 1, 2, 32, 2, 0, 32], [2]]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("spec", [_ARCHIVE_SPEC, _SUBINT_SPEC], ids=["archives", "subints"])
def test_sharded_assembly_over_gloo_equals_one_process(world, spec):
    want = _one_process(spec, _KW)
    got = _run_world(spec, world, _KW)
    status, body = got[0]
    assert status == "ok", body
    wd = want.pop("fit_durations")
    gd = body.pop("fit_durations")
    assert body == want
    np.testing.assert_allclose(gd, wd, rtol=1e-15)
    assert len(want["lines"]) > 0 and want["ok_idatafiles"] == [i for i, c in enumerate(spec) if any(c)]
    for r in range(1, world):
        status, other = got[r]
        assert status == "ok" and other["lines"] == [] and other["order"] == [] and other["DMs"] == []


@pytest.mark.timeout(120)
def test_a_failing_rank_ends_the_call_on_every_rank():
    t0 = time.time()
    got = _run_world(_ARCHIVE_SPEC, 2, _KW, fail_rank=1, timeout=100)
    assert time.time() - t0 < 100
    status, msg = got[0]
    assert status == "RuntimeError" and "rank 1" in msg and "stub fit failed on purpose" in msg
    assert got[1] == ("FloatingPointError", "stub fit failed on purpose")


def test_distributed_without_a_process_group_raises():
    gt = _StubGetTOAs(_archives([[32]]), MODEL, quiet=True)
    with pytest.raises(ValueError):
        gt.get_TOAs(distributed=True, **_KW)


def test_deltadm_mean_is_the_weighted_mean():
    DMs = np.array([30.1, 0.0, 30.3, 30.2])
    errs = np.array([0.1, 0.0, 0.2, 0.1])
    ok = np.array([0, 2, 3])
    m, e = pptoas.deltadm_mean(DMs, errs, 30.0, ok)
    w = errs[ok] ** -2
    want = np.sum(w * (DMs[ok] - 30.0)) / w.sum()
    assert abs(m - want) < 1e-15
    assert e > 0


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------
def _kw(*args):
    opts = pptoas_run.parser().parse_args(["-d", "x.npz", "-m", MODEL] + list(args))
    assert pptoas_run.refusal(opts) is None
    return pptoas_run.get_toas_kwargs(opts)


def test_cli_maps_options_to_get_TOAs_arguments():
    kw = _kw()
    assert kw["nu_refs"] is None and kw["DM0"] is None and kw["bary"] and kw["fit_DM"] and not kw["fit_GM"]
    assert kw["addtnl_toa_flags"] == {} and kw["scat_guess"] is None and kw["seed"] == "reference"
    assert _kw("--nu_ref", "inf")["nu_refs"] == (np.inf, None)
    assert _kw("--nu_ref", "1400")["nu_refs"] == (1400.0, None)
    assert _kw("--nu_tau", "1000")["nu_refs"] == (None, 1000.0)
    assert _kw("--nu_ref", "inf", "--nu_tau", "1000")["nu_refs"] == (np.inf, 1000.0)
    assert _kw("--flags", "pta,NANOGrav,version,0.1")["addtnl_toa_flags"] == {"pta": "NANOGrav", "version": "0.1"}
    assert _kw("--scat_guess", "1e-4,1500,-4")["scat_guess"] == [1e-4, 1500.0, -4.0]
    kw = _kw("--DM", "12.5", "--no_bary", "--fix_DM", "--fit_dt4", "--fit_scat", "--no_logscat", "--fix_alpha",
             "--print_phase", "--print_flux", "--print_parangle", "--quiet", "--seed", "device")
    assert kw["DM0"] == 12.5 and not kw["bary"] and not kw["fit_DM"] and kw["fit_GM"] and kw["fit_scat"]
    assert not kw["log10_tau"] and kw["fix_alpha"] and kw["print_phase"] and kw["print_flux"]
    assert kw["print_parangle"] and kw["quiet"] and kw["seed"] == "device"


@pytest.mark.parametrize("extra", [["--psrchive"], ["-T"], ["--showplot"], ["--saveplot"], ["-f", "princeton"],
                                   ["--errfile", "e.txt"], ["--narrowband", "--gpus", "2"]])
def test_cli_refuses_what_it_cannot_do(extra, tmp_path):
    r = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.pptoas_run", "-d", str(tmp_path / "x.npz"),
                        "-m", MODEL] + extra, capture_output=True, text=True, cwd=ROOT, timeout=60)
    assert r.returncode != 0 and "pptoas_run:" in r.stderr and r.stdout == ""


def test_one_DM_replaces_every_DM_by_its_archives_mean():
    gt = _StubGetTOAs(_archives([[32, 32], [32, 0, 32, 32]]), MODEL, quiet=True)
    gt.get_TOAs(**_KW)
    toas = pptoas_run.one_DM_toas(gt)
    assert len(toas) == 5
    for t, ia in zip(toas, [0, 0, 1, 1, 1]):
        assert t.DM == gt.DeltaDM_means[ia] + gt.DM0s[ia] and t.DM_error == gt.DeltaDM_errs[ia]
        assert " -DM_mean " in pptoas.toa_string(t)


# ---------------------------------------------------------------------------
# the launcher
# ---------------------------------------------------------------------------
_SLEEPER = """import os, sys, time
open(os.path.join(sys.argv[1], "rank%s.pid" % os.environ["RANK"]), "w").write(str(os.getpid()))
time.sleep(600)
"""


def _alive(pid):
    try:
        with open("/proc/%d/stat" % pid) as f:
            stat = f.read()
    except OSError:
        return False
    return stat[stat.rindex(")") + 2] != "Z"


@pytest.mark.timeout(180)
def test_launcher_leaves_no_rank_behind_after_sigterm(tmp_path):
    (tmp_path / "sleeper_mod.py").write_text(_SLEEPER)
    code = ("import sys; sys.path.insert(0, %r); from pulseportraiture_amd.pptoas_run import launch; "
            "sys.exit(launch(2, [%r], module='sleeper_mod', grace=5.0))" % (ROOT, str(tmp_path)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = str(tmp_path)
    p = subprocess.Popen([sys.executable, "-c", code], env=env, start_new_session=True)
    try:
        pids = []
        deadline = time.time() + 120
        while time.time() < deadline and len(pids) < 2:
            pids = [int((tmp_path / f).read_text()) for f in ("rank0.pid", "rank1.pid")
                    if (tmp_path / f).exists() and (tmp_path / f).read_text()]
            time.sleep(0.2)
        assert len(pids) == 2 and all(_alive(x) for x in pids)
        time.sleep(0.5)                  # (the launcher has seen the ranks)
        p.send_signal(signal.SIGTERM)
        rc = p.wait(timeout=60)
        assert rc != 0
        t_end = time.time() + 5.0
        while time.time() < t_end and any(_alive(x) for x in pids):
            time.sleep(0.1)
        assert not any(_alive(x) for x in pids)
    finally:
        if p.poll() is None:
            kill_group(p)


@pytest.mark.timeout(180)
def test_cli_with_two_ranks_exits_nonzero_when_the_ranks_fail(tmp_path):
    """`--gpus 2` starts its ranks itself; when they fail (here: no such metafile) the command ends
    with a non-zero code within its time limit and writes nothing."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "x.tim"
    r = subprocess.run([sys.executable, "-m", "pulseportraiture_amd.pptoas_run", "--gpus", "2", "--backend", "gloo",
                        "-d", str(tmp_path / "missing.txt"), "-m", MODEL, "-o", str(out)],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=150, start_new_session=True)
    assert r.returncode != 0 and "missing.txt" in r.stderr
    assert not out.exists()
