"""get_TOAs(distributed=True) and `python -m pulseportraiture_amd.pptoas_run --gpus N` on the
GPU: ranks that share this box's GPU over gloo give the same bits as one rank, in archive
mode (whole archives per rank, with the fit-flag carry between them) and in subint mode
(the good subints of one archive sliced over the ranks).  Every child runs in a session of
its own under a time limit; a failure or a timeout ends the test."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

from tests.gpu_support import child_env, run_command, run_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(GOLDEN, "example.gmodel")

# every per-archive result list of GetTOAs (fit_durations aside: wall time)
LISTS = ("obs", "doppler_fs", "nu0s", "nu_fits", "nu_refs", "ok_idatafiles", "ok_isubs", "epochs", "MJDs", "Ps",
         "phis", "phi_errs", "TOAs", "TOA_errs", "DM0s", "DMs", "DM_errs", "DeltaDM_means", "DeltaDM_errs", "GMs",
         "GM_errs", "taus", "tau_errs", "alphas", "alpha_errs", "scales", "scale_errs", "snrs", "channel_snrs",
         "profile_fluxes", "profile_flux_errs", "fluxes", "flux_errs", "flux_freqs", "red_chi2s", "covariances",
         "nfevals", "rcs", "order")

# rank program of the API runs: rank 0 pickles its result lists and .tim lines
DRIVER = r'''
import json, os, pickle, sys
from datetime import timedelta
import torch.distributed as dist
from pulseportraiture_amd.pptoas import GetTOAs, toa_string
listfile, model, kwjson, out = sys.argv[1:5]
dist.init_process_group("gloo", timeout=timedelta(seconds=600))
try:
    gt = GetTOAs(listfile, model, quiet=True)
    gt.get_TOAs(distributed=True, **json.loads(kwjson))
    if dist.get_rank() == 0:
        lists = {k: getattr(gt, k) for k in %r}
        lists["fit_durations"] = gt.fit_durations
        lists["lines"] = [toa_string(t) for t in gt.TOA_list]
        with open(out, "wb") as f:
            pickle.dump(lists, f)
    else:
        assert gt.TOA_list == [] and gt.DMs == []
finally:
    dist.destroy_process_group()
''' % (LISTS,)


def _cli(args, timeout=420):
    return run_module("pptoas_run", args, ROOT, timeout)


def _api(tmp, nproc, listfile, kw, tag, timeout=420):
    """get_TOAs(distributed=True, **kw) on `nproc` ranks started by pptoas_run.launch."""
    (tmp / "pp_api_driver.py").write_text(DRIVER)
    out = tmp / ("lists_%s.pkl" % tag)
    code = ("import sys; from pulseportraiture_amd.pptoas_run import launch; "
            "sys.exit(launch(%d, sys.argv[1:], module='pp_api_driver'))" % nproc)
    run_command([sys.executable, "-c", code, str(listfile), MODEL, json.dumps(kw), str(out)], ROOT, timeout,
                child_env(str(tmp)))
    with open(out, "rb") as f:
        return pickle.load(f)


def _write_npz(path, g, ia):
    """Archive `ia` of an option golden as an .npz of DataBunch fields (epochs: pickled MJD objects)."""
    from pulseportraiture_amd.pptoas import MJD
    q = lambda k: g["in%d_%s" % (ia, k)]        # noqa: E731
    epochs = np.empty(len(q("epoch_days")), dtype=object)
    epochs[:] = [MJD(int(d), float(f)) for d, f in zip(q("epoch_days"), q("epoch_fracs"))]
    _save(path, subints=q("subints"), freqs=q("freqs"), Ps=q("Ps"), epochs=epochs, weights=q("weights"),
          noise_stds=q("noise_stds"), SNRs=q("SNRs"), DM=float(q("scal_DM")), doppler_factors=q("doppler_factors"),
          backend_delay=float(q("scal_backend_delay")), telescope=str(q("scal_telescope")),
          telescope_code=str(q("scal_telescope_code")), backend=str(q("scal_backend")),
          frontend=str(q("scal_frontend")), bw=float(q("scal_bw")), nu0=float(q("scal_nu0")),
          subtimes=q("subtimes"), source=str(q("scal_source")))


def _save(path, **fields):
    np.savez(path, **{k: (np.asarray(v) if not isinstance(v, np.ndarray) else v) for k, v in fields.items()})


def _listfile(tmp, paths, name="archives.txt"):
    f = tmp / name
    f.write_text("".join(str(p) + "\n" for p in paths))
    return f


def _canon(v):
    """Bit-exact canonical form of a result-list entry."""
    if hasattr(v, "intday"):
        return (v.intday(), np.float64(v.fracday()).tobytes())
    if isinstance(v, dict):
        return sorted((k, repr(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)) or (isinstance(v, np.ndarray) and v.dtype == object):
        return [_canon(x) for x in v]
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (float, np.floating)):
        return np.float64(v).tobytes()
    return repr(v)


def _assert_same_bits(a, b):
    for k in LISTS + ("lines",):
        assert _canon(a[k]) == _canon(b[k]), k
    assert len(a["fit_durations"]) == len(b["fit_durations"])


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.timeout(1800)
def test_gettoas_opt_two_archives_on_two_ranks_sharing_the_gpu(tmp_path):
    from tests.test_gpu_parity import _OPT_LISTS
    g = _golden("gettoas_opt_two_archives")
    paths = []
    for ia in range(int(g["narchives"])):
        paths.append(tmp_path / ("arch%d.npz" % ia))
        _write_npz(paths[-1], g, ia)
    lst = _listfile(tmp_path, paths)
    # the command line: --gpus 2 writes the bytes --gpus 1 writes
    t1, t2 = tmp_path / "one.tim", tmp_path / "two.tim"
    _cli(["--gpus", "1", "-d", str(lst), "-m", MODEL, "-o", str(t1), "--print_phase", "--quiet"])
    _cli(["--gpus", "2", "-d", str(lst), "-m", MODEL, "-o", str(t2), "--print_phase", "--quiet"])
    one = t1.read_bytes()
    assert one.count(b"\n") == 5 and one == t2.read_bytes()
    # the API: every result list equal bit for bit, and within the caller golden's tolerances
    kw = dict(print_phase=True, quiet=True)
    a1 = _api(tmp_path, 1, lst, kw, "one")
    a2 = _api(tmp_path, 2, lst, kw, "two")
    _assert_same_bits(a1, a2)
    assert [ln + "\n" for ln in a1["lines"]] == one.decode().splitlines(True)
    for ia in range(2):
        for fld, (rt, at) in _OPT_LISTS.items():
            got = a2[fld][ia]
            if fld in ("nu_fits", "nu_refs"):
                got = [[np.nan if x is None else float(x) for x in row] for row in got]
            got, want = np.asarray(got, dtype=np.float64), g["out_a%d_%s" % (ia, fld)]
            if fld == "covariances":
                dg = np.sqrt(np.abs(np.einsum("sii->si", want)))
                assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-8 * dg[:, :, None] * dg[:, None, :]
                              + 1e-300), fld
            elif rt == 0 and at == 0:
                np.testing.assert_array_equal(got, want, err_msg=fld)
            else:
                np.testing.assert_allclose(got, want, rtol=rt, atol=at, err_msg=fld)


def _fewchan_archives(tmp_path, split):
    """gettoas_opt_fewchan (good channels [32, 1, 2, 32, 2, 32]) as one archive, or split into [32, 1] and
    [2, 32, 2, 32]: then the second archive's first subint takes the flags left over from the first's last."""
    g = _golden("gettoas_opt_fewchan")
    full = tmp_path / "fewchan.npz"
    _write_npz(full, g, 0)
    if not split:
        return [full]
    z = dict(np.load(full, allow_pickle=True))
    out = []
    for k, rows in enumerate((slice(0, 2), slice(2, 6))):
        part = {n: (v[rows] if n in ("subints", "freqs", "Ps", "epochs", "weights", "noise_stds", "SNRs",
                                     "doppler_factors", "subtimes") else v) for n, v in z.items()}
        out.append(tmp_path / ("fewchan_%d.npz" % k))
        _save(out[-1], **part)
    w = [np.load(p)["weights"] for p in out]
    assert [list((x > 0).sum(1)) for x in w] == [[32, 1], [2, 32, 2, 32]]
    return out


@pytest.mark.timeout(1200)
def test_gettoas_opt_fewchan_in_archive_mode_carries_the_flags(tmp_path):
    lst = _listfile(tmp_path, _fewchan_archives(tmp_path, split=True))
    kw = dict(fit_GM=True, bary=False, quiet=True)
    a1 = _api(tmp_path, 1, lst, kw, "one")
    a2 = _api(tmp_path, 2, lst, kw, "two")
    _assert_same_bits(a1, a2)
    # (the two-channel subint after the one-channel one was fitted for phase only: no DM on its line)
    assert " -pp_dm " not in a2["lines"][2] and " -pp_dm " in a2["lines"][3]


@pytest.mark.timeout(1200)
def test_gettoas_opt_fewchan_in_subint_mode_over_three_ranks(tmp_path):
    lst = _listfile(tmp_path, _fewchan_archives(tmp_path, split=False))
    kw = dict(fit_GM=True, bary=False, quiet=True)
    a1 = _api(tmp_path, 1, lst, kw, "one")
    a3 = _api(tmp_path, 3, lst, kw, "three")
    _assert_same_bits(a1, a3)
    assert len(a3["lines"]) == 6


@pytest.mark.timeout(1800)
def test_subint_mode_on_a_64_subint_archive(tmp_path):
    """One synthetic archive of 64 subints x 512 channels x 1024 bins (tests/synth_host.py), the
    reference's seed, over 2 ranks: the same bits as one rank."""
    from pulseportraiture_amd.pptoas import MJD
    from tests import synth_host as sh
    nsub, C, B = 64, 512, 1024
    freqs, model = sh.model_portrait(C, B)
    subints = np.empty((nsub, 1, C, B))
    for i in range(nsub):
        subints[i, 0] = sh.make_inputs(C, B, seed=1000 + i, DM0=30.0, model=model)["data"]
    epochs = np.empty(nsub, dtype=object)
    epochs[:] = [MJD(58000, 0.001 * i) for i in range(nsub)]
    weights = np.ones((nsub, C))
    weights[5, ::3] = 0.0
    path = tmp_path / "synth64.npz"
    _save(path, subints=subints, freqs=np.broadcast_to(freqs, (nsub, C)), Ps=np.full(nsub, sh.P_EXAMPLE),
          epochs=epochs, weights=weights, noise_stds=np.full((nsub, 1, C), 0.05), DM=30.0,
          doppler_factors=1.0 + 1e-5 * np.arange(nsub))
    del subints
    lst = _listfile(tmp_path, [path])
    kw = dict(quiet=True)
    a1 = _api(tmp_path, 1, lst, kw, "one")
    a2 = _api(tmp_path, 2, lst, kw, "two")
    _assert_same_bits(a1, a2)
    assert len(a2["lines"]) == nsub


@pytest.mark.timeout(1200)
def test_pptoas_run_over_rccl_with_a_device_per_rank(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:          # (counting devices does not initialise the GPU)
        pytest.skip("needs two GPUs: RCCL wants a device per rank")
    g = _golden("gettoas_opt_two_archives")
    paths = []
    for ia in range(int(g["narchives"])):
        paths.append(tmp_path / ("arch%d.npz" % ia))
        _write_npz(paths[-1], g, ia)
    lst = _listfile(tmp_path, paths)
    t1, t2 = tmp_path / "one.tim", tmp_path / "two.tim"
    _cli(["--gpus", "1", "-d", str(lst), "-m", MODEL, "-o", str(t1), "--quiet"])
    _cli(["--gpus", "2", "--backend", "nccl", "-d", str(lst), "-m", MODEL, "-o", str(t2), "--quiet"])
    assert t1.read_bytes() == t2.read_bytes() and t1.read_bytes().count(b"\n") == 5
