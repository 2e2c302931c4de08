"""ppzap on the GPU against the true reference (tests/golden/ppzap_*.npz, from make_golden_ppzap.py): the
channel noise and norms of every normalize_portrait method at nbin 256, 1000 (Bluestein) and 2048, f64 and
f32, host and device input (and nbin 4096 against NumPy); the clip's zap lists; the command line's bytes for both methods, on one rank and
on two ranks sharing the GPU over gloo; a subint's noise and zap row independent of its batch.  Every child
runs in a session of its own under a time limit."""
import os

import numpy as np
import pytest

from tests.gpu_support import default_eng, run_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODEL = os.path.join(GOLDEN, "example.gmodel")
G = np.load(os.path.join(GOLDEN, "ppzap_noise.npz"))
NORMS = ["none", "mean", "max", "prof", "rms", "abs"]
CLIPPED = ["none", "mean", "max", "prof", "abs"]     # (rms: every normalised noise is 1, the clip decides nothing)


def _ok(ia):
    isubs = G["a%d_ok_isubs" % ia]
    return G["a%d_subints" % ia].astype(np.float64)[isubs], G["a%d_weights" % ia][isubs]


def _norm(name):
    return None if name == "none" else name


@pytest.mark.parametrize("ia", [0, 1, 2])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("dtype,rtol", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_channel_noise_against_the_reference(ia, norm, dtype, rtol):
    ports, w = _ok(ia)
    noise, norms = default_eng().channel_noise(ports.astype(dtype), norm=_norm(norm), weights=w)
    np.testing.assert_allclose(noise, G["a%d_noise_%s" % (ia, norm)], rtol=rtol, atol=0)
    np.testing.assert_allclose(norms, G["a%d_norms_%s" % (ia, norm)], rtol=rtol, atol=0)


def _bunch(ia):
    from pulseportraiture_amd.pptoas import data_from_arrays
    x = G["a%d_subints" % ia].astype(np.float64)
    return data_from_arrays(x, G["a%d_freqs" % ia], G["a%d_Ps" % ia], np.zeros(len(x)),
                            weights=G["a%d_weights" % ia])


@pytest.mark.parametrize("ia", [0, 1, 2])
@pytest.mark.parametrize("norm", CLIPPED)
@pytest.mark.parametrize("nstd", [3, 5])
def test_zap_lists_against_the_reference(ia, norm, nstd):
    from pulseportraiture_amd.ppzap import get_zap_channels
    d = _bunch(ia)
    if norm != "none":          # (the command line's -N; without it the bunch has no noise: measured on the device)
        ports, w = _ok(ia)
        ns = np.zeros((d.nsub, 1, d.nchan))
        ns[d.ok_isubs, 0] = default_eng().channel_noise(ports, norm=norm, weights=w)[0]
        d.noise_stds = ns
    want = [[int(c) for c in np.nonzero(r)[0]] for r in G["a%d_zap_%s_%d" % (ia, norm, nstd)]]
    assert get_zap_channels(d, nstd=nstd) == want


@pytest.mark.parametrize("ia", [1, 2])
def test_a_subints_noise_and_zap_row_do_not_depend_on_its_batch(ia):
    eng = default_eng()
    x, w = _ok(ia)
    good = w > 0
    noise = eng.channel_noise(x)[0]
    for norm in (None, "prof"):
        n1, m1 = eng.channel_noise(x[2:3], norm=norm, weights=w[2:3])
        z1 = eng.zap_median(noise[2:3], good[2:3], 3.0)
        for nb in (7, 512):
            idx = np.arange(nb) % len(x)
            idx[nb // 2] = 2
            nb_, mb_ = eng.channel_noise(x[idx], norm=norm, weights=w[idx])
            assert nb_[nb // 2].tobytes() == n1[0].tobytes() and mb_[nb // 2].tobytes() == m1[0].tobytes()
            zb = eng.zap_median(noise[idx], good[idx], 3.0)
            assert zb[nb // 2].tobytes() == z1[0].tobytes()


@pytest.mark.parametrize("norm", [None, "mean", "prof"])
@pytest.mark.parametrize("ia", [0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_tensor_input_gives_the_host_bits(norm, ia, dtype):
    import torch
    ports, w = _ok(ia)
    ports = ports.astype(dtype)
    host = default_eng().channel_noise(ports, norm=norm, weights=w)
    dev = default_eng().channel_noise(torch.as_tensor(ports, device="cuda"), norm=norm, weights=w)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nbin_4096_several_waves_per_row(dtype):
    """nbin 4096 is the tuned length whose workgroup has several waves (their totals go through LDS): the noise
    and norms against NumPy's rfft, host and device input bit for bit, and a row's bits alone and in a batch."""
    import torch
    rng = np.random.default_rng(5)
    ph = (np.arange(4096) + 0.5) / 4096
    x = 40.0 * np.exp(-0.5 * ((ph - 0.4) / 0.01) ** 2) + rng.standard_normal((3, 8, 4096)) * rng.uniform(1, 9, (3, 8, 1))
    x[1, 3] = 0.0
    x = x.astype(dtype)
    eng = default_eng()
    p = np.abs(np.fft.rfft(x.astype(np.float64), axis=-1)) ** 2 / 4096
    want = np.sqrt(p[..., int(0.75 * 2049):].mean(axis=-1))
    for norm, ref in ((None, np.ones(x.shape[:2])), ("mean", x.astype(np.float64).mean(-1)),
                      ("max", x.astype(np.float64).max(-1)), ("abs", np.sqrt((x.astype(np.float64) ** 2).sum(-1))),
                      ("prof", None)):
        noise, norms = eng.channel_noise(x, norm=norm, weights=np.ones((3, 8)))
        if ref is not None:
            ref = np.where(x.any(-1), ref, 1.0)
            np.testing.assert_allclose(norms, ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(noise, want / np.abs(norms), rtol=1e-12, atol=0)
        dev = eng.channel_noise(torch.as_tensor(x, device="cuda"), norm=norm, weights=np.ones((3, 8)))
        assert noise.tobytes() == dev[0].tobytes() and norms.tobytes() == dev[1].tobytes()
        one = eng.channel_noise(x[1:2], norm=norm, weights=np.ones((1, 8)))
        assert one[0][0].tobytes() == noise[1].tobytes() and one[1][0].tobytes() == norms[1].tobytes()


def _paz(tmp):
    p = tmp / "paz.txt"
    return p.read_text() if p.exists() else ""


@pytest.mark.parametrize("k", range(6))
def test_noise_method_command_line_bytes(k, tmp_path):
    for ia in range(3):
        x = G["a%d_subints" % ia].astype(np.float64)
        np.savez(tmp_path / ("arch%d.npz" % ia), subints=x, freqs=G["a%d_freqs" % ia], Ps=G["a%d_Ps" % ia],
                 epochs=np.zeros(len(x)), weights=G["a%d_weights" % ia])
    (tmp_path / "list.txt").write_text("arch0.npz\narch1.npz\narch2.npz\n")
    out = run_module("ppzap_run", ["-d", "list.txt"] + [str(a) for a in G["cli%d_argv" % k]], tmp_path, 600)
    assert out == str(G["cli%d_stdout" % k])
    assert _paz(tmp_path) == str(G["cli%d_file" % k])


def _write_archive(path, g, pre):
    """An archive of a get_TOAs golden as an .npz of DataBunch fields (epochs: pickled MJD objects)."""
    from pulseportraiture_amd.pptoas import MJD
    q = lambda k: g[pre + k]        # noqa: E731
    epochs = np.empty(len(q("epoch_days")), dtype=object)
    epochs[:] = [MJD(int(d), float(f)) for d, f in zip(q("epoch_days"), q("epoch_fracs"))]
    fields = dict(subints=q("subints"), freqs=q("freqs"), Ps=q("Ps"), epochs=epochs, weights=q("weights"),
                  noise_stds=q("noise_stds"), SNRs=q("SNRs"), DM=float(q("scal_DM")),
                  doppler_factors=q("doppler_factors"), backend_delay=float(q("scal_backend_delay")),
                  telescope=str(q("scal_telescope")), telescope_code=str(q("scal_telescope_code")),
                  backend=str(q("scal_backend")), frontend=str(q("scal_frontend")), bw=float(q("scal_bw")),
                  nu0=float(q("scal_nu0")), subtimes=q("subtimes"), source=str(q("scal_source")))
    np.savez(path, **{k: np.asarray(v) for k, v in fields.items()})


def test_model_method_command_line_bytes_on_one_and_two_ranks(tmp_path):
    gm = np.load(os.path.join(GOLDEN, "ppzap_model.npz"))
    _write_archive(tmp_path / "zap.npz", np.load(os.path.join(GOLDEN, "gettoas_zap.npz")), "")
    _write_archive(tmp_path / "two0.npz", np.load(os.path.join(GOLDEN, "gettoas_opt_two_archives.npz")), "in0_")
    (tmp_path / "list.txt").write_text("zap.npz\ntwo0.npz\n")
    runs = [(0, ["--gpus", "1"]), (1, ["--gpus", "1"]), (0, ["--gpus", "2", "--backend", "gloo"]),
            (1, ["--gpus", "2", "--backend", "gloo"])]
    for k, ranks in runs:
        (tmp_path / "paz.txt").unlink(missing_ok=True)
        out = run_module("ppzap_run", ["-d", "list.txt", "-m", MODEL] + [str(a) for a in gm["cli%d_argv" % k]] + ranks,
                         tmp_path, 900)
        assert out == str(gm["cli%d_stdout" % k]), ranks
        assert _paz(tmp_path) == str(gm["cli%d_file" % k]), ranks
