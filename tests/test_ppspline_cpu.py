"""The host side of ppspline, without a GPU: the command line's parser and refusals, the significance
decisions and the splprep stage against the true reference's outputs (tests/golden/ppspline_*.npz, from
make_golden_ppspline.py), the .spl round trip, and the model of zero components.  The device stages
are stood in for by the reference's own numbers from the fixture."""
import os
import pickle

import numpy as np
import pytest

from tests import ppspline_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FITTED = [n for n in pc.CASES if n != "64x256_mean_only"]


def _g(name):
    return np.load(os.path.join(GOLDEN, "ppspline_%s.npz" % name))


def _port(name):
    if name in pc.REGENERATED:
        port = pc.make_input(name)[0]
        assert pc.sha256(port) == str(_g(name)["input_sha256"])
        return port
    g = _g(name)
    return g["port"] if "port" in g.files else _g("64x256")["port"]


class GoldenEngine(object):
    """The engine's PCA stages answered from a fixture (the reference's numbers)."""

    def __init__(self, g, port):
        self.g, self.ok = g, g["weights"] > 0
        self.port = port[self.ok]

    def channel_noise(self, port, norm=None, weights=None):
        return self.g["noise_stds"][self.ok], np.ones(self.ok.sum())

    def pca_gram(self, port, weights):
        return self.g["mean_prof"], np.diag(np.arange(12.0, 0.0, -1.0)), 1.0

    def pca_basis(self, vecs, eigval):
        return self.g["eigvec"], self.g["stats"][:, :4]

    def pca_project(self, ieig):
        ev = self.g["eigvec"][:, ieig]
        proj = np.dot(self.port - self.g["mean_prof"], ev)
        return proj, np.dot(proj, ev.T) + self.g["mean_prof"]

    def spline_portrait(self, mean_prof, eigvec, tck, freqs, nbin=None):
        from pulseportraiture_amd.splmodel import gen_spline_portrait
        return gen_spline_portrait(mean_prof, freqs, eigvec, tck)


def _portrait(name):
    from pulseportraiture_amd.pptoas import data_from_arrays
    from pulseportraiture_amd.ppspline import DataPortrait
    g, port = _g(name), _port(name)
    data = data_from_arrays(port[None, None], g["freqs"], [0.003], [55000.0], weights=g["weights"][None],
                            noise_stds=g["noise_stds"][None, None], SNRs=g["SNRs"][None, None], bw=float(g["bw"]),
                            source="fake", filename=name + ".npz")
    return DataPortrait(data, quiet=True), g, port


def test_parser_defaults_are_the_references():
    from pulseportraiture_amd.ppspline_run import parser, refusal
    o = parser().parse_args(["-d", "avg.npz"])
    assert (o.datafile, o.modelfile, o.model_name, o.archive, o.norm) == ("avg.npz", None, None, None, "prof")
    assert (int(o.max_ncomp), float(o.snr_cutoff), float(o.rchi2_tol), int(o.k), float(o.sfac)) == (10, 150.0, 0.1, 3, 1.0)
    assert o.max_nbreak is None and not o.smooth and not o.make_plots and not o.quiet
    assert refusal(o, ["avg.npz"]) is None
    o = parser().parse_args("-d a.npz -o m.spl -l name -N rms -n 4 -S 99.5 -T 0.05 -k 5 -f 2.5 -t 7 --quiet".split())
    assert (o.modelfile, o.model_name, o.norm, o.max_ncomp, o.snr_cutoff, o.rchi2_tol, o.k, o.sfac, o.max_nbreak,
            o.quiet) == ("m.spl", "name", "rms", "4", "99.5", "0.05", "5", "2.5", "7", True)


@pytest.mark.parametrize("argv,word", [(["-s"], "PyWavelets"), (["-a", "out.fits"], "PSRCHIVE"), (["--plots"], "plots")])
def test_refused_options_exit_with_a_message(argv, word, capsys):
    from pulseportraiture_amd.ppspline_run import main
    assert main(["-d", "avg.npz"] + argv) == 2
    err = capsys.readouterr().err
    assert err.startswith("ppspline_run: ") and word in err


def test_a_metafile_of_several_archives_is_refused(tmp_path, capsys):
    from pulseportraiture_amd.ppspline_run import main
    meta = tmp_path / "bands.txt"
    meta.write_text("lband.npz\nsband.npz\n")
    assert main(["-d", str(meta)]) == 2
    assert "joining several bands" in capsys.readouterr().err


@pytest.mark.parametrize("name", list(pc.CASES))
def test_significance_decisions_from_the_references_statistics(name):
    from pulseportraiture_amd.ppspline import significant_eigvec
    g, kw = _g(name), pc.CASES[name][5]
    max_ncomp = kw.get("max_ncomp", 10)
    ieig, snrs = significant_eigvec(g["stats"][:, :4], pc.CASES[name][1], return_max=min(max_ncomp, 10),
                                    snr_cutoff=kw.get("snr_cutoff", 150.0))
    np.testing.assert_array_equal(ieig, g["ieig"])
    np.testing.assert_allclose(snrs, g["stats"][:len(snrs), 4], rtol=1e-14)


def test_the_crossings_test_and_the_limits_decide_as_the_reference():
    from pulseportraiture_amd.ppspline import significant_eigvec
    nbin = 1000                                     # threshold int(0.02 nbin) = 20 crossings
    unit = np.sqrt(nbin / 2.0)
    #        ev_snr:  500 (no check)  200, 19 crossings  200, 20 crossings  149 (cut)  450.1 (no check)  160, 3 crossings
    stats = np.array([[500 * unit, 1, 1, 99], [200 * unit, 1, 1, 19], [200 * unit, 1, 1, 20], [149 * unit, 1, 1, 0],
                      [450.1 * unit, 1, 1, 500], [160 * unit, 1, 1, 3]])
    np.testing.assert_array_equal(significant_eigvec(stats, nbin)[0], [0, 1, 4, 5])
    np.testing.assert_array_equal(significant_eigvec(stats, nbin, return_max=2)[0], [0, 1])
    np.testing.assert_array_equal(significant_eigvec(stats, nbin, check_max=2, return_max=1)[0], [0])
    np.testing.assert_array_equal(significant_eigvec(stats, nbin, check_crossings=False)[0], [0, 1, 2, 4, 5])
    assert len(significant_eigvec(stats, nbin, snr_cutoff=np.inf)[0]) == 0


@pytest.mark.parametrize("name", FITTED)
def test_splprep_stage_from_the_references_projections(name):
    from pulseportraiture_amd.ppspline import fit_spline_curve
    g, kw = _g(name), pc.CASES[name][5]
    ok = g["weights"] > 0
    snrs = g["SNRs"][ok]
    tck, u, fp, ier, msg = fit_spline_curve(g["proj_port"], snrs / np.sum(snrs), g["freqs"][ok], float(g["bw"]), snrs,
                                            g["noise_stds"][ok], k=kw.get("k", 3), sfac=kw.get("sfac", 1.0),
                                            max_nbreak=kw.get("max_nbreak"), quiet=True)
    np.testing.assert_array_equal(tck[0], g["t"])
    np.testing.assert_allclose(np.array(tck[1]), g["c"], rtol=1e-9, atol=1e-9 * np.abs(g["c"]).max())
    assert tck[2] == int(g["k"]) and ier == int(g["ier"])
    np.testing.assert_allclose(u, g["u"], rtol=1e-15)
    if kw.get("max_nbreak"):
        assert len(np.unique(tck[0])) <= kw["max_nbreak"]


@pytest.mark.parametrize("name", ["64x256", "48x1000", "64x256_mean_only"])
def test_make_spline_model_host_flow_and_the_spl_round_trip(name, tmp_path, capsys):
    from pulseportraiture_amd.splmodel import gen_spline_portrait, read_spline_model
    dp, g, port = _portrait(name)
    kw = dict(pc.CASES[name][5])
    dp.make_spline_model(smooth=False, engine=GoldenEngine(g, port), model_name="a name", **kw)
    out = capsys.readouterr().out
    np.testing.assert_array_equal(dp.ieig, g["ieig"])
    assert dp.ncomp == len(g["ieig"]) and dp.model_name == "a name"
    ok = g["weights"] > 0
    if dp.ncomp:
        np.testing.assert_array_equal(dp.tck[0], g["t"])
        np.testing.assert_allclose(dp.model[g["rows"]], g["model_rows"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(dp.modelx[g["rows_x"]], g["modelx_rows"], rtol=0, atol=1e-9)
        assert "uses %d basis profile components and %d breakpoints (%d B-splines with k=%d)." % (
            dp.ncomp, len(np.unique(g["t"])), len(g["t"]) - int(g["k"]) - 1, int(g["k"])) in out
    np.testing.assert_array_equal(dp.model_masked, dp.model * ok[:, None])
    path = str(tmp_path / "m.spl")
    dp.write_model(path, quiet=True)
    with open(path, "rb") as f:
        raw = f.read()
    assert raw[:2] == b"\x80\x02"                                   # pickle protocol 2
    content = pickle.loads(raw)
    assert content[:3] == ["a name", "fake", name + ".npz"] and content[4].shape == (port.shape[1], dp.ncomp)
    back = read_spline_model(path, quiet=True)
    np.testing.assert_array_equal(back[3], dp.mean_prof)
    np.testing.assert_array_equal(back[4], dp.eigvec[:, dp.ieig] if dp.ncomp else np.zeros((port.shape[1], 0)))
    np.testing.assert_array_equal(read_spline_model(path, freqs=g["freqs"], quiet=True)[1],
                                  gen_spline_portrait(dp.mean_prof, g["freqs"], content[4], dp.tck))


def test_zero_component_model_is_the_tiled_mean_profile(capsys):
    dp, g, port = _portrait("64x256_mean_only")
    dp.make_spline_model(smooth=False, snr_cutoff=np.inf, engine=GoldenEngine(g, port))
    assert dp.ncomp == 0 and len(dp.ieig) == 0 and dp.proj_port.shape == (64, 0)
    assert len(dp.tck[0]) == 0 and len(dp.tck[1]) == 0 and dp.tck[2] == 0 and len(dp.u) == 0
    assert dp.fp is None and dp.ier is None and dp.msg is None
    for m in (dp.model, dp.modelx, dp.reconst_port):
        np.testing.assert_array_equal(m, np.tile(g["mean_prof"], (64, 1)))
    assert dp.model_name == "64x256_mean_only.npz.spl"
    assert "uses 0 basis profile components; it returns the average profile." in capsys.readouterr().out


def test_smoothing_is_refused_with_the_reason():
    dp, g, port = _portrait("64x256")
    with pytest.raises(NotImplementedError, match="PyWavelets"):
        dp.make_spline_model(engine=GoldenEngine(g, port))          # (smooth=True is the reference's default)
