"""tests/gauss_refs.py against the true reference's fixtures (tests/golden/make_golden_ppgauss.py,
make_golden_ppgauss_join.py), and what tests/test_gpu_gauss_kernels.py relies on: that its input family carries power
at the highest harmonics, that a peak sample chosen the other way at a bin edge gives the same row, how far the f64
host construction (gaussfit.host_residuals) is from the long-double reference on every one of its cases, and that
gram_exact is the definition.  No GPU.

With PP_GAUSS_KERNELS_PARITY_OUT set, the host distances are written there as JSON (the GPU file writes them again
beside the device's deviations: profiles/gauss_kernels_parity.json)."""
import os

import numpy as np
import pytest

from tests import gauss_refs as gr
from tests.gpu_support import measured_writer

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MEASURED, _write_measured = measured_writer("PP_GAUSS_KERNELS_PARITY_OUT")
LD = np.longdouble


def _g(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _fixture_bar(data, want, errs):
    """tests/test_ppgauss_cpu.py::test_host_residuals_against_the_reference's: (1e-14 + 1e-13 |model|) / sigma_n plus one
    ulp of the row."""
    model = data[None] - want * errs[None, :, None]
    return (1e-14 + 1e-13 * np.abs(model)) / errs[None, :, None] + np.spacing(np.abs(want))


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_residuals_are_the_true_references_rows(nbin, code, scattered):
    """All 9 sets of the tag: the base and DC, tau, a loc, a loc slope, a wid, an amp, an amp index, the scattering index
    stepped."""
    g = _g("ppgauss_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    data, errs, freqs = g["n%d_data" % nbin], g["n%d_errs" % nbin], g["n%d_freqs" % nbin]
    want = g[tag + "_rows"].reshape(9, 3, nbin)
    got = gr.residuals(g[tag + "_sets"], data, errs, freqs, code, float(g["nu_ref"]))
    assert got.dtype == LD and got.shape == want.shape
    dev = np.abs(got - want.astype(LD)).astype(np.float64)
    bar = _fixture_bar(data, want, errs)
    assert np.all(dev <= bar), float((dev / bar).max())


@pytest.mark.parametrize("nbin", [64, 100])
@pytest.mark.parametrize("code", ["000", "011"])
@pytest.mark.parametrize("scattered", [0, 1])
def test_joined_residuals_are_the_true_references_rows(nbin, code, scattered):
    """The 7 sets of the tag (phase2, DM1, DM2, tau, a loc and the scattering index stepped) and the all-zero set, two
    bands and a channel in none, within the unjoined fixtures' bar."""
    g = _g("ppgauss_join_rows")
    tag = "n%d_c%s_t%d" % (nbin, code, scattered)
    data, errs, freqs = g["n%d_data" % nbin], g["errs"], g["freqs"]
    band = np.full(len(freqs), -1)
    band[g["band0"]], band[g["band1"]] = 0, 1
    vecs = np.vstack([g[tag + "_sets"], g[tag + "_zero_set"][None]])
    want = np.vstack([g[tag + "_rows"], g[tag + "_zero_rows"][None]]).reshape(len(vecs), len(freqs), nbin)
    sets, join = np.hstack([vecs[:, :-5], vecs[:, -1:]]), vecs[:, -5:-1].reshape(-1, 2, 2)
    got = gr.residuals(sets, data, errs, freqs, code, float(g["nu_ref"]), join, band, float(g["P"]))
    dev = np.abs(got - want.astype(LD)).astype(np.float64)
    bar = _fixture_bar(data, want, errs)
    assert np.all(dev <= bar), float((dev / bar).max())
    # (the all-zero set is the unjoined model)
    plain = gr.residuals(sets[-1], data, errs, freqs, code, float(g["nu_ref"]))
    assert np.array_equal(got[-1], plain[0])


@pytest.mark.parametrize("nbin", [8192, 4094])
@pytest.mark.parametrize("code", gr.CODES)
def test_the_family_carries_power_at_the_highest_harmonics(nbin, code):
    """In every channel of the unscattered row, |harmonic M - 1| and |harmonic M| are at least 1e-3 of |harmonic 1|: a
    wrong filter value, phasor or sign at high k or at k = M moves the row by far more than any bar."""
    import scipy.fft
    M = nbin // 2
    row = gr.portrait(gr.row_sets(nbin)[0], gr.FREQS, nbin, code, gr.NU_REF)[0]
    H = np.abs(scipy.fft.rfft(row, axis=-1))
    worst = float(min((H[:, M - 1] / H[:, 1]).min(), (H[:, M] / H[:, 1]).min()))
    print("nbin %d code %s: least |H_M-1|, |H_M| over |H_1| = %.3e" % (nbin, code, worst))
    assert worst >= 1e-3


@pytest.mark.parametrize("key", gr.all_cases(), ids=lambda k: gr.case(*k).name)
def test_every_case_decides_nothing_by_a_rounding(key):
    """peak_margin >= 1e-9 but where a loc parameter sits on a bin edge; and there, the other peak sample gives the same
    row: with every such component flipped, the (unscattered, unrotated) model moves by less than 1e-17 of its peak --
    four thousand times below the f64 spacing the kernels work in."""
    c = gr.case(*key)
    assert c.margins_ok()
    plain = c.sets.copy()
    plain[:, 1] = 0.0
    edge = gr.on_edge(c.sets, c.nbin)
    assert edge.any() or c.sets.shape[1] == 9          # (the one-component sets hold the narrow one alone)
    a = gr.portrait(plain, c.freqs, c.nbin, c.code, gr.NU_REF)
    b = gr.portrait(plain, c.freqs, c.nbin, c.code, gr.NU_REF, flip=edge)
    assert float(np.abs(a - b).max()) <= 1e-17 * float(np.abs(a).max())


def test_the_purposeful_components_sit_where_they_should():
    for nbin in gr.POW2_NBIN + gr.ANY_NBIN:
        loc = gr.family_comps(nbin)[:, 0] * nbin
        assert loc[gr.ON_EDGE] == np.rint(loc[gr.ON_EDGE])
        assert loc[gr.ON_CENTRE] - 0.5 == np.rint(loc[gr.ON_CENTRE] - 0.5)
        assert abs(loc[gr.NARROW] - np.floor(loc[gr.NARROW]) - 0.2) < 1e-9
        m = gr.peak_margin(gr.row_sets(nbin)[:1], gr.FREQS, nbin, "000", gr.NU_REF)[0]
        assert m[:, gr.ON_EDGE].max() < 1e-9 and m[:, gr.ON_CENTRE].min() > 0.1 and m[:, gr.NARROW].min() > 0.1


@pytest.mark.parametrize("key", gr.all_cases(), ids=lambda k: gr.case(*k).name)
def test_host_distance_of_every_case_is_recorded(key):
    """The f64 host construction's distance from the long-double reference, per channel, kept in the case for the GPU
    file's bar (the larger of the standing bar and ten times this).  The reference stands closer to the true rows than
    f64 can: the distance is at least finite and far below the data's noise."""
    c = gr.case(*key)
    r = c.reference()
    assert r["rows"].dtype == LD and r["model"].dtype == LD
    assert np.all(np.isfinite(r["host"])) and np.all(r["host"] < 1e-9)
    assert np.all(r["bar"] >= r["standing"]) and np.all(r["bar"] >= 10 * r["host"])
    MEASURED.setdefault("host_distance", {})[c.name] = dict(
        host_distance=float(r["host"].max()), of_standing_bar=float((r["host"] / r["standing"]).max()),
        widened=bool(np.any(10 * r["host"] > r["standing"])))
    print(c.name, "host distance %.3f of the standing bar" % float((r["host"] / r["standing"]).max()))


@pytest.mark.parametrize("nbin", [2048, 250])
def test_a_tiny_tau_moves_the_familys_rows_by_more_than_the_bar(nbin):
    """tau = 1e-12 rot shifts a row by tau times its slope, and the narrow component's slope is 8 / (0.5 bin): the true
    rows of tau = 1e-12 and of tau = 0 differ by thousands of bars at 2048 and at 250 bins.  So the GPU file cannot ask the
    device's tau = 1e-12 rows to lie within the bar of its tau = 0 rows; it asks that of the difference of the two
    deviations from their references (one bar, not the two that each deviation's own bar allows)."""
    c = gr.case("extreme", nbin, "000")
    r = c.reference()
    moved = np.abs(r["rows"][1] - r["rows"][2]).max(axis=-1).astype(np.float64)
    MEASURED.setdefault("tiny_tau_true_shift", {})[c.name] = dict(of_bar=float((moved / r["bar"]).max()))
    print(c.name, "true shift of tau = 1e-12: %.1f of the bar" % float((moved / r["bar"]).max()))
    assert float((moved / r["bar"]).max()) > 1e3


def test_gram_exact_is_the_definition():
    R_int, shifts = gr.integer_rows(4, 30, 11)
    assert np.all(R_int != 0) and np.abs(R_int).max() <= 512
    chi2, g, G = gr.gram_exact(R_int, shifts)
    V = [[int(v) for v in row] for row in R_int]
    dot = lambda p, q: sum(x * y for x, y in zip(p, q))     # noqa: E731
    assert int(chi2) == dot(V[0], V[0])
    assert [int(v) for v in g] == [dot(V[a], V[0]) for a in (1, 2, 3)]
    assert [[int(v) for v in row] for row in G] == [[dot(V[a], V[b]) for b in (1, 2, 3)] for a in (1, 2, 3)]
    # the f64 rows are exact, and the f64 definition on them gives these integers
    R, h = gr.gram_rows(R_int, shifts)
    from pulseportraiture_amd import gaussfit
    c2, gv, Gm = gaussfit.normal_equations(R, h)
    assert c2 == float(chi2) and np.array_equal(gv, g.astype(np.float64)) and np.array_equal(Gm, G.astype(np.float64))
    # ... in Python integers where int64 is not provably enough
    big = np.array([[2 ** 30, -2 ** 30, 3], [5, 7, -11]], dtype=np.int64)
    chi2, g, G = gr.gram_exact(big, [0])
    assert chi2 == 2 ** 61 + 9 and list(g) == [-2 * 2 ** 30 - 33] and G[0, 0] == 195
