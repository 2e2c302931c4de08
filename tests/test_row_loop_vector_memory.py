"""What the row loop of the headline transform kernel asks of the CU's vector-memory path, read from the code object's
disassembly (no GPU needed; tools/kernel_resources.py).

The path returns in order across the CU's eight waves, so every small load in a row queues behind the row pieces the
other waves have in flight.  k_xspec_q1024<double, false> keeps the constants of a lane (stage twiddles, split twiddle)
in its own LDS, fetches phi_n through the scalar cache and sends the row's results out in one store that every lane
takes part in; the wait at the top of a row is then a counted one for the row's data alone."""
import collections
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "k_xspec_q1024<double, false>"


def _tools():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or shutil.which("objcopy") is None:
        pytest.skip("no llvm-objdump / objcopy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources


def _mnemonics(loop, prefix):
    return collections.Counter(t.split()[0] + (" nt" if t.endswith(" nt") else "") for t in loop if t.startswith(prefix))


def test_row_loop_of_the_headline_kernel_loads_the_row_and_nothing_per_row_besides():
    """Vector loads in the row loop: the 16 once-read (`nt`) pieces of the next row; the seven template values of the
    channel-change branch; and that branch's two 8-byte reads of the per-subint template table (row pointer, cut
    pointer: channel_lookup).  No twiddle (three more 16-byte loads before) and no phi_n (a third 8-byte load before):
    phi_n is the loop's one 8-byte scalar load."""
    kr = _tools()
    loop = kr.row_loop(kernel=HEADLINE)
    v = _mnemonics(loop, "global_load")
    assert v["global_load_dwordx4 nt"] == 16, v
    assert v["global_load_dwordx4"] == 7, v
    assert v["global_load_dwordx2"] == 2, v
    x2 = [t for t in loop if t.startswith("global_load_dwordx2")]
    # (both table reads take a 64-bit address from registers; phi_n was base + offset, `v, s[..]`)
    assert all(re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off", t) for t in x2), x2
    assert not any(t.startswith(("flat_", "buffer_", "scratch_")) for t in loop), "flat / buffer / scratch access in the row loop"
    s = _mnemonics(loop, "s_load")
    assert s["s_load_dwordx2"] == 1, s


def test_row_loop_of_the_headline_kernel_has_one_store_and_counted_waits_at_its_top():
    """One result store per row, and the waits for the row's data in front of the first butterflies are counted ones
    that end with vmcnt(1) -- the store of the previous row may still be under way -- not vmcnt(0)."""
    kr = _tools()
    loop = kr.row_loop(kernel=HEADLINE)
    stores = [t for t in loop if t.startswith("global_store")]
    assert len(stores) == 1 and stores[0].startswith("global_store_dwordx2"), stores
    # the f64 butterflies of stage 1 start with v_add_f64; the waits between the last scalar-path vmcnt(0) (ticket
    # draws, mask words: once per chunk) and the first ds_write of the transpose are the row's
    first_lds = next(i for i, t in enumerate(loop) if t.startswith("ds_write_b128"))
    first_add = next(i for i, t in enumerate(loop) if t.startswith("v_add_f64"))
    waits = [t for t in loop[first_add - 1:first_lds] if t.startswith("s_waitcnt vmcnt")]
    assert waits, "no wait for the row in front of stage 1"
    counts = [int(re.search(r"vmcnt\((\d+)\)", t).group(1)) for t in waits]
    assert min(counts) == 1 and counts == sorted(counts, reverse=True), counts


def test_headline_kernel_still_fits_eight_times_into_a_compute_unit():
    """256 registers (two waves per SIMD) and at most 19 456 B of LDS (eight workgroups in the CU's 160 KB), with the
    lane constants' tables inside that."""
    kr = _tools()
    md = kr.metadata(pat="k_xspec_q1024<double")
    assert set(md) == {HEADLINE, "k_xspec_q1024<double, true>"}, sorted(md)
    for k, d in md.items():
        assert d["vgpr"] + d["agpr"] <= 256, (k, d)
        assert d["lds"] <= 19456, (k, d)
    assert md[HEADLINE]["lds"] == 17408 + 2 * 64 * 16, md[HEADLINE]
