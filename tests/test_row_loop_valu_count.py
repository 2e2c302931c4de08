"""The vector-ALU instructions of the headline transform kernel's row loop, counted in the code object's disassembly
(no GPU needed; tools/kernel_resources.py).

k_xspec_q1024<double, false> is bound by VALU issue: every wave64 VALU instruction, an f64 FMA or a v_mov alike, takes
an issue slot.  The f64 arithmetic is pinned -- its operation count fixes the bits of the Taylor sums -- and what
surrounds it (selects, moves, lane index arithmetic) is kept at what profiles/row_valu_budget.txt lists.  Counts are
static: one trip through the loop, both row tops and all seven slots of the unrolled slot loop counted once."""
import collections
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "k_xspec_q1024<double, false>"
# the build before the selects, moves and lane index arithmetic of the row loop were reworked
PARENT_VALU, PARENT_SELECTS_MOVES = 1222, 92


def _row_loop():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or shutil.which("objcopy") is None:
        pytest.skip("no llvm-objdump / objcopy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    loop = kernel_resources.row_loop(kernel=HEADLINE)
    # mnemonics without the encoding suffix: v_add_f64, v_fmac_f64 (_e32), v_cndmask_b32 (_e32 | _e64), v_mov_b32 (_e32 | _dpp)
    strip = lambda m: m[:-4] if m.endswith(("_e32", "_e64", "_dpp")) else m
    return collections.Counter(strip(t.split()[0]) for t in loop)


def test_f64_arithmetic_of_the_headline_row_loop_is_what_it_was():
    """No f64 addition, product or FMA added, removed or turned into another: 425 / 262 / 257 / 20."""
    c = _row_loop()
    f64 = {m: n for m, n in c.items() if m.startswith("v_") and "_f64" in m and
           m.startswith(("v_add_f64", "v_mul_f64", "v_fmac_f64", "v_fma_f64"))}
    assert f64 == {"v_add_f64": 425, "v_mul_f64": 262, "v_fmac_f64": 257, "v_fma_f64": 20}, f64


def test_selects_and_moves_of_the_headline_row_loop():
    """v_cndmask_b32 + v_mov_b32 (DPP forms included) + v_mov_b64: 92 before; 77 = 41 selects (28 of them the lambda = 0
    lane's in the slot loop), 32 v_mov_b32 (4 the quad exchanges' DPP moves, most of the rest in the once-per-chunk row
    top) and 4 v_mov_b64 (the partner value's hand-over from slot to slot, 14, is gone)."""
    c = _row_loop()
    n = c["v_cndmask_b32"] + c["v_mov_b32"] + c["v_mov_b64"]
    assert n < PARENT_SELECTS_MOVES
    assert n == 77, (n, c["v_cndmask_b32"], c["v_mov_b32"], c["v_mov_b64"])
    assert c["v_mul_lo_u32"] == 0, "a quarter-rate integer product in the row loop"
    assert c["ds_bpermute_b32"] == 0, "a lane exchange through the LDS unit in the row loop"


def test_static_valu_of_the_headline_row_loop():
    """Every v_ instruction of the loop: 1222 before, 1183 now."""
    c = _row_loop()
    valu = sum(n for m, n in c.items() if m.startswith("v_"))
    assert valu < PARENT_VALU
    assert valu == 1183, valu
