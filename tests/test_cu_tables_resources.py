"""Registers, LDS and the row loop of k_xspec_cu1024<double>, read from the code object (no GPU needed;
tools/kernel_resources.py).

The kernel is k_xspec_q1024<double, false>'s row without the two pieces of f64 work whose operands are the same in
every row: the product tree of the stage-1 twiddle powers and the steps of the split twiddle.  Those come from LDS
tables the CU's eight waves share, so the kernel must fit a CU exactly once: 512 threads at two waves per SIMD, and one
dynamic LDS block of no more than the CU's 160 KB."""
import collections
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the kernel is a translation unit of its own, pp_xspec_cu.hip, whose names carry the unit's namespace)
KERNEL = "pp_cu_unit::k_xspec_cu1024<double>"
OLD_VALU = 1183                      # k_xspec_q1024<double, false> (tests/test_row_loop_valu_count.py)
OLD_F64 = {"v_add_f64": 425, "v_mul_f64": 262, "v_fmac_f64": 257, "v_fma_f64": 20}
# What the tables take out of the loop, counted from the source (pp_fftq.h, pp_common.h):
#   a squaring of the tree, (fma(x, x, -y y), 2 x y):          x + x, two products, one FMA
#   a product cmul(a, b) = (fma(ax, bx, -ay by), fma(ax, by, ay bx)):   two products, two FMAs
# the tree forms t1^2 .. t1^15 with seven squarings (even powers) and seven products (odd powers); the unrolled slot
# loop steps the split twiddle six times (slots 1 .. 6), a product each.
SQUARING = {"v_add_f64": 1, "v_mul_f64": 2, "v_fmac_f64": 1}
PRODUCT = {"v_mul_f64": 2, "v_fmac_f64": 2}
REMOVED = {m: 7 * SQUARING.get(m, 0) + (7 + 6) * PRODUCT.get(m, 0) for m in OLD_F64}
NEW_F64 = {m: OLD_F64[m] - REMOVED[m] for m in OLD_F64}
assert NEW_F64 == {"v_add_f64": 418, "v_mul_f64": 222, "v_fmac_f64": 224, "v_fma_f64": 20}


def _tools():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or shutil.which("objcopy") is None:
        pytest.skip("no llvm-objdump / objcopy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources


@pytest.fixture(scope="module")
def loop():
    return _tools().row_loop(kernel=KERNEL)


def _counts(loop):
    strip = lambda m: m[:-4] if m.endswith(("_e32", "_e64", "_dpp")) else m
    return collections.Counter(strip(t.split()[0]) for t in loop)


def test_kernel_fits_a_compute_unit_once():
    """At most 256 registers (eight waves are two per SIMD), no static LDS beside the one dynamic block, and that block
    -- CU_LDS_BYTES of pp_xspec1024cu.h, which the host passes to the launch -- within the CU's 163 840 B."""
    md = _tools().metadata(pat="k_xspec_cu1024")
    assert set(md) == {KERNEL}, sorted(md)
    d = md[KERNEL]
    assert d["vgpr"] + d["agpr"] <= 256, d
    src = open(os.path.join(ROOT, "pulseportraiture_amd", "csrc", "pp_xspec1024cu.h")).read()
    m = re.search(r"static_assert\(CU_LDS_BYTES == (\d+) &&", src)
    assert m, "the size of the dynamic LDS block is stated in the source"
    assert d["lds"] + int(m.group(1)) <= 163840, (d["lds"], m.group(1))
    assert int(m.group(1)) == 8 * 17408 + (15 + 7) * 64 * 16


def test_row_loop_has_no_scratch_flat_or_buffer_access(loop):
    """A spill inside the row loop queues behind the prefetched row like every other vector-memory access."""
    assert not any(t.startswith(("scratch_", "flat_", "buffer_")) for t in loop), "scratch / flat / buffer access in the row loop"


def test_row_loop_has_fewer_vector_alu_instructions(loop):
    c = _counts(loop)
    valu = sum(n for m, n in c.items() if m.startswith("v_"))
    print("static VALU of the row loop: %d (k_xspec_q1024<double, false>: %d)" % (valu, OLD_VALU))
    assert valu < OLD_VALU, valu


def test_f64_arithmetic_is_the_old_row_without_the_tree_and_the_steps(loop):
    c = _counts(loop)
    f64 = {m: n for m, n in c.items() if m.startswith(("v_add_f64", "v_mul_f64", "v_fmac_f64", "v_fma_f64"))}
    assert f64 == NEW_F64, f64
