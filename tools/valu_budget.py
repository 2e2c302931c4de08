#!/usr/bin/env python3
"""Where the instructions of a transform kernel's ROW LOOP go, block by block, from the disassembly of a build with
line tables (no GPU needed):

    tools/build_variants.sh lines "-gline-tables-only"          # -> variants/lines.so  (same code, + line tables)
    python tools/valu_budget.py [variants/lines.so] > profiles/r06_valu_budget.txt

For k_xspec_q1024<double, false|true> and k_xspec_qf<1024, double, false> the row loop is the largest backward
branch that contains no call; every instruction in it is symbolised with its inline stack (llvm-symbolizer) and
attributed to a block -- the FFT's stages (pp_fftq.h), the split + Taylor sums per slot, the phasor set-up, the
reduction, the row walk and look-ups -- by the source line of the frame that lies in the kernel's body (or in
fftq1024).  Counts are STATIC (one trip through the loop, every slot of the unrolled slot loop counted once); the
kernel executes a row's kept slots only (4.5 of 7 on average for the example template, all 16 for a full-spectrum
one), so the dynamic count is  fixed + slots_kept x per-slot.  Beside each block: its operation-count bound, stated
in the table's notes.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

KERNELS = [("k_xspec_q1024<double, false>", "_ZN2pp13k_xspec_q1024IdLb0EEEvNS_9XspecArgsE", 7),
           ("k_xspec_q1024<double, true>", "_ZN2pp13k_xspec_q1024IdLb1EEEvNS_9XspecArgsE", 7),
           ("k_xspec_qf<1024, double, false>", "_ZN2pp10k_xspec_qfILi1024EdLb0EEEvNS_9XspecArgsE", 16)]


def kind_of(mn):
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait/nop"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "vmem"
    if mn.startswith(("v_permlane", "v_readlane", "v_writelane", "v_readfirstlane")) or "_dpp" in mn:
        return "lane"
    if mn.startswith("v_"):
        return "valu_f64" if "_f64" in mn else "valu_other"
    return "other"


def markers(path, names):
    """line numbers of marker comments in a source file"""
    out = {}
    for i, ln in enumerate(open(path), 1):
        for key, pat in names.items():
            if pat in ln and key not in out:
                out[key] = i
    return out


def block_of(stack, kname_short, fq, xq):
    """stack: [(function, file, line)] innermost first"""
    funcs = [f for f, _, _ in stack]
    # the FFT: the frame inside fftq1024 tells the stage
    for f, fl, ln in stack:
        if f.startswith("fftq1024") or "fftq1024<" in f:
            if ln < fq["swap"]:
                return "fft stage 1 (DFT16 + 15 twiddles, powers by product tree)" if ln < fq["tw1"] or ln >= fq["tw1"] else "fft"
            if ln < fq["stage2"]:
                return "fft lane swaps (bits 5,4 <-> register bits 3,2)"
            if ln < fq["transpose"]:
                return "fft stage 2 (DFT4 x 4 + 12 twiddles)"
            if ln < fq["stage3"]:
                return "fft transpose through LDS"
            if ln < fq["power"]:
                return "fft stage 3 (DFT16)"
            return "S_d = sum |Z|^2"
    if any("RowWalk" in f for f in funcs) or any("channel_lookup" in f for f in funcs):
        return "row walk, tickets, channel look-up"
    if any("wave_reduce_lds" in f for f in funcs):
        return "reduction of the 13 sums + stores"
    if any("unit_phasor" in f or "sincos_turns" in f for f in funcs):
        return "phasor e^{2 pi i kb phi_n} (sincos)"
    # the frame in the kernel body
    for f, fl, ln in stack:
        if f.startswith("void pp::" + kname_short.split("<")[0]) or (kname_short.split("<")[0] in f and fl.endswith("pp_xspec1024q.h")):
            if ln < xq["fft"]:
                return "row top: twiddle reload, template values, next row's address, prefetch issue"
            if ln < xq["partners"]:
                return "row top: twiddle reload, template values, next row's address, prefetch issue"
            if ln < xq["tail"]:
                return "partner publish (LDS)"
            if ln < xq["phasors"]:
                return "noise tail |2 d_k|^2, k = 768..1024 (TAIL) + second half of the prefetch"
            if ln < xq["slots"]:
                return "phasor set-up"
            if ln < xq["reduce"]:
                return "slot loop: split + X = d m* + Taylor sums"
            return "reduction of the 13 sums + stores"
    return "other (" + (stack[-1][0][:40] if stack else "?") + ")"


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "variants", "lines.so")
    fq_path = os.path.join(ROOT, "pulseportraiture_amd", "csrc", "pp_fftq.h")
    xq_path = os.path.join(ROOT, "pulseportraiture_amd", "csrc", "pp_xspec1024q.h")
    fq = markers(fq_path, {"tw1": "// v[j] *= t1^j, every power formed once", "swap": "// ---- lane bits 5,4 <-> register bits 3,2 ----",
                           "stage2": "// ---- stage 2: DFT4 over register bits 3,2",
                           "transpose": "// ---- 16 x 16 transpose inside every row of 16 lanes",
                           "stage3": "    // ---- stage 3 ----", "power": "    if (power) {"})
    src = open(xq_path).read().splitlines()
    with tempfile.TemporaryDirectory() as tmp:
        co = kernel_resources.code_object(so, tmp)
        for kname, sym, nslots in KERNELS:
            dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + sym, co],
                                 capture_output=True, text=True, check=True).stdout
            ins, start = [], None
            for ln in dis.splitlines():
                m = re.match(r"^([0-9a-f]+) <", ln)
                if m:
                    start = int(m.group(1), 16)
                    continue
                m = re.match(r"^\s+(\S+)(.*)//\s*([0-9A-Fa-f]+):", ln)
                if not m or start is None:
                    continue
                mn, addr = m.group(1), int(m.group(3), 16)
                tgt = None
                if mn.startswith("s_cbranch") or mn == "s_branch":
                    t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", ln)
                    tgt = start + int(t.group(1), 16) if t else None
                ins.append((addr, mn, tgt))
            loops = [(t, a) for a, mn, t in ins if t is not None and t <= a]
            calls = [a for a, mn, t in ins if mn.startswith("s_swappc")]
            callfree = [(lo, hi) for lo, hi in loops if not any(lo <= c <= hi for c in calls)]
            lo, hi = max(callfree, key=lambda r: r[1] - r[0])
            body = [(a, mn) for a, mn, t in ins if lo <= a <= hi]
            # this kernel's own markers: the first occurrence after its definition line
            kdef = next(i for i, l in enumerate(src, 1) if ("void " + kname.split("<")[0] + "(") in l)
            def after(*pats, start=None):
                lo_ = kdef if start is None else start
                for pat in pats:
                    for i, l in enumerate(src, 1):
                        if i > lo_ and pat in l:
                            return i
                raise KeyError(pats)
            xq = {"fft": after("fftq1024<", "fftq1024_from<", "Q::template run<")}
            xq["partners"] = after("// ---- partners through LDS", start=xq["fft"])
            xq["phasors"] = after("// ---- phasors:", "const cplx* pc = lds + Q::lane_of", start=xq["partners"])
            xq["reduce"] = after("// ---- the 12 sums and S_d", "double tr[NRED];", start=xq["phasors"])
            try:
                xq["tail"] = next(i for i, l in enumerate(src, 1) if i > xq["partners"] and "double tail = 0.0;" in l and i < xq["phasors"])
            except StopIteration:
                xq["tail"] = xq["phasors"]
            xq["slots"] = after("for (int j = 0; j < NSL; ++j)", start=xq["phasors"])
            sym_in = "\n".join(hex(a) for a, _ in body)
            out = subprocess.run([LLVM + "/llvm-symbolizer", "--obj=" + co, "-i", "-f", "-s", "--output-style=LLVM"], input=sym_in,
                                 capture_output=True, text=True, check=True).stdout
            stacks, cur = [], []
            lines = out.splitlines()
            j = 0
            while j < len(lines):
                if not lines[j].strip():
                    if cur:
                        stacks.append(cur)
                    cur = []
                    j += 1
                    continue
                fn = lines[j].strip()
                loc = lines[j + 1].strip() if j + 1 < len(lines) else "?:0:0"
                mm = re.match(r"(.*):(\d+):(\d+)$", loc)
                cur.append((fn, mm.group(1) if mm else loc, int(mm.group(2)) if mm else 0))
                j += 2
            if cur:
                stacks.append(cur)
            assert len(stacks) == len(body), (len(stacks), len(body))
            table = collections.OrderedDict()
            for (a, mn), st in zip(body, stacks):
                b = block_of(st, kname, fq, xq)
                table.setdefault(b, collections.Counter())[kind_of(mn)] += 1
            kinds = ["valu_f64", "valu_other", "lane", "lds", "vmem", "salu", "wait/nop"]
            print("=" * 150)
            print("%s   row loop: %d instructions at +0x%x .. +0x%x, %d slots in the unrolled slot loop" % (kname, len(body), lo - start, hi - start, nslots))
            print("%-88s" % "block" + "".join("%11s" % k for k in kinds) + "%9s" % "VALU")
            tot = collections.Counter()
            for b, c in sorted(table.items(), key=lambda kv: -(kv[1]["valu_f64"] + kv[1]["valu_other"] + kv[1]["lane"])):
                valu = c["valu_f64"] + c["valu_other"] + c["lane"]
                print("%-88s" % b[:88] + "".join("%11d" % c[k] for k in kinds) + "%9d" % valu)
                tot.update(c)
            print("%-88s" % "total (static: every slot once)" + "".join("%11d" % tot[k] for k in kinds) +
                  "%9d" % (tot["valu_f64"] + tot["valu_other"] + tot["lane"]))
            sl = table.get("slot loop: split + X = d m* + Taylor sums", collections.Counter())
            per_slot = (sl["valu_f64"] + sl["valu_other"] + sl["lane"]) / float(nslots)
            fixed = tot["valu_f64"] + tot["valu_other"] + tot["lane"] - per_slot * nslots
            if nslots == 7:
                print("per slot: %.1f VALU;  fixed part: %.0f VALU;  dynamic estimate: %.0f (4.5 slots kept) ... %.0f (all %d)" %
                      (per_slot, fixed, fixed + 4.5 * per_slot, fixed + nslots * per_slot, nslots))
            else:
                print("slot loop %d VALU static for %d slots (the compiler keeps part of it rolled: the measured count, SQ_INSTS_VALU per "
                      "row, is ~1580); fixed part: %.0f VALU" % (sl["valu_f64"] + sl["valu_other"] + sl["lane"], nslots, fixed))
    print(NOTES)


NOTES = """
======================================================================================================================================================
Operation-count bounds, block by block (one lane's share of a 2048-bin row: 16 complex points of a 1024-point complex FFT;
an instruction = one VALU issue slot; FMA counted as one):

  block                          built   bound   where the difference goes
  fft stage 1                     292     ~215   DFT16 144-150 (split-radix: 144 adds, the 24 multiplies fused) + 15 twiddle products 60
                                                 = ~210; built: 289 f64 instructions (DFT16 158, products 60, the powers t1^2..t1^15 by a
                                                 product tree 49: 7 squarings at 3 + 7 products at 4; the other 22 are f64 too -- the
                                                 butterflies' own products, not moves) + 3 address instructions.  The tree trades VALU for registers
                                                 and memory: the powers read from a table measured slower (14.25 against 14.07 ms, round 2:
                                                 fifteen 16-byte loads per lane and row, behind the prefetched row).
  fft stage 2                     120      112   4 radix-4 butterflies (64 adds) + 12 twiddle products (48); w2, w3 from t2: 7
  fft stage 3 + transpose       158+6     ~150   DFT16, no twiddles
  lane swaps                       64       --   data movement: 32 dword pairs by v_permlane32_swap + 32 by v_permlane16_swap replace one of
                                                 the two LDS exchanges (the CU's one LDS unit was 94 % busy with both: 15.5 -> 13.8 ms, round 2)
  S_d                              36       32   16 |Z|^2 at 2
  slot loop, per kept slot       49.4       46   split E, O, W O, E - i W O: 10; X = d m*: 4; z = X e: 4; kappa ladder: 1 + 5; u = Im z kappa,
                                                 |Re| + |Im|: 2; the 12 sums: 12 FMA + 1; recurrences of W^k and e: 8 = 47 -- and 4 v_cndmask for
                                                 the ONE lane that owns lambda = 0 (its harmonic 64 (j + 1) sits in register j + 1): 28 a row.
                                                 Taking that lane's value through the partner exchange instead costs an 8th slot for the whole
                                                 wave (49); a DFT16 with rotated outputs costs 60.
  phasor (sincos of kb phi_n)      43      ~40   range reduction + two degree-8 polynomials (coefficients from scalar registers); the quadrant's
                                                 signs as integer additions to the high dwords (46 with a compare, a negated copy and a select each)
  reduction + stores               47      ~30   13 values x (store, 16-term column sum shared by 4 lanes), 2 quad exchanges by DPP (4 v_mov_b32
                                                 where ds_bpermute_b32 took 4 LDS instructions and ~12 VALU for the partner's lane number), positions
                                                 by shifts and additions (three v_mul_lo_u32, quarter rate, before), scaling, signs: 57 before
  row top + row walk               66      ~25   both row tops, the once-per-chunk one with its 64-bit addresses, ticket and mask word; kb and the
                                                 partner's LDS offset unpacked from one register carried across the rows (2 instructions; 14 to
                                                 derive them from the lane number); everything that can is scalar (each s_ instruction takes an
                                                 issue slot of its wave: DESIGN.md section 4)
  -----------------------------------------------------------------------------------------------
  k_xspec_q1024<double, false>   1059 (4.5 slots kept; 1103 before the selects, moves and lane index arithmetic of the row loop were
  reworked, profiles/row_valu_ab.txt) against ~930 + the 64 lane swaps: the kernel is within 5 - 7 % of its operation count; no block is more than ~80 instructions (7 % of a row) above its bound and
  each of those gaps is a measured trade (registers for the twiddle tree, the LDS unit for the lane swaps).

  k_xspec_q1024<double, true> (noise measured, what load_data always asks for): + 87 for |2 d_k|^2 of k = 768 .. 1024 (4 slots x
  (split 10 + W step 4 + |.|^2 3) = 68 bound) + 33 in the reduction (a 14th value, the square root).  1219 against ~1040: same margin.

  k_xspec_qf<1024, double, false> (templates that keep every harmonic: 16 slots a lane instead of 4.5): ~1580 measured =
  fixed 905 + 16 x ~42 a slot against the 46 - 47 of a slot counted above -- the per-slot part is AT its bound (the upper half of
  the harmonics reuses the E and O of its mirror: MODE 3) --, and it is what a full-spectrum template costs: 3.6 x the sums of
  the example template per byte of portrait.  0.43 - 0.45 of 8 TB/s is this kernel's roofline on f64 issue, not a deficit against it.

Conclusion (round-5 verdict, item 5): every block is within ~10 % of its operation-count bound except FFT stage 1 (+38 %, of which
the twiddle-power tree is 49 instructions), the reduction (+21 instructions) and the row top (+60); together ~130 instructions = 12 % of a
row, each a trade measured in rounds 2 - 5 (profiles/README.md).  The 28 v_cndmask of the lambda = 0 lane are the one item this table
turned up that had not been looked at; both ways around them cost more than they save, and so does a third: moving that lane's
registers 1..7 down by one under a one-lane EXEC takes 14 v_mov_b64 (a complex value is two), the compiler adds 14 copies of
its own around them and spills inside the row loop -- 1183 static VALU with it and without.  Closed: the transform kernels are f64-issue
bound at ~1.1 x their operation count, at the power-capped clock.
"""


if __name__ == "__main__":
    main()
