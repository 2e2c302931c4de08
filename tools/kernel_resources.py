#!/usr/bin/env python3
"""Registers, spills, LDS and scratch of every kernel in libpptoas_hip.so, read from
the code object's metadata (no GPU needed):  python tools/kernel_resources.py [filter]

... and, from the disassembly, WHERE the scratch traffic of a kernel sits (loop_scratch): the metadata's
"spilled VGPRs" cannot tell the saves and restores around the one call to tail_work (executed once per
ticket a wave draws) from spills inside the row loop (executed per row, and a scratch load queues behind
the prefetched row like every other vector-memory access).  A loop is a backward branch; a scratch
instruction, or an SGPR spill to a VGPR lane (v_writelane / v_readlane), counts as "in a loop" when
some loop that contains NO call (s_swappc) spans it -- the phase loop around the call site is not one.
    python tools/kernel_resources.py --loops [filter]

... and whether two builds are the same kernels: symbols, resource notes and instruction text, kernel by kernel
    python tools/kernel_resources.py --compare A.so B.so"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def code_objects(so, tmp):
    """The gfx950 code objects of the library, one per translation unit (pp_toas.hip's first; pp_xspec_cu.hip's kernels
    carry their unit's namespace, pp_cu_unit::, in their names)."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
    blob, magic, cos = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", []
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    for i, (lo, hi) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        part, co = os.path.join(tmp, "fat%d.bin" % i), os.path.join(tmp, "dev%d.co" % i)
        with open(part, "wb") as f:
            f.write(blob[lo:hi])
        subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        cos.append(co)
    return cos


def _objdump(so, tmp):
    return "".join(subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                                  check=True).stdout for co in code_objects(so, tmp))


def loop_scratch(so=None, pat=""):
    """{kernel (demangled, short): dict(scratch_total, scratch_in_loops, lane_spills_in_loops, calls, loops)} for the
    kernels whose name contains `pat`."""
    so = so or os.path.join(ROOT, "pulseportraiture_amd", "csrc", "libpptoas_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        full = _objdump(so, tmp)
        blocks, cur = {}, None
        for ln in full.splitlines():
            m = re.match(r"^([0-9a-f]+) <([^>]+)>:", ln)
            if m:
                cur = m.group(2)
                blocks[cur] = [ln]
            elif cur is not None:
                blocks[cur].append(ln)
        want = [k for k in blocks if k.startswith("_ZN2pp")]
        dem = subprocess.run(["c++filt"], input="\n".join(want), capture_output=True, text=True).stdout.split("\n")
        out = {}
        for sym, name in zip(want, dem):
            short = re.sub(r"\(.*\)$", "", re.sub(r"^(void )?(pp::)?", "", name))
            if pat and pat not in short:
                continue
            if not short.startswith("k_"):
                continue
            dis = "\n".join(blocks[sym])
            ins = []          # (address, mnemonic, branch target or None)
            start = None
            for ln in dis.splitlines():
                m = re.match(r"^([0-9a-f]+) <", ln)
                if m:
                    start = int(m.group(1), 16)
                    continue
                m = re.match(r"^\s+(\S+).*//\s*([0-9A-Fa-f]+):", ln)
                if not m or start is None:
                    continue
                mnem, addr = m.group(1), int(m.group(2), 16)
                tgt = None
                if mnem.startswith("s_cbranch") or mnem == "s_branch":
                    t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", ln)
                    if t:
                        tgt = start + int(t.group(1), 16)
                    elif re.search(r"<[^>+]*>", ln):
                        tgt = start
                ins.append((addr, mnem, tgt))
            loops = [(t, a) for a, mn, t in ins if t is not None and t <= a]
            calls = [a for a, mn, t in ins if mn.startswith("s_swappc")]
            callfree = [(lo, hi) for lo, hi in loops if not any(lo <= cc <= hi for cc in calls)]
            inloop = lambda a: any(lo <= a <= hi for lo, hi in callfree)
            scr = [a for a, mn, t in ins if mn.startswith("scratch_")]
            lane = [a for a, mn, t in ins if mn.startswith("v_writelane") or mn.startswith("v_readlane")]
            out[short] = dict(scratch_total=len(scr), scratch_in_loops=sum(1 for a in scr if inloop(a)),
                              lane_spills_total=len(lane), lane_spills_in_loops=sum(1 for a in lane if inloop(a)),
                              calls=len(calls), loops=len(loops), instructions=len(ins))
        return out


def row_loop(so=None, kernel=""):
    """The instructions (text, operands included) of the ROW LOOP of the kernel whose short demangled name is `kernel`:
    the widest call-free loop that holds the 16 once-read (`nt`) loads of the next row (the compiler closes the loop with
    more than one backward branch, one of them into the middle of the row; the loop around the call to tail_work and the
    loops inside the row -- ticket draws, mask words -- are not it)."""
    so = so or os.path.join(ROOT, "pulseportraiture_amd", "csrc", "libpptoas_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        full = _objdump(so, tmp)
    syms = re.findall(r"^[0-9a-f]+ <(_ZN\d+pp[^>]+)>:", full, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    want = [sy for sy, name in zip(syms, dem) if re.sub(r"\(.*\)$", "", re.sub(r"^(void )?(pp::)?", "", name)) == kernel]
    if len(want) != 1:
        raise KeyError(kernel)
    ins, start, on = [], None, False          # (address, text, branch target or None)
    for ln in full.splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:", ln)
        if m:
            on = (m.group(2) == want[0])
            start = int(m.group(1), 16)
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
        if not on or not m:
            continue
        text, addr = m.group(1), int(m.group(2), 16)
        mnem, tgt = text.split()[0], None
        if mnem.startswith("s_cbranch") or mnem == "s_branch":
            t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", ln)
            tgt = start + int(t.group(1), 16) if t else start
        ins.append((addr, text, tgt))
    calls = [a for a, tx, t in ins if tx.startswith("s_swappc")]
    loops = [(lo, hi) for hi, tx, lo in ins if lo is not None and lo <= hi and not any(lo <= c <= hi for c in calls)]
    is_row = lambda tx: tx.startswith("global_load_dwordx") and tx.endswith(" nt")
    best = None
    for lo, hi in loops:
        if sum(1 for a, tx, t in ins if lo <= a <= hi and is_row(tx)) >= 16 and (best is None or hi - lo > best[1] - best[0]):
            best = (lo, hi)
    if best is None:
        raise ValueError("no row loop in " + kernel)
    return [tx for a, tx, t in ins if best[0] <= a <= best[1]]


def metadata(so=None, pat=""):
    """{kernel (demangled, short): dict(vgpr, agpr, sgpr, vspill, sspill, lds, scratch)} from the code object's notes."""
    so = so or os.path.join(ROOT, "pulseportraiture_amd", "csrc", "libpptoas_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        notes = "".join(subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True,
                                       check=True).stdout for co in code_objects(so, tmp))
    keys = dict(vgpr="vgpr_count", agpr="agpr_count", sgpr="sgpr_count", vspill="vgpr_spill_count",
                sspill="sgpr_spill_count", lds="group_segment_fixed_size", scratch="private_segment_fixed_size")
    rows = []
    for e in re.split(r"\n  - ", notes):
        m = re.search(r"\.name:\s+(\S+)", e)
        if m and ".vgpr_count" in e:
            rows.append((m.group(1), {k: int(re.search(r"\.%s:\s+(\d+)" % v, e).group(1)) for k, v in keys.items()}))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for (sym, d), n in zip(rows, names):
        n = re.sub(r"\(.*\)$", "", re.sub(r"^(void )?(pp::)?", "", n))
        if not pat or pat in n:
            out[n] = d
    return out


def disassembly(so):
    """{kernel symbol (mangled): [instruction text, ...]} of the code object, addresses stripped."""
    with tempfile.TemporaryDirectory() as tmp:
        full = _objdump(so, tmp)
    out, cur = {}, None
    for ln in full.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:", ln)
        if m and cur is not None:
            cur.append(m.group(1))
    return out


# the mnemonics whose counts may not change where the text of a kernel does: memory, LDS, f64 arithmetic, lane spills, calls
COUNTED = re.compile(r"^(global_|scratch_|ds_|v_\w+_f64|v_fma|v_readlane|v_writelane|s_swappc)")


def masked(text):
    """An instruction with register numbers and branch-target offsets masked."""
    text = re.sub(r"<[^>]*>", "<>", text)
    text = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", text)
    return re.sub(r"\b([vsa])\d+\b", r"\1", text)


def waves_per_simd(vgpr):
    return 4 if vgpr <= 128 else 3 if vgpr <= 168 else 2


def compare(so_a, so_b):
    """One line per kernel of B that differs from A's (symbols, resource notes, instruction text) and a summary.
    Returns the number of kernels that break the rules of an instruction-preserving refactor: a symbol gone or new,
    a resource note changed (VGPR / SGPR counts may move where nothing spills and the waves per SIMD stay), or a text
    that differs in more than order (counts of the COUNTED mnemonics unequal, total off by more than 0.5 %)."""
    import collections
    import difflib
    ma, mb = metadata(so_a), metadata(so_b)
    da, db = disassembly(so_a), disassembly(so_b)
    short = lambda n: re.sub(r"\(.*\)$", "", re.sub(r"^(void )?(pp::)?", "", n))
    syms = sorted(set(da) | set(db))
    names = dict(zip(syms, (short(n) for n in subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True,
                                                             text=True).stdout.split("\n"))))
    bad = differ = moved = 0
    for n in sorted(set(ma) ^ set(mb)):
        print("SYMBOL   %-70s only in %s" % (n[:70], "A" if n in ma else "B"))
        bad += 1
    for n in sorted(set(ma) & set(mb)):
        if ma[n] == mb[n]:
            continue
        ch = {k: (ma[n][k], mb[n][k]) for k in ma[n] if ma[n][k] != mb[n][k]}
        clean = all(d[k] == 0 for d in (ma[n], mb[n]) for k in ("vspill", "sspill", "scratch"))
        ok = clean and set(ch) <= {"vgpr", "sgpr"} and waves_per_simd(ma[n]["vgpr"]) == waves_per_simd(mb[n]["vgpr"])
        print("%-8s %-70s %s" % ("moved" if ok else "NOTES", n[:70], " ".join("%s %d->%d" % (k, x, y) for k, (x, y) in ch.items())))
        moved += ok
        bad += not ok
    for sy in sorted(set(da) & set(db)):
        ta, tb = da[sy], db[sy]
        if ta == tb:
            continue
        differ += 1
        xa, xb = [masked(t) for t in ta], [masked(t) for t in tb]
        nd = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in
                 difflib.SequenceMatcher(None, xa, xb, autojunk=False).get_opcodes() if tag != "equal")
        ca = collections.Counter(t.split()[0] for t in ta)
        cb = collections.Counter(t.split()[0] for t in tb)
        cnt = {k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]}
        ok = not any(COUNTED.match(k) for k in cnt) and abs(len(tb) - len(ta)) <= 0.005 * len(ta)
        print("%-8s %-70s %d -> %d instructions, %d masked lines differ; counts: %s" %
              ("text" if ok else "TEXT", names[sy][:70], len(ta), len(tb), nd,
               " ".join("%s %d->%d" % (k, x, y) for k, (x, y) in cnt.items()) or "equal"))
        bad += not ok
    for sy in sorted(set(da) ^ set(db)):
        if names[sy] not in ma and names[sy] not in mb:      # (a function that is no kernel: no notes of its own)
            print("SYMBOL   %-70s only in %s" % (names[sy][:70], "A" if sy in da else "B"))
            bad += 1
    print("%d symbols (%d kernels) in A, %d (%d) in B; resource notes: %d moved within the rule; instruction text: %d differ; "
          "%d break the rules" % (len(da), len(ma), len(db), len(mb), moved, differ, bad))
    return bad


def main():
    so = os.path.join(ROOT, "pulseportraiture_amd", "csrc", "libpptoas_hip.so")
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "--loops":
        res = loop_scratch(so, sys.argv[2] if len(sys.argv) > 2 else "")
        print("%-60s %8s %8s %8s %8s %6s %6s" % ("kernel", "scratch", "in-loop", "lanespl", "in-loop", "calls", "loops"))
        for k, v in sorted(res.items()):
            print("%-60s %8d %8d %8d %8d %6d %6d" % (k[:60], v["scratch_total"], v["scratch_in_loops"], v["lane_spills_total"],
                                                      v["lane_spills_in_loops"], v["calls"], v["loops"]))
        return
    pat = sys.argv[1] if len(sys.argv) > 1 else ""
    print("%-84s %5s %5s %5s %6s %6s %7s %7s" % ("kernel", "vgpr", "agpr", "sgpr", "vspill", "sspill", "lds", "scratch"))
    for n, d in metadata(so, pat).items():
        print("%-84s %5d %5d %5d %6d %6d %7d %7d" % (n[:84], d["vgpr"], d["agpr"], d["sgpr"], d["vspill"], d["sspill"],
                                                     d["lds"], d["scratch"]))


if __name__ == "__main__":
    main()
