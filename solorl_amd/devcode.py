"""Static inspection of the built gfx950 code object (no GPU needed): per-function counts of scratch (spill),
FLAT and global memory instructions.  Used by tests/test_abi.py to pin two properties that were each worth a
regression hunt on the GPU: the fp32 team-mode phases must not spill (101 spilled VGPRs in one phase
multiplied the kernel's HBM traffic by eight) and must not reach their context through FLAT instructions."""
import os
import re
import subprocess
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(lib_path, workdir):
    """gfx950 code objects of the library: its .hip_fatbin section holds one offload bundle per translation unit (the engine is built
    from several, solorl_amd/build.py), back to back -- split at the bundle magic, unbundle each."""
    fat = os.path.join(workdir, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib_path, os.path.join(workdir, "x.so")])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for k, a in enumerate(starts):
        part = os.path.join(workdir, "fat%d.bin" % k)
        open(part, "wb").write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = os.path.join(workdir, "dev%d.co" % k)
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        if os.path.getsize(co) > 0:
            out.append(co)
    return out


def disassemble(lib_path):
    """Disassembly of every code object, concatenated.  A function template instantiated in several translation units (the sweeps
    depend on the arithmetic type only, the units are split by type AND robot) appears once per unit: later copies are renamed
    `<name>.dupN` so that per-function statistics are never mixed (the copies are identical code)."""
    out, seen = [], {}
    with tempfile.TemporaryDirectory() as d:
        for co in _code_objects(lib_path, d):
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True).splitlines():
                m = re.match(r"^([0-9a-f]+) <([^>]+)>:", line)
                if m:
                    k = seen.get(m.group(2), 0)
                    seen[m.group(2)] = k + 1
                    if k:
                        line = "%s <%s.dup%d>:" % (m.group(1), m.group(2), k)
                out.append(line)
    return "\n".join(out)


def kernel_static_lds(lib_path):
    """{kernel name: static LDS bytes (.group_segment_fixed_size of the code object's metadata)}"""
    with tempfile.TemporaryDirectory() as d:
        notes = "\n".join(subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True) for co in _code_objects(lib_path, d))
    out, size = {}, None
    for line in notes.splitlines():       # per kernel the keys come in alphabetical order: the size line precedes the name line
        m = re.search(r"\.group_segment_fixed_size:\s*(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.search(r"^\s*\.name:\s*(\S+)", line)
        if m and size is not None:
            out[m.group(1)] = size
            size = None
    return out


def kernel_resources(lib_path):
    """{kernel name: {"vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", ...}} from the
    code objects' metadata (one record per kernel: a list item that starts with its first key)."""
    with tempfile.TemporaryDirectory() as d:
        notes = "\n".join(subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True) for co in _code_objects(lib_path, d))
    out, cur, col = {}, None, None
    for line in notes.splitlines():
        m = re.match(r"^(\s*-?\s*)\.([a-z_]+):\s*(\S*)\s*$", line)
        if not m:
            continue
        if m.group(1).strip() == "-" and m.group(2) == "agpr_count":      # (keys are sorted: a kernel's record starts here)
            cur, col = {}, len(m.group(1))
        if cur is None or len(m.group(1)) != col:                          # (the argument records below a kernel have a .name too)
            continue
        if m.group(2) == "name":
            out[m.group(3)] = cur
        elif m.group(3).isdigit():
            cur[m.group(2)] = int(m.group(3))
    return out


def function_stats(lib_path):
    """{mangled name: {"insts", "body", "barriers", "scratch", "flat", "global"}}.  `insts` counts every disassembled word up to the next
    symbol, the s_nop run that pads the function to the next one's alignment included (up to 63 for a kernel: it changes with the
    layout of the code object, not with the function); `body` stops at the function's last instruction that is not such a filler."""
    out, cur = {}, None
    for line in disassemble(lib_path).splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), dict(insts=0, body=0, barriers=0, scratch=0, flat=0, **{"global": 0})) if ".dup" not in m.group(1) else None
            continue
        if cur is None or "\t" not in line:
            continue
        op = line.split("\t")[1].strip().split(" ")[0] if len(line.split("\t")) > 1 else ""
        if not op:
            continue
        cur["insts"] += 1
        if op != "s_nop": cur["body"] = cur["insts"]
        if op == "s_barrier": cur["barriers"] += 1
        if op.startswith("scratch_"): cur["scratch"] += 1
        elif op.startswith("flat_"): cur["flat"] += 1
        elif op.startswith("global_"): cur["global"] += 1
    return out


def _function_rows(text, name_filter):
    """{mangled name: [(byte offset in the function, instruction text)]} of the functions whose name contains `name_filter`"""
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is not None and "\t" in line:
            cur.append(line)
    out = {}
    off_re = re.compile(r"//\s*([0-9A-Fa-f]+):")
    for name, lines in funcs.items():
        if name_filter not in name or not lines or ".dup" in name:
            continue
        base = int(off_re.search(lines[0]).group(1), 16)
        rows = []
        for l in lines:
            mo = off_re.search(l)
            if mo:
                rows.append((int(mo.group(1), 16) - base, l.split("\t")[1].strip() if len(l.split("\t")) > 1 else ""))
        out[name] = rows
    return out


def _branch_target(op):
    if not op.startswith(("s_cbranch", "s_branch")):
        return None
    mt = re.search(r"<[^>]*\+0x([0-9a-f]+)>", op)
    return int(mt.group(1), 16) if mt else None


def loop_stats(lib_path, name_filter, text=None):
    """For every function whose mangled name contains `name_filter`: the widest backward branch (spanning more than
    200 bytes) is taken as THE loop; returns {name: {"insts", "scratch", "insts_in_loop", "s_nop_in_loop", "scratch_in_loop",
    "valu_in_loop", "lds_in_loop", ..., "ops_in_loop": [mnemonics of the span, in address order]}}.  Used to pin that the PGS sweep loops touch no memory at all (callee-saved registers are
    saved around them) and what a sweep issues: a lone wavefront pays ~4 cycles for EVERY instruction of the span, whatever it does
    (`insts_in_loop`: all of them, the cold blocks inside the span included; `s_nop_in_loop`: the hazard fillers among them).
    `text`: a disassembly to use instead of the library's."""
    out = {}
    for name, rows in _function_rows(disassemble(lib_path) if text is None else text, name_filter).items():
        lo = hi = None
        for off, op in rows:
            tgt = _branch_target(op)
            if tgt is not None and tgt < off and off - tgt > 200:
                if lo is None or off - tgt > hi - lo:         # the widest backward branch = the sweep loop
                    lo, hi = tgt, off
        inl = [op for off, op in rows if lo is not None and lo <= off <= hi]
        out[name] = dict(insts=len(rows), scratch=sum(op.startswith("scratch_") for _, op in rows), loop=(lo, hi),
                         ops_in_loop=[op.split(" ")[0] for op in inl], insts_in_loop=len(inl), s_nop_in_loop=sum(op.startswith("s_nop") for op in inl),
                         scratch_in_loop=sum(op.startswith("scratch_") for op in inl), valu_in_loop=sum(op.startswith("v_") for op in inl),
                         lds_in_loop=sum(op.startswith("ds_") for op in inl), lds_reads_in_loop=sum(op.startswith("ds_read") for op in inl),
                         vmem_in_loop=sum(op.startswith(("global_", "flat_", "buffer_")) for op in inl))
    return out


# what only the K7 early exit puts on a sweep's path: the rows' compares and the friction pairs' running maximum, the scalar merges of
# their wave masks with the has-a-zero-field test, and the branch on it (the fixed-iteration sweeps issue none of these)
_K7_ONLY = ("v_cmp_", "v_max3_f32", "s_or_b64", "s_and_b64", "s_andn2_b64", "s_sub_u32", "s_subb_u32", "s_cmp_eq_u64", "s_cmp_lg_u64")


def hot_path_stats(lib_path, name_filter, text=None):
    """The COMMON path of every sweep loop found by `name_filter` -- what a sweep issues when no team leaves in it, which is all but
    four of a solve's sweeps (`loop_stats` counts the whole span, the cold block that publishes a team's result included, and keeps
    that meaning).  The loop is the one closed by the widest backward branch on a scalar condition (the down-counter's); the path runs
    from that branch's target to the first forward branch -- the one that skips the cold block -- continues at its target, the counter
    block, and ends with the back edge: found as the SHORTEST instruction path from the loop head to the back edge over forward
    branches, which is that path wherever the block layout puts the cold block.  Returns {name: {"head", "back_edge", "insts",
    "s_nop", "k7_only", "ops": [mnemonics in path order]}}; `k7_only` counts the instructions left on the path that only the early
    exit needs (_K7_ONLY and the branch over the cold block)."""
    out = {}
    for name, rows in _function_rows(disassemble(lib_path) if text is None else text, name_filter).items():
        head = back = None
        for k, (off, op) in enumerate(rows):
            tgt = _branch_target(op)
            if tgt is not None and op.startswith("s_cbranch_scc") and tgt < off and off - tgt > 200:
                if head is None or off - tgt > rows[back][0] - head:
                    head, back = tgt, k
        if head is None:
            out[name] = dict(head=None, back_edge=None, insts=0, s_nop=0, k7_only=0, ops=[])
            continue
        index = {off: k for k, (off, _) in enumerate(rows)}
        INF = float("inf")
        best, nxt = [INF] * (len(rows) + 1), [None] * (len(rows) + 1)
        best[back] = 1
        for k in range(back - 1, index[head] - 1, -1):       # forward edges only: one pass from the back edge up
            off, op = rows[k]
            tgt = _branch_target(op)
            succ = []
            if not op.startswith(("s_branch", "s_endpgm", "s_setpc")):
                succ.append(k + 1)
            if tgt is not None and off < tgt <= rows[back][0] and tgt in index:
                succ.append(index[tgt])
            for j in succ:
                if best[j] + 1 < best[k]:
                    best[k], nxt[k] = best[j] + 1, j
        ops, k = [], index[head]
        while k is not None and best[k] < INF:
            ops.append(rows[k][1].split(" ")[0])
            k = nxt[k]
        skip = sum(1 for a, b in zip(ops, ops[1:]) if a.startswith("s_cbranch")) if ops else 0     # (branches on the path that are not its end)
        out[name] = dict(head=head, back_edge=rows[back][0], insts=len(ops), s_nop=sum(o.startswith("s_nop") for o in ops),
                         k7_only=sum(o.startswith(_K7_ONLY) for o in ops) + skip, ops=ops)
    return out


if __name__ == "__main__":
    import sys
    from .build import LIB
    for name, s in sorted(function_stats(sys.argv[1] if len(sys.argv) > 1 else LIB).items()):
        if s["insts"] > 100:
            print("%-120s insts %6d scratch %4d flat %4d global %4d" % (name[:120], s["insts"], s["scratch"], s["flat"], s["global"]))
