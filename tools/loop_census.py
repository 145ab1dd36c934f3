"""Census of the path kernel's inner loop, read from the compiler's assembly: what the code between two bursts of traversal steps
(retire, pass trigger, hand-out, Tracer::start, window reload) is made of, and how large the burst loop itself is.

    python tools/loop_census.py [--csrc DIR] [--asm FILE] [--keep FILE]

Compiles csrc/pt_path.hip to gfx950 assembly with the flags of cpupathtrace_amd/build.py (device side only) and reports, for every
instantiation of pt_path_kernel, four regions:

    ahead    the inner for(;;) of the kernel in front of the burst loop (text order)
    behind   the rest of that loop behind the burst loop
    burst    the burst loop itself (with the loop of slow_step's pops inside it)
    pop      the loop of slow_step's pops alone: the one loop nested in the burst loop (counted in `burst` as well)

and per region: instructions, VGPR-to-VGPR moves (v_mov_b32 / v_mov_b64 from a vector register), lane reads and writes (v_readlane /
v_writelane: the reloads and saves of spilled scalars), flat loads, scratch accesses, branches and record loads (`record_loads`:
global_load_dwordx4 -- a 64-byte record is a row of four of them).  Beside the regions, an instantiation's result holds `record_groups`: the
lengths of the uninterrupted rows of such loads in the burst loop, in text order.  A tree in HBM has two rows of four there (node_step's
request, and the one behind the rare step: tests/test_step_fetch_census.py); a tree in LDS is read with ds_read and has none.

The regions are found by the loop annotations the compiler writes next to every basic block ("in Loop: Header=BB0_123 Depth=2"), not by
markers in the source, which would change the code they are meant to measure: the inner loop is the innermost loop whose own blocks hold
the hand-out's ds_bpermute_b32, the burst loop the one loop nested in it that holds the packed slab arithmetic (v_pk_mul_f32), the pop loop the one loop nested in that.
--csrc DIR takes the sources of another checkout (the parent's, for a side-by-side table); --asm FILE reads an assembly file made earlier.
tests/test_path_loop_census.py holds ceilings on these numbers."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGIONS = ("ahead", "behind", "burst", "pop")
COLUMNS = ("instructions", "moves", "lane_reads", "lane_writes", "flat_loads", "scratch", "branches", "record_loads")

_KERNEL = re.compile(r"^(_Z\w*pt_path_kernelILb([01])ELb([01])ELi(\d+)E\w*):")
_LABEL = re.compile(r"^\.L(BB\d+_\d+):")
_ENTRY = re.compile(r"^; %bb\.\d+:")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
_VGPR_SRC = re.compile(r"^v_mov_b(?:32|64)(?:_e32|_e64)?\s+v[\[\d][^,]*,\s*v[\[\d]")


def compile_asm(csrc, out, extra=()):
    """pt_path.hip of `csrc` -> assembly file `out`, with the library's flags."""
    from cpupathtrace_amd import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-pthread")]
    cmd = [build.hipcc()] + flags + list(extra) + ["-Wno-unused-command-line-argument", "-x", "hip", "--cuda-device-only", "-S", os.path.join(csrc, "pt_path.hip"), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def _blocks(lines):
    """Basic blocks of one function in text order: [name, innermost loop header or None, instruction list]; and {header: parent header or None}."""
    blocks, parent = [], {}
    cur = ["entry", None, []]
    blocks.append(cur)
    i = 0
    while i < len(lines):
        line = lines[i]
        label = _LABEL.match(line)
        if label or _ENTRY.match(line):
            name = label.group(1) if label else line.split(":")[0]
            loop = None
            head = _HEADER.search(line)
            # a header's annotation may run over the following comment lines: "Parent Loop ..." first, "=> This Loop Header" last
            notes = [line]
            j = i + 1
            while j < len(lines) and lines[j].startswith(" ") and lines[j].strip().startswith(";"):
                notes.append(lines[j])
                j += 1
            text = " ".join(notes)
            head = _HEADER.search(text)
            if head and label:
                depth = int(head.group(1))
                loop = name
                up = [m.group(1) for m in _PARENT.finditer(text) if int(m.group(2)) == depth - 1]
                parent[name] = up[0] if up else None
            else:
                inside = _IN_LOOP.search(text)
                loop = inside.group(1) if inside else None
            cur = [name, loop, []]
            blocks.append(cur)
            i = j
            continue
        s = line.strip()
        if line.startswith("\t") and s and not s.startswith((".", ";")):
            cur[2].append(s.split(";")[0].strip())
        i += 1
    return blocks, parent


def _count(instrs):
    c = dict.fromkeys(COLUMNS, 0)
    for ins in instrs:
        op = ins.split()[0]
        c["instructions"] += 1
        c["moves"] += 1 if _VGPR_SRC.match(ins) else 0
        c["lane_reads"] += 1 if op.startswith("v_readlane") else 0
        c["lane_writes"] += 1 if op.startswith("v_writelane") else 0
        c["flat_loads"] += 1 if op.startswith("flat_load") else 0
        c["scratch"] += 1 if op.startswith("scratch_") else 0
        c["branches"] += 1 if op.startswith(("s_cbranch", "s_branch")) else 0
        c["record_loads"] += 1 if op.startswith("global_load_dwordx4") else 0
    return c


def _record_groups(instrs):
    """Lengths of the uninterrupted rows of global_load_dwordx4 in an instruction list, in text order (the s_nop the compiler puts in
    front of the load that overwrites its own address registers does not end a row)."""
    groups, row = [], 0
    for ins in instrs:
        if ins.split()[0].startswith("global_load_dwordx4"):
            row += 1
        elif row and not ins.startswith("s_nop"):
            groups.append(row)
            row = 0
    return groups + ([row] if row else [])


def census_function(lines):
    blocks, parent = _blocks(lines)

    def within(loop, outer):  # is `loop` the loop `outer` or nested in it
        while loop is not None:
            if loop == outer:
                return True
            loop = parent.get(loop)
        return False

    def depth(loop):
        d = 0
        while loop is not None:
            d, loop = d + 1, parent.get(loop)
        return d

    handout = {b[1] for b in blocks if b[1] and any(i.startswith("ds_bpermute_b32") for i in b[2])}
    if not handout:
        raise RuntimeError("no loop holds the hand-out's ds_bpermute_b32")
    inner = max(handout, key=depth)
    burst = [h for h, p in parent.items() if p == inner and any(within(b[1], h) and any(i.startswith("v_pk_mul_f32") for i in b[2]) for b in blocks)]
    if len(burst) != 1:
        raise RuntimeError("expected one burst loop inside %s, found %r" % (inner, burst))
    burst = burst[0]
    pop = [h for h, p in parent.items() if p == burst]
    if len(pop) != 1:
        raise RuntimeError("expected one pop loop inside %s, found %r" % (burst, pop))
    pop = pop[0]
    order = [k for k, b in enumerate(blocks) if within(b[1], burst)]
    first, last = order[0], order[-1]
    region = {r: [] for r in REGIONS}
    for k, b in enumerate(blocks):
        if within(b[1], burst):
            region["burst"] += b[2]
            if within(b[1], pop):
                region["pop"] += b[2]
        elif within(b[1], inner):
            region["ahead" if k < first else "behind" if k > last else "ahead"] += b[2]
    out = {r: _count(region[r]) for r in REGIONS}
    out["record_groups"] = _record_groups(region["burst"])
    out["loops"] = {"inner": inner, "burst": burst, "pop": pop, "inner_depth": depth(inner)}
    return out


def census(asm_text):
    """{"<wide,in_lds,window>": {region: {column: count}}} for every instantiation of pt_path_kernel in the assembly."""
    lines = asm_text.splitlines()
    found = {}
    k = 0
    while k < len(lines):
        m = _KERNEL.match(lines[k])
        if m:
            end = k + 1
            while end < len(lines) and not lines[end].startswith(".Lfunc_end"):
                end += 1
            name = "<%s,%s,%s>" % ("true" if m.group(2) == "1" else "false", "true" if m.group(3) == "1" else "false", m.group(4))
            found[name] = census_function(lines[k + 1:end])
            k = end
        k += 1
    return found


def run(csrc=None, asm=None, keep=None):
    if asm is None:
        with tempfile.TemporaryDirectory() as tmp:
            asm = compile_asm(csrc or os.path.join(ROOT, "cpupathtrace_amd", "csrc"), keep or os.path.join(tmp, "pt_path.s"))
            return census(open(asm).read())
    return census(open(asm).read())


def table(result):
    rows = ["%-18s %-7s" % ("instantiation", "region") + "".join("%13s" % c for c in COLUMNS)]
    for name in sorted(result):
        for r in REGIONS:
            rows.append("%-18s %-7s" % (name, r) + "".join("%13d" % result[name][r][c] for c in COLUMNS))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--csrc", help="directory of pt_path.hip and its headers (default: this tree's)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the assembly in this file")
    args = ap.parse_args()
    print(table(run(args.csrc, args.asm, args.keep)))


if __name__ == "__main__":
    main()
