"""Compare the gfx950 kernels of two builds of libpathtrace_hip.so, kernel symbol by kernel symbol: the instruction text (llvm-objdump -d
with the `// address: encoding` comments and the padding behind a function removed) and the register notes of the code objects.

    python tools/kernel_diff.py OLD.so NEW.so [--match SUBSTR]

Per kernel: "identical" or the number of differing lines, then VGPRs, SGPRs, scratch bytes and spill counts of both builds.  This is the
check DESIGN.md 2.1 and 2.2 made by hand after moving device code between files: a move that is meant to change nothing shows as
"identical" for every kernel it was not meant to touch.  Exit status 0 whatever it finds: it reports, the reader judges."""
import argparse
import difflib
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
NOTES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
PADDING = re.compile(r"^(s_nop 0|s_code_end|\.\.\.|)$")


def kernels(lib, tmp, tag):
    """{symbol: (instruction lines, notes)} over every code object of the library."""
    data = open(lib, "rb").read()
    # code objects sit in .hip_fatbin as ELF images behind a clang offload bundle header; the first ELF is the host library itself
    starts = [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01", data)][1:]
    found = {}
    for i, s in enumerate(starts):
        path = os.path.join(tmp, "%s%d.o" % (tag, i))
        with open(path, "wb") as fh:
            fh.write(data[s:])
        notes, rec = {}, {}
        for line in subprocess.run([LLVM + "/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"\s+[-\s]*\.(\w+):\s+(.*)$", line)
            if not m:
                continue
            rec[m.group(1)] = m.group(2).strip()
            if m.group(1) == "wavefront_size":  # the last key of a kernel's record
                notes[rec.get("name", "?")] = rec
                rec = {}
        text, name = {}, None
        for line in subprocess.run([LLVM + "/llvm-objdump", "-d", path], capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
                text[name] = []
            elif name is not None:
                text[name].append(line.split("//")[0].strip())
        for name, lines in text.items():
            if name in notes:
                while lines and PADDING.match(lines[-1]):
                    lines.pop()
                found[name] = (lines, notes[name])
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="", help="only kernels whose symbol contains this")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(args.old, tmp, "old"), kernels(args.new, tmp, "new")
    names = sorted(n for n in set(old) | set(new) if args.match in n)
    print("old: %s\nnew: %s\n%d kernels%s" % (args.old, args.new, len(names), " matching '%s'" % args.match if args.match else ""))
    for n in names:
        print(n)
        if n not in old or n not in new:
            print("    only in the %s build" % ("new" if n in new else "old"))
            continue
        (a, na), (b, nb) = old[n], new[n]
        differing = sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op != "equal")
        print("    %s" % ("identical (%d lines)" % len(a) if differing == 0 else "%d differing lines of %d -> %d" % (differing, len(a), len(b))))
        print("    " + ", ".join("%s %s -> %s" % (k, na.get(k, "?"), nb.get(k, "?")) for k in NOTES))


if __name__ == "__main__":
    main()
