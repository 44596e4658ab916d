"""Per-kernel digest of hipcc -S listings: has a source change altered the code the GPU runs?

  python tools/kernel_isa.py digest file.s [file.s ...] [--filter TEXT]  > new.txt
  python tools/kernel_isa.py diff old.txt new.txt        (exit status 1 if a kernel is missing on either side or its line differs)

digest prints one tab-separated line per kernel, sorted by name: the demangled name without "(anonymous namespace)::", a hash
of the normalised instruction stream, its number of instructions, and from the .amdhsa_kernel block next_free_vgpr,
next_free_sgpr, private_segment_fixed_size (scratch bytes per lane) and group_segment_fixed_size (static LDS bytes).

Normalisation: a kernel's body runs from its label to its .Lfunc_end; everything from ';' on, blank lines and assembler
directives are dropped, basic-block labels are kept, and .LBB<function>_<block> becomes .LBB_<block> (the function number
changes when a kernel changes files).  Symbol references stay as text.  Listings come from `make isa` in csrc/.
"""
import hashlib
import re
import shutil
import subprocess
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
HEADER = "# kernel\thash\tinstructions\tvgpr\tsgpr\tscratch\tlds"


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if tool is None or not any(n.startswith("_Z") for n in names):
        return list(names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return [d.replace("(anonymous namespace)::", "") for d in out]


def normalise(body):
    """The instruction stream of one kernel: a list of lines (instructions and labels)."""
    lines = []
    for raw in body.splitlines():
        line = " ".join(raw.split(";", 1)[0].split())
        if not line:
            continue
        if line.startswith(".") and not line.endswith(":"):      # an assembler directive
            continue
        lines.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line))
    return lines


def kernels(text):
    """(mangled name, hash, instructions, vgpr, sgpr, scratch, lds) of every kernel in a listing."""
    rows = []
    for m in re.finditer(r"^[ \t]*\.amdhsa_kernel[ \t]+(\S+)(.*?)^[ \t]*\.end_amdhsa_kernel", text, re.S | re.M):
        name, block = m.group(1), m.group(2)
        start = re.search(r"^%s:" % re.escape(name), text, re.M)
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start.end())
        lines = normalise(text[start.end():end.start()])
        figures = [re.search(r"\.amdhsa_%s[ \t]+(\S+)" % f, block).group(1) for f in FIELDS]
        n_instr = sum(1 for l in lines if not l.endswith(":"))
        rows.append((name, hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], str(n_instr), *figures))
    return rows


def digest(texts, flt=""):
    rows = [r for t in texts for r in kernels(t)]
    names = demangle([r[0] for r in rows])
    return sorted("\t".join((n,) + r[1:]) for n, r in zip(names, rows) if flt in n)


def read_digest(lines):
    """name -> the rest of its line; '#' lines (notes, renames) are skipped."""
    table = {}
    for line in lines:
        line = line.rstrip("\n")
        if line and not line.startswith("#"):
            name, rest = line.split("\t", 1)
            table[name] = rest
    return table


def diff(a_lines, b_lines):
    """Report lines: kernels on one side only, and kernels whose hash or figures differ.  Empty: the digests agree."""
    a, b = read_digest(a_lines), read_digest(b_lines)
    out = ["only in first:  %s" % n for n in sorted(a.keys() - b.keys())]
    out += ["only in second: %s" % n for n in sorted(b.keys() - a.keys())]
    for n in sorted(a.keys() & b.keys()):
        if a[n] != b[n]:
            out.append("differs: %s\n    first:  %s\n    second: %s" % (n, a[n], b[n]))
    return out


def main(argv):
    if len(argv) >= 2 and argv[0] == "digest":
        args, flt = argv[1:], ""
        if "--filter" in args:
            i = args.index("--filter")
            flt = args[i + 1]
            del args[i:i + 2]
        print(HEADER)
        for line in digest([open(f).read() for f in args], flt):
            print(line)
        return 0
    if len(argv) == 3 and argv[0] == "diff":
        report = diff(open(argv[1]), open(argv[2]))
        for line in report:
            print(line)
        if not report:
            print("%d kernels, no difference" % len(read_digest(open(argv[1]))))
        return 1 if report else 0
    print(__doc__, file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
