#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds by symbol.

The check behind every "the earlier kernels are unchanged" in DESIGN.md.  Build
the assembly of both commits (the parent's from a `git worktree` or an
exported copy):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S \\
        libquic_amd/csrc/qfec_kernels.hip -o head.s
    python tools/kernel_diff.py parent.s head.s

A side with several kernel files (qfec_kernels.hip and qturn_kernels.hip; a
commit that moves kernels from one file to another) is their assembly files
concatenated, `cat xor.s turn.s > head.s`: kernels are paired by symbol
wherever they stand, and no two files define one kernel.  A change that edits
one kernel file and no header compares that file alone: the other file's
kernels are compiled from text it did not touch.

A kernel's stream is what libquic_amd/isa_guard.py cuts from its symbol's label
to its .Lfunc_end, comments dropped, with the function numbers taken out of the
local labels (.LBB<n>_ -> .LBB_): a kernel added or removed in front of another
renumbers those and changes nothing else.  Also compared, from each kernel's
.amdhsa_kernel block: next_free_vgpr, next_free_sgpr, group_segment_fixed_size,
private_segment_fixed_size and kernarg_size.

A change that drops template parameters renames its kernels.  Then

    python tools/kernel_diff.py --renames MAP parent.s head.s

renames the first file's kernels before pairing: each line of MAP holds two
mangled symbols, `old new`.  (No instruction mentions a kernel symbol; the
directives that close a kernel's stream name its own, and are renamed with
it.)  An `old` that is no kernel of the first file, or two lines with the same
`old` or the same `new`, end the run with exit status 2: a stale map must not
hide a missing kernel.

Prints the kernel counts, the symbols only one side has, the symbols whose
stream or resources differ.  Exit status 1 if anything differs.  CPU only.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libquic_amd import isa_guard  # noqa: E402

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size",
             "private_segment_fixed_size", "kernarg_size")
LOCAL_LABEL = re.compile(r"\.LBB\d+_")


def streams(path):
    """{symbol: [instruction and directive lines]} of an assembly file."""
    out = {}
    for name, _, body in isa_guard.kernels(path):
        out[name] = [LOCAL_LABEL.sub(".LBB_", line.strip()) for line in body if line.strip()]
    return out


def resources(path):
    """{symbol: {figure: value}} from the .amdhsa_kernel blocks."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
        if m and cur is not None and m.group(1) in RESOURCES:
            cur[m.group(1)] = m.group(2)
    return out


def _die(msg):
    print(msg, file=sys.stderr)
    sys.exit(2)


def read_renames(path, kernels):
    """{old: new} from a map file; exits 2 on a line that could hide a kernel."""
    ren = {}
    for n, line in enumerate(open(path), 1):
        f = line.split()
        if not f:
            continue
        if len(f) != 2:
            _die(f"{path}:{n}: expected `old new`, got {len(f)} fields")
        old, new = f
        if old not in kernels:
            _die(f"{path}:{n}: {old} is not a kernel of the first file")
        if old in ren:
            _die(f"{path}:{n}: {old} is renamed twice")
        if new in ren.values():
            _die(f"{path}:{n}: two kernels are renamed to {new}")
        ren[old] = new
    return ren


def main(argv):
    renames = None
    if len(argv) >= 3 and argv[1] == "--renames":
        renames, argv = argv[2], argv[:1] + argv[3:]
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = argv[1], argv[2]
    sa, sb, ra, rb = streams(a), streams(b), resources(a), resources(b)
    if renames is not None:
        ren = read_renames(renames, sa)
        # a rename onto a kernel that keeps its own name would merge the two
        for old, new in ren.items():
            if new in sa and new not in ren:
                _die(f"{renames}: {old} is renamed to {new}, a kernel of the first file")
        # (every old name leaves before a new one arrives: a new name may be
        # another line's old one; the directives at a stream's end name the
        # kernel's own symbol)
        moved = [(old, new, sa.pop(old), ra.pop(old, {})) for old, new in ren.items()]
        for old, new, stream, figures in moved:
            sa[new] = [line.replace(old, new) for line in stream]
            ra[new] = figures
    print(f"{a}: {len(sa)} kernels")
    print(f"{b}: {len(sb)} kernels")
    only_a, only_b = sorted(set(sa) - set(sb)), sorted(set(sb) - set(sa))
    both = sorted(set(sa) & set(sb))
    code = [n for n in both if sa[n] != sb[n]]
    res = [n for n in both if ra.get(n) != rb.get(n)]
    for title, names in ((f"only in {a}", only_a), (f"only in {b}", only_b),
                         ("instruction streams differ", code), ("resources differ", res)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
            if names is res:
                print("    " + ", ".join(f"{k} {ra[n].get(k)} -> {rb[n].get(k)}" for k in RESOURCES
                                         if ra[n].get(k) != rb[n].get(k)))
    same = len(both) - len(set(code) | set(res))
    print(f"{same} of {len(both)} common kernels identical (streams and resources)")
    sys.exit(1 if only_a or only_b or code or res else 0)


if __name__ == "__main__":
    main(sys.argv)
