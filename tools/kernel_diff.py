#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of one source file by symbol.

The check behind every "the earlier kernels are unchanged" in DESIGN.md.  Build
the assembly of both commits (the parent's from a `git worktree` or an
exported copy):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S \\
        libquic_amd/csrc/qfec_kernels.hip -o head.s
    python tools/kernel_diff.py parent.s head.s

A kernel's stream is what libquic_amd/isa_guard.py cuts from its symbol's label
to its .Lfunc_end, comments dropped, with the function numbers taken out of the
local labels (.LBB<n>_ -> .LBB_): a kernel added or removed in front of another
renumbers those and changes nothing else.  Also compared, from each kernel's
.amdhsa_kernel block: next_free_vgpr, next_free_sgpr, group_segment_fixed_size,
private_segment_fixed_size and kernarg_size.

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


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = argv[1], argv[2]
    sa, sb, ra, rb = streams(a), streams(b), resources(a), resources(b)
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
