#!/usr/bin/env python
"""Is a kernel still the same kernel?  Compares two `hipcc -S` outputs of one HIP source (compile-only: runs without a GPU),
e.g. the parent commit's and the working tree's, both made with the Makefile's flags plus `--cuda-device-only -S`.
Kernels are paired by mangled name.  Per kernel: SAME / DIFF for the instruction text (directives, comments and label-only
lines dropped, trailing `;` comments stripped), and next_free_vgpr, next_free_sgpr, accum_offset (where the AGPRs begin),
private_segment_fixed_size (scratch) and group_segment_fixed_size (static LDS) of both sides.  A kernel only one side has
is a DIFF.  Exit status 1 on any DIFF.
usage: tools/isa_compare.py <parent.s> <new.s>"""
import re
import sys

FIELDS = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]


def kernels(path):
    """{mangled name: (instruction lines, {field: value})}"""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, desc = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M).group(0)
        body = body.replace(m.group(0), "")   # the descriptor sits between the last instruction and .Lfunc_end
        ins = []
        for line in body.splitlines()[1:-1]:
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(" ".join(line.split()))
        res[name] = (ins, {f: int(re.search(r"\.amdhsa_%s (\d+)" % f, desc).group(1)) for f in FIELDS})
    return res


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"# {sys.argv[1]} -> {sys.argv[2]}")
    print("# verdict  instructions  vgpr  sgpr  accum_offset  scratch  lds   kernel")
    ndiff = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            ndiff += 1
            print(f"DIFF  only in {'parent' if name in old else 'new'}: {name}")
            continue
        (oi, of), (ni, nf) = old[name], new[name]
        same = oi == ni and of == nf
        ndiff += not same
        where = ""
        if oi != ni:
            first = next((k for k, (x, y) in enumerate(zip(oi, ni)) if x != y), min(len(oi), len(ni)))
            where = f"   first difference at instruction {first}"
        cols = "  ".join(f"{of[f]}->{nf[f]}" if of[f] != nf[f] else f"{of[f]}" for f in FIELDS)
        count = f"{len(oi)}" if len(oi) == len(ni) else f"{len(oi)}->{len(ni)}"
        print(f"{'SAME' if same else 'DIFF'}  {count}  {cols}  {name}{where}")
    print(f"# {len(set(old) | set(new))} kernels, {ndiff} DIFF")
    sys.exit(1 if ndiff else 0)


if __name__ == "__main__":
    main()
