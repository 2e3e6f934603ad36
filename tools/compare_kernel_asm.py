#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files (hipcc --cuda-device-only -S), DESIGN.md 33's procedure: the
function bodies between a kernel's label and its .end_amdhsa_kernel / .Lfunc_end, comments stripped, the function number
in block labels masked.  Prints one line per kernel of the first file (identical / DIFFERENT / absent), then the kernels
only the second file has with their registers, LDS and scratch.

    tools/compare_kernel_asm.py [--in-order] parent.s new.s

--in-order: the k-th kernel of the first file is compared with the k-th of the second, whatever their names (templates
that were renamed or took a parameter; both files must hold the same number of kernels), and both names are printed.
"""
import re
import sys


def kernels(path):
    out, meta, name, body = {}, {}, None, []
    for line in open(path):
        s = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", s)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if s.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = re.sub(r"\.LBB\d+_", ".LBB_", s).strip()
            if s and not s.startswith(".loc") and not s.startswith(".file"):
                body.append(s)
    cur = None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            meta[cur] = {}
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size|"
                     r"accum_offset)\s+(\S+)", line)
        if m and cur:
            meta[cur][m.group(1)] = m.group(2)
    return out, meta


def main():
    args = [x for x in sys.argv[1:] if x != "--in-order"]
    a, _ = kernels(args[0])  # noqa
    b, meta = kernels(args[1])
    if "--in-order" in sys.argv:
        ka, kb = [k for k in a if k in _], [k for k in b if k in meta]
        assert len(ka) == len(kb), (len(ka), len(kb))
        for old, new in zip(ka, kb):
            print("paired     ", old, "->", new, meta[new], "was", _[old])
        a = {new: [line.replace(old, new) for line in a[old]] for old, new in zip(ka, kb)}
    same = diff = 0
    for k in sorted(a):
        if k not in meta and k not in b:
            print("absent     ", k)
        elif a[k] == b.get(k):
            same += 1
            print("identical  ", len(a[k]), k)
        else:
            diff += 1
            print("DIFFERENT  ", len(a[k]), len(b.get(k, [])), k)
    print("%d identical, %d different" % (same, diff))
    for k in sorted(b):
        if k not in a and k in meta:
            print("new        ", len(b[k]), k, meta[k])
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
