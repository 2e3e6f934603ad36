#!/usr/bin/env python3
"""Per kernel of a gfx950 assembly file: VGPRs, scratch bytes, and what stands between the last matrix instruction and
the end of the program -- the count of full waits on memory (s_waitcnt vmcnt(0)), of global loads and of global stores.
A load -> wait -> store chain per element shows as about as many full waits as stores:
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only eigenkernel_amd/csrc/ek_gemm.hip -o ek_gemm.s
    python tools/epilogue_waits.py ek_gemm.s [name-filter]
Kernels without a matrix instruction are measured from their first instruction (column `from` says which)."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """name -> (lines of the body, {metadata key: value})"""
    body, meta, cur, last = {}, {}, None, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", s)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".Lfunc_end") and cur is not None:
            last, cur = cur, None
            meta[last] = {}
            continue
        if cur is not None:
            body[cur].append(s)
            continue
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", s)
        if m and last is not None:
            meta[last].setdefault(m.group(1), int(m.group(2)))
    return body, meta


def tail_counts(lines):
    last = -1
    for i, s in enumerate(lines):
        if s.startswith("v_mfma"):
            last = i
    tail = lines[last + 1:]
    waits = sum(1 for s in tail if re.match(r"s_waitcnt\s+vmcnt\(0\)", s))
    loads = sum(1 for s in tail if s.startswith("global_load"))
    stores = sum(1 for s in tail if s.startswith("global_store"))
    return ("mfma" if last >= 0 else "start"), waits, loads, stores


def main():
    path = sys.argv[1]
    filt = sys.argv[2] if len(sys.argv) > 2 else ""
    body, meta = kernels(path)
    names = [n for n in body if n in meta and meta[n].get("NumVgprs") is not None]
    pretty = demangle(names)
    print("%-60s %5s %5s %7s %5s %6s %6s %6s" % ("kernel", "vgpr", "agpr", "scratch", "from", "waits", "loads", "stores"))
    for n in names:
        p = re.sub(r"\(anonymous namespace\)::|ek::|void ", "", pretty[n]).split("(")[0]
        if filt and filt not in p:
            continue
        frm, w, l, st = tail_counts(body[n])
        md = meta[n]
        print("%-60s %5d %5d %7d %5s %6d %6d %6d" % (p[:60], md.get("NumVgprs", -1), md.get("NumAgprs", 0),
                                                    md.get("ScratchSize", -1), frm, w, l, st))


if __name__ == "__main__":
    main()
