#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings of one kernel file, kernel by kernel: instruction count, VGPR / SGPR count,
scratch bytes, and whether the instruction streams are identical (symbol names and local label numbers aside).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only iisan_amd/csrc/rowops.hip -o new.s      (and the same at the parent)
    python3 tools/isa_compare.py parent.s new.s [--strip ELi768EEE=EEE] [--only layernorm768]

--strip OLD=NEW rewrites mangled names of the NEW listing before matching (a template parameter added with a default: the 768-wide
instantiations of rowops.hip gained a trailing `Li768E`).  Kernels only in the new listing are listed with their own figures."""
import re
import sys


def load(path):
    txt = open(path).read()
    body = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end", txt, re.S | re.M):
        ins = [l.strip() for l in m.group(2).split("\n")]
        ins = [l for l in ins if l and not l.startswith((";", ".")) and not l.endswith(":")]
        if "s_endpgm" in ins:                   # (padding behind the last s_endpgm)
            ins = ins[:len(ins) - ins[::-1].index("s_endpgm")]
        body[m.group(1)] = ins
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", txt, re.S):
        get = lambda k: int(re.search(k + r":\s*(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = (get(r"\.vgpr_count"), get(r"\.sgpr_count"), get(r"\.private_segment_fixed_size"))
    return body, meta


def main():
    args = sys.argv[1:]
    strip, only = [], None
    while len(args) > 2:
        flag, val = args[-2], args[-1]
        if flag == "--strip":
            strip.append(val.split("="))
        elif flag == "--only":
            only = val
        else:
            sys.exit(__doc__)
        args = args[:-2]
    if len(args) != 2:
        sys.exit(__doc__)
    (old, om), (new, nm) = load(args[0]), load(args[1])

    def key(n):
        for a, b in strip:
            n = n.replace(a, b)
        return n

    newk = {key(n): n for n in new}
    norm = lambda x: re.sub(r"\.L\w+?\d+_", ".L_", re.sub(r"_Z\w+", "SYM", x))
    print("| kernel | instructions parent -> new | VGPR / SGPR / scratch parent -> new | code |\n|---|---|---|---|")
    n_cmp = n_diff = 0
    for k in sorted(old):
        if only and only not in k:
            continue
        if k not in newk:
            print(f"| `{k}` | {len(old[k])} -> - | {om[k]} -> - | MISSING in the new listing |")
            n_diff += 1
            continue
        n = newk[k]
        same = [norm(x) for x in old[k]] == [norm(x) for x in new[n]] and om[k] == nm[n]
        n_cmp += 1
        n_diff += not same
        print(f"| `{k}` | {len(old[k])} -> {len(new[n])} | {om[k]} -> {nm[n]} | {'identical' if same else 'DIFFERENT'} |")
    for k in sorted(newk):
        if k not in old and (not only or only in k):
            n = newk[k]
            print(f"| `{n}` | - -> {len(new[n])} | - -> {nm[n]} | new |")
    print(f"\n{n_cmp} kernels compared, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
