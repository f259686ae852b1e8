#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly listings of one kernel file, kernel by kernel: instruction count, VGPR / SGPR count,
scratch bytes, and whether the instruction streams are identical (symbol names and local label numbers aside).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only iisan_amd/csrc/rowops.hip -o new.s      (and the same at the parent)
    python3 tools/isa_compare.py parent.s new.s [--ignore-arg RowKeepNone] [--strip ELi768EEE=EEE] [--only layernorm768]

--ignore-arg NAME matches kernels by kernel name plus template arguments, read off the mangled names, instead of by the whole mangled
name, and drops a trailing template argument NAME first: a template parameter added with a default (`typename KEEP = RowKeepNone`)
leaves the instantiations that do not name it on the key they had.  The parameter list is not part of the key — an added template
argument renumbers the substitutions (`S9_` -> `SA_`) in it, which no textual rewrite of the name can follow.
--strip OLD=NEW rewrites mangled names of the NEW listing before matching (enough when the added argument is the last thing that can
be substituted: the 768-wide instantiations of rowops.hip gained a trailing `Li768E`).
Kernels only in the new listing are listed with their own figures.
--classes (anywhere on the line) adds a second table: per kernel and listing, the number of v_mfma*, v_exp_f32, ds_* and global_* /
buffer_* instructions — what has to stay put when a refactor moves only integer address arithmetic."""
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


# ---- kernel name + template arguments of an Itanium-mangled name: the subset of the grammar this project's kernels use -------------

def _source_name(s, i):
    m = re.compile(r"\d+").match(s, i)
    n = int(m.group())
    return s[m.end():m.end() + n], m.end() + n


def _template_args(s, i):
    """s[i] == 'I': the mangled arguments up to the matching 'E' and the position behind it"""
    args, i = [], i + 1
    while s[i] != "E":
        j = _type(s, i)
        args.append(s[i:j])
        i = j
    return args, i + 1


def _type(s, i):
    """position behind the type or literal that starts at s[i]"""
    c = s[i]
    if c == "L":                                # literal: L <type> <value> E
        return s.index("E", _type(s, i + 1)) + 1
    if c.isdigit():
        i = _source_name(s, i)[1]
        return _template_args(s, i)[1] if s[i] == "I" else i
    if c == "N":                                # nested name: components up to 'E'
        i += 1
        while s[i] != "E":
            i = _template_args(s, i)[1] if s[i] == "I" else _type(s, i)
        return i + 1
    if c in "PKROV":
        return _type(s, i + 1)
    if c == "S":
        return i + 2 if s[i + 1].islower() else s.index("_", i) + 1
    if c == "D":
        m = re.compile(r"DF\d+[_b]").match(s, i)
        return m.end() if m else i + 2
    if c in "IJ":
        return _template_args(s, i)[1]
    if c.islower():
        return i + 1
    raise ValueError(s[i:])


def _pretty(arg):
    m = re.fullmatch(r"L([a-z])(n?)(\d+)E", arg)
    if m:
        return ("false", "true")[int(m.group(3))] if m.group(1) == "b" else ("-" if m.group(2) else "") + m.group(3)
    m = re.fullmatch(r"\d+(\w+)", arg)
    return m.group(1) if m and _source_name(arg, 0)[1] == len(arg) else arg


def template_key(sym, ignore=()):
    """`kernel<arg, ...>` of a mangled kernel name, trailing arguments named in `ignore` dropped; the name itself where the parser gives up"""
    try:
        i, name, args = 2, None, []
        nested = sym[i] == "N"
        i += nested
        while True:
            part, i = _source_name(sym, i)
            if part != "_GLOBAL__N_1":
                name = part if name is None else name + "::" + part
            if not (nested and sym[i].isdigit()):
                break
        if sym[i] == "I":
            args = [_pretty(a) for a in _template_args(sym, i)[0]]
    except (ValueError, IndexError, AttributeError):
        return sym
    while args and args[-1] in ignore:
        args.pop()
    return name + ("<" + ", ".join(args) + ">" if args else "")


# --classes: the instructions whose number decides a kernel's speed, counted per kernel in both listings
CLASSES = {"v_mfma": r"v_mfma", "v_exp_f32": r"v_exp_f32", "ds": r"ds_", "global/buffer": r"(global|buffer)_"}


def main():
    args = sys.argv[1:]
    classes = "--classes" in args
    args = [a for a in args if a != "--classes"]
    strip, only, ignore = [], None, []
    while len(args) > 2:
        flag, val = args[-2], args[-1]
        if flag == "--strip":
            strip.append(val.split("="))
        elif flag == "--only":
            only = val
        elif flag == "--ignore-arg":
            ignore.append(val)
        else:
            sys.exit(__doc__)
        args = args[:-2]
    if len(args) != 2:
        sys.exit(__doc__)
    (old, om), (new, nm) = load(args[0]), load(args[1])

    def key(n, is_new):
        if ignore:
            return template_key(n, ignore)
        for a, b in strip if is_new else ():
            n = n.replace(a, b)
        return n

    oldk, newk = {key(n, False): n for n in old}, {key(n, True): n for n in new}
    if len(oldk) != len(old) or len(newk) != len(new):
        sys.exit("two kernels of one listing share a key: match by the whole mangled name (no --ignore-arg)")
    norm = lambda x: re.sub(r"\.L\w+?\d+_", ".L_", re.sub(r"_Z\w+", "SYM", x))
    print("| kernel | instructions parent -> new | VGPR / SGPR / scratch parent -> new | code |\n|---|---|---|---|")
    n_cmp = n_diff = 0
    for k in sorted(oldk):
        o = oldk[k]
        if only and only not in k:
            continue
        if k not in newk:
            print(f"| `{k}` | {len(old[o])} -> - | {om[o]} -> - | MISSING in the new listing |")
            n_diff += 1
            continue
        n = newk[k]
        same = [norm(x) for x in old[o]] == [norm(x) for x in new[n]] and om[o] == nm[n]
        n_cmp += 1
        n_diff += not same
        print(f"| `{k}` | {len(old[o])} -> {len(new[n])} | {om[o]} -> {nm[n]} | {'identical' if same else 'DIFFERENT'} |")
    for k in sorted(newk):
        if k not in oldk and (not only or only in k):
            n = newk[k]
            print(f"| `{k if ignore else n}` | - -> {len(new[n])} | - -> {nm[n]} | new |")
    print(f"\n{n_cmp} kernels compared, {n_diff} differ")
    if classes:
        count = lambda ins: " / ".join(str(sum(bool(re.match(c, x)) for x in ins)) for c in CLASSES.values())
        print("\n| kernel | " + " / ".join(CLASSES) + " parent | new |\n|---|---|---|")
        for k in sorted(set(oldk) | set(newk)):
            if not only or only in k:
                print(f"| `{k}` | {count(old[oldk[k]]) if k in oldk else '-'} | {count(new[newk[k]]) if k in newk else '-'} |")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
