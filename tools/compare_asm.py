#!/usr/bin/env python3
"""Compare the device code of two builds of csrc/mvba.s or csrc/mvsvd.s (`make asm`), kernel by kernel.

    python tools/compare_asm.py OLD.s NEW.s

A host-side change may reorder the template instantiations: the sections of the file then move, and the function ordinal
inside local labels (.LBB<n>_<k>, .Lfunc_end<n>, .Ltmp<n>) shifts.  Nothing else may differ.  So every function is keyed by
its symbol and compared with those ordinals normalised: its instructions, its kernel descriptor (.amdhsa_kernel block) and its
`.set <symbol>.<resource>` lines (num_vgpr, num_sgpr, scratch, ...).  Exit status 0: the same symbols, every one identical.
"""
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)(\d+)")


def norm(line):
    line = line.split(" ; ")[0].rstrip() if not line.lstrip().startswith(";") else ""
    return LABEL.sub(lambda m: "." + m.group(1) + "#", line)


def functions(path):
    """symbol -> {'text': [...], 'desc': [...], 'set': [...]}"""
    out = {}
    lines = open(path).read().splitlines()
    cur, part = None, None
    for ln in lines:
        s = ln.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            cur, part = m.group(1), "text"
            out.setdefault(cur, {"text": [], "desc": [], "set": []})
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur, part = m.group(1), "desc"
            out.setdefault(cur, {"text": [], "desc": [], "set": []})
            continue
        m = re.match(r"\.set\s+([^,\s]+)\.(\w+),", s)
        if m and m.group(1) in out:
            out[m.group(1)]["set"].append(norm(s))
            continue
        if cur is None:
            continue
        if part == "text" and re.match(r"\.Lfunc_end\d+:", s):
            cur = None
            continue
        if part == "desc" and s == ".end_amdhsa_kernel":
            cur = None
            continue
        n = norm(s)
        if n:
            out[cur][part].append(n)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    ka = {k for k, v in a.items() if v["desc"]}
    kb = {k for k, v in b.items() if v["desc"]}
    bad = 0
    for k in sorted(set(a) - set(b)):
        print("missing in new:", k); bad += 1
    for k in sorted(set(b) - set(a)):
        print("new symbol:", k); bad += 1
    for k in sorted(set(a) & set(b)):
        for part in ("text", "desc", "set"):
            if a[k][part] != b[k][part]:
                print(f"differs ({part}):", k); bad += 1
    plain = open(sys.argv[1]).read() == open(sys.argv[2]).read()
    print(f"{len(ka)} kernels in old, {len(kb)} in new, {len(set(a) & set(b))} functions compared, "
          f"{'files byte-identical' if plain else 'files differ in order / label ordinals'}; {bad} difference(s)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
