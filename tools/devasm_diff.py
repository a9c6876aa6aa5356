#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 device assembly files.

    tools/devasm_diff.py OLD.s NEW.s [OLD2.s NEW2.s ...]

The files are what `hipcc $(HIPFLAGS) --cuda-device-only -S` writes (tools/
t7_resources.py's assemble).  For a change that must leave the device code
alone -- a host-side refactor -- every pair has to come out identical:
  * the same set of kernel symbols (t7_resources.metadata);
  * per kernel the same text from its label to its end: every instruction and
    the .amdhsa_kernel descriptor;
  * per kernel the same amdhsa.kernels entry: registers, spills, scratch, LDS,
    the arguments and the kernarg size.
The order of the kernels in the file follows the order of their first use in
the source and may differ; the number a function has by its place in the file
is therefore taken out of its local labels (.LBB<n>_, .Lfunc_end<n>, ...) and
out of the comments that name them.
One line per pair, then one per differing kernel; exit status 1 on any.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from t7_resources import demangle, metadata  # noqa: E402

LOCAL = re.compile(r"(BB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")  # BB: labels and the loop comments that name them


def bodies(lines):
    """{symbol: [line]} for every function: label line to .Lfunc_end."""
    out, name, cur = {}, None, None
    types = {m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+(\S+),@function", ln)] if m}
    for ln in lines:
        if name is None:
            m = re.match(r"(\S+):", ln)
            if m and m.group(1) in types:
                name, cur = m.group(1), []
            continue
        # the comment column moves with the width of a label's number
        cur.append(re.sub(r"\s+;", " ;", LOCAL.sub(lambda m: m.group(1), ln)))
        if ln.startswith(".Lfunc_end"):
            out[name], name = cur, None
    return out


def entries(lines):
    """{kernel symbol: [line]} of the amdhsa.kernels list."""
    start = next((i for i, ln in enumerate(lines) if ln.startswith("amdhsa.kernels:")), None)
    out, cur = {}, []
    if start is None:
        return out
    for ln in lines[start + 1:] + ["end"]:
        if ln.startswith("  - ") or not ln.startswith(" "):
            for e in cur:
                m = re.match(r"\s+\.name:\s+(\S+)$", e)
                if m:
                    out[m.group(1)] = cur
            cur = []
            if not ln.startswith(" "):
                break
        cur.append(ln)
    return out


def compare(old, new):
    a, b = (open(p).read().splitlines() for p in (old, new))
    ma, mb = metadata(a), metadata(b)
    fa, fb, ea, eb = bodies(a), bodies(b), entries(a), entries(b)
    names = demangle(sorted(set(ma) | set(mb) | set(fa) | set(fb)))
    bad = []
    for k in sorted(set(ma) ^ set(mb)):
        bad.append("%s only in %s" % (names[k], old if k in ma else new))
    for k in sorted((set(fa) ^ set(fb)) - (set(ma) ^ set(mb))):
        bad.append("function %s only in %s" % (names[k], old if k in fa else new))
    for k in sorted(set(fa) & set(fb)):
        what = [w for w, x, y in (("text", fa[k], fb[k]), ("metadata", ea.get(k), eb.get(k)),
                                  ("resources", ma.get(k), mb.get(k))) if x != y]
        if what:
            bad.append("%s differs in %s" % (names[k], ", ".join(what)))
    same_order = [k for k in fa if k in fb] == [k for k in fb if k in fa]
    print("%-18s %3d kernels, %3d functions in all: %s%s" % (
        os.path.basename(new), len(mb), len(fb), "DIFFERENT" if bad else "identical",
        "" if same_order else " (in another order)"))
    for ln in bad:
        print("    " + ln)
    return not bad


def main():
    args = sys.argv[1:]
    if not args or len(args) % 2:
        sys.exit(__doc__)
    ok = [compare(args[i], args[i + 1]) for i in range(0, len(args), 2)]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
