#!/usr/bin/env python3
"""Resource table of a HIP file's gfx950 kernels, from its device assembly.

    tools/t7_resources.py [FILE.s | FILE.hip] [--loop SUBSTR]

A .hip file is compiled with the HIPFLAGS of csrc/Makefile (read from it) plus
--cuda-device-only -S; `make resources` runs this for every kernel file
(track7_pred.hip is the code object of the k_track7_pred instances:
tools/t7_resources.py csrc/track7_pred.hip --loop k_track7_pred; track7_mask.hip
that of k_track7_mask and k_track7_mask_lazy).
Per kernel, from the code object's metadata: VGPRs, SGPRs, scalar and vector
spill counts, scratch and LDS.  Then static instruction counts of the kernel's
whole text ("all") and of its largest outermost loop ("loop": the trackers'
frame loop, found by the compiler's block comments): VALU; reload / spill, the
lane reads and writes of the scalar spill register; all v_readlane /
v_writelane / v_readfirstlane; s_nop; scalar loads; s_waitcnt; SALU; branches.
--loop limits those rows to kernels whose demangled name contains SUBSTR.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "klt-feature-tracker-acceleration-gpus_amd", "csrc")
META = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def hipflags():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, re.M)
    flags = m.group(1).replace("$(ARCH)", "gfx950").replace("$(INC)", "-I%s -I%s" % (
        os.path.join(CSRC, "..", "..", "include"), CSRC))
    return flags.split()


def assemble(src, out):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc] + hipflags() + ["--cuda-device-only", "-S", src, "-o", out], check=True,
                   stderr=subprocess.DEVNULL)


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        res = out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        res = list(names)
    short = []
    for r in res:
        r = r.replace("kltdev::(anonymous namespace)::", "")
        short.append(r.split("(")[0].replace("void ", ""))
    return dict(zip(names, short))


def metadata(lines):
    """{mangled name: {field: int}} from the amdhsa.kernels YAML."""
    kernels, cur = {}, {}
    for ln in lines:
        s = ln.strip()
        if s.startswith("- .agpr_count:") or s.startswith("- .args:"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", s)
        if not m:
            continue
        if m.group(1) == "name" and m.group(2).startswith("_Z"):
            cur["name"] = m.group(2)
            kernels[m.group(2)] = cur
        elif m.group(1) in META:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def classify(op):
    return {
        "valu": op.startswith("v_") and not op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")),
        "readlane": op.startswith("v_readlane"),
        "writelane": op.startswith("v_writelane"),
        "readfirst": op.startswith("v_readfirstlane"),
        "s_nop": op == "s_nop",
        "s_load": op.startswith(("s_load", "s_buffer_load")),
        "waitcnt": op == "s_waitcnt",
        "salu": op.startswith("s_") and not op.startswith(("s_load", "s_buffer_load", "s_nop", "s_waitcnt",
                                                           "s_cbranch", "s_branch", "s_endpgm")),
        "branch": op.startswith(("s_cbranch", "s_branch")),
    }


KEYS = ("valu", "reload", "spill", "readlane", "writelane", "readfirst", "s_nop", "s_load", "waitcnt", "salu", "branch")


def body_of(lines, name):
    """Instructions [(op, text, loop)] of kernel `name`; loop: the label of the
    outermost (depth 1) loop the instruction's block belongs to, by the
    compiler's block comments, or None."""
    start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
    ins, loop, fresh, spill = [], None, False, None
    for ln in lines[start + 1:]:
        code, _, note = ln.partition(";")
        s = code.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.search(r"implicit-def: \$(vgpr\d+) : SGPR spill", note)
        if m:
            spill = "v" + m.group(1)[4:]
        m = re.match(r"\.L(BB\w+):", s)
        if m:  # a block starts: its comments (this line and the next ones) name its loops
            loop, fresh = None, True
            if "Loop Header: Depth=1" in note:
                loop = m.group(1)
        if fresh and (m or not s):
            d1 = re.search(r"(?:Header=|Parent Loop )(BB\w+) Depth=1", note)
            if d1:
                loop = d1.group(1)
            continue
        if not s or s.startswith("."):
            continue
        fresh = False
        ins.append((s.split()[0], s, loop))
    return ins, spill


def count(ins, spill):
    c = dict.fromkeys(KEYS, 0)
    for op, text, _ in ins:
        for k, hit in classify(op).items():
            c[k] += hit
        if spill and re.search(r",\s*%s," % spill, text):  # v_readlane_b32 sN, vSPILL, lane
            c["reload"] += op.startswith("v_readlane")
        if spill and re.match(r"v_writelane_b32\s+%s," % spill, text):
            c["spill"] += 1
    return c


def widest_loop(ins):
    """The instructions of the depth-1 loop that holds the most of them."""
    size = {}
    for _, _, loop in ins:
        if loop:
            size[loop] = size.get(loop, 0) + 1
    if not size:
        return []
    top = max(size, key=size.get)
    return [i for i in ins if i[2] == top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file", nargs="?", default=os.path.join(CSRC, "track7.hip"))
    ap.add_argument("--loop", default="")
    args = ap.parse_args()
    path = args.file
    tmp = None
    if not path.endswith(".s"):
        tmp = tempfile.mkdtemp()
        asm = os.path.join(tmp, "dev.s")
        assemble(path, asm)
        path = asm
    lines = open(path).read().splitlines()
    if tmp:
        shutil.rmtree(tmp)
    meta = metadata(lines)
    names = demangle(list(meta))
    print("%-46s %5s %5s %7s %7s %7s %6s" % ("kernel", "VGPR", "SGPR", "s.spill", "v.spill", "scratch", "LDS"))
    for k in sorted(meta, key=lambda k: names[k]):
        m = meta[k]
        print("%-46s %5d %5d %7d %7d %7d %6d" % (names[k], m["vgpr_count"], m["sgpr_count"], m["sgpr_spill_count"],
                                                 m["vgpr_spill_count"], m["private_segment_fixed_size"],
                                                 m["group_segment_fixed_size"]))
    print()
    print("%-46s %-6s %s" % ("kernel", "span", " ".join("%9s" % k for k in KEYS)))
    for k in sorted(meta, key=lambda k: names[k]):
        if args.loop not in names[k]:
            continue
        ins, spill = body_of(lines, k)
        for span, part in (("all", ins), ("loop", widest_loop(ins))):
            c = count(part, spill)
            print("%-46s %-6s %s" % (names[k], span, " ".join("%9d" % c[x] for x in KEYS)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
