#!/usr/bin/env python3
"""Does the working tree generate the device code that <rev> generated?

    scripts/isa_diff.py [--keep DIR] [--ops] [--rename OLD=NEW ...] <rev> [rewriting_amd/csrc/rw_x.hip ...]      (default: every .hip of rewriting_amd/csrc)

The sources of <rev> (git show <rev>:path) go into a temporary directory; both sides are compiled to gfx950 assembly
with the library's own flags (csrc/build.sh, the file's "// hipcc-flags:" line, + --cuda-device-only -S), at most 16
compilations at a time.  The listings are split at the function symbols and compared as text, kernel by kernel: the
instruction text and the .amdhsa_* resource block (registers, scratch, LDS).  The lines that name the compilation
unit's __hip_cuid_ symbol are dropped -- they differ between two builds of unchanged code -- and so is the function index
inside local labels.  --rename compares a kernel of <rev> with the one that carries another symbol now.  Per kernel one line,
"same", or "differs" with both instruction counts and both resource blocks; exit status 1 if anything differs.
--ops adds, per differing kernel, the arithmetic mnemonics whose counts changed (ARITH below: floating-point VALU
operations, conversions, selects, MFMAs, lane permutes -- integer address arithmetic, moves, waits and nops are not
counted) or "arithmetic instructions: equal multiset": the same operations on other registers or in another order.
Needs hipcc and git, no GPU.  A full run compiles every file twice and takes minutes.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "rewriting_amd/csrc"
HEADERS = [CSRC + "/rw_common.h", CSRC + "/rw_inflate_core.h", "include/rewriting_hip.h"]
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result".split()
NOPK = "-Xclang -target-feature -Xclang -packed-fp32-ops".split()
# --ops: floating-point arithmetic (the _dpp forms included), conversions and selects; matrix instructions; lane permutes
ARITH = re.compile(r"v_(pk_)?(add|sub|mul|fma|fmac|mac|mad|max|min|rsq|sqrt|rcp|div\w*)_\w*(f16|f32|f64)\w*$"
                   r"|v_(cvt\w*|cndmask)\w*$|v_\w*mfma\w*$|v_permlane\w*$")


def compile_asm(tree, rel, out):
    src = os.path.join(tree, rel)
    with open(src) as f:
        head = f.read(4096)
    extra = re.search(r"^// hipcc-flags: (.*)$", head, re.M)
    keep_pk = re.search(r"^// hipcc-keep-packed-fp32", head, re.M)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ([] if keep_pk else NOPK)
    cmd += (extra.group(1).split() if extra else []) + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stdout))
    return out


# local labels carry the function's index in its file (.LBB10_6, BB10_9 in comments, .Lfunc_end10, .LJTI10_0), which moves
# when a kernel is added, removed or reordered in front of it: the index is dropped
LOCAL_LABEL = re.compile(r"(\.L|\b)(BB|JTI|func_begin|func_end)\d+")


def split_listing(path, rename=()):
    """{symbol: [lines]} for every function, {kernel: [.amdhsa_ lines]}, and the lines outside both; rename: (old, new)
    pairs of symbols, applied to every line."""
    funcs, res, rest = {}, {}, []
    cur = kern = None
    with open(path) as f:
        for line in f:
            line = re.sub(r"\s+;", " ;", LOCAL_LABEL.sub(r"\1\2", line.rstrip()))    # (comments are padded to a column)
            for old, new in rename:
                line = line.replace(old, new)
            if "__hip_cuid_" in line:
                continue
            if cur is not None and re.match(r"\s*(\.text$|\.section\s+\.text\.)", line):
                continue                 # back to the code section: ".text", or the own section of a template instantiation
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                cur = m.group(1)
                funcs[cur] = []
                continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                kern = m.group(1)
                res[kern] = []
                continue
            if kern is not None:
                if line.strip() == ".end_amdhsa_kernel":
                    kern = None
                else:
                    res[kern].append(line.strip())
                continue
            if cur is not None:
                if re.match(r"\s*\.size\s+%s," % re.escape(cur), line):
                    cur = None
                else:
                    funcs[cur].append(line)
                continue
            rest.append(line)
    return funcs, res, rest


def n_instructions(lines):
    n = 0
    for line in lines:
        s = line.strip()
        if s and not s.startswith((".", ";")) and not s.split(";")[0].rstrip().endswith(":"):
            n += 1
    return n


def arith_counts(lines):
    """{mnemonic: count} of the instructions ARITH matches"""
    counts = {}
    for line in lines:
        s = line.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            m = s.split()[0]
            if ARITH.match(m):
                counts[m] = counts.get(m, 0) + 1
    return counts


def show_resources(tag, block):
    keep = [l for l in block if re.search(r"vgpr|sgpr|private_segment_fixed|group_segment_fixed|accum_offset", l)]
    print("      %s: %s" % (tag, "  ".join(l.replace(".amdhsa_", "") for l in keep)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("files", nargs="*")
    ap.add_argument("--ops", action="store_true", help="per differing kernel: the arithmetic mnemonics whose counts changed")
    ap.add_argument("--keep", metavar="DIR", help="keep both listings of every file in DIR (<file>.old.s, <file>.new.s)")
    ap.add_argument("--rename", metavar="OLD=NEW", action="append", default=[],
                    help="a symbol of <rev> and its name in the working tree (a kernel that became a template instantiation)")
    args = ap.parse_args()
    rename = [tuple(r.split("=", 1)) for r in args.rename]
    files = [os.path.relpath(os.path.abspath(f), ROOT) for f in args.files]
    if not files:
        files = sorted(CSRC + "/" + f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))

    differing = 0
    with tempfile.TemporaryDirectory() as tmp:
        lst = tmp
        if args.keep:
            lst = os.path.abspath(args.keep)
            os.makedirs(lst, exist_ok=True)
        for rel in files + HEADERS:
            dst = os.path.join(tmp, "old", rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(dst, "wb") as f:
                f.write(subprocess.check_output(["git", "show", "%s:%s" % (args.rev, rel)], cwd=ROOT))
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for rel in files:
                base = os.path.basename(rel)
                jobs[rel] = (pool.submit(compile_asm, os.path.join(tmp, "old"), rel, os.path.join(lst, base + ".old.s")),
                             pool.submit(compile_asm, ROOT, rel, os.path.join(lst, base + ".new.s")))
            for rel in files:
                old_f, old_r, old_x = split_listing(jobs[rel][0].result(), rename)
                new_f, new_r, new_x = split_listing(jobs[rel][1].result())
                print("%s  (%d lines of assembly at %s, %d now)" % (
                    rel, sum(map(len, old_f.values())) + len(old_x), args.rev, sum(map(len, new_f.values())) + len(new_x)))
                for name in sorted(set(old_f) | set(new_f)):
                    a, b = old_f.get(name), new_f.get(name)
                    ra, rb = old_r.get(name, []), new_r.get(name, [])
                    if a == b and ra == rb:
                        print("  same     %s" % name)
                        continue
                    differing += 1
                    if a is None or b is None:
                        print("  differs  %s  (only %s)" % (name, "in the working tree" if a is None else "at " + args.rev))
                        continue
                    print("  differs  %s  instructions %d -> %d, resource block %s" % (
                        name, n_instructions(a), n_instructions(b), "equal" if ra == rb else "DIFFERENT"))
                    show_resources(args.rev, ra)
                    show_resources("now", rb)
                    if args.ops:
                        ca, cb = arith_counts(a), arith_counts(b)
                        changed = ["%s %d -> %d" % (m, ca.get(m, 0), cb.get(m, 0))
                                   for m in sorted(set(ca) | set(cb)) if ca.get(m, 0) != cb.get(m, 0)]
                        print("      arithmetic instructions: %s" % ("  ".join(changed) if changed else "equal multiset"))
                if old_x != new_x:
                    differing += 1
                    print("  differs  (the listing outside the functions: data, metadata)")
    print("%d differ" % differing if differing else "all same")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
