#!/usr/bin/env python3
"""Is the device code of two checkouts the same?  Runs without a GPU (hipcc cross-compiles gfx950).

  python tools/isa_diff.py <checkout A> <checkout B> [--jobs N] [--keep DIR] [--only REGEX]

Every translation unit of each checkout (its own fmcmc_amd/build.py: units(), or sources() in a checkout from before units())
is compiled with that checkout's own command line plus `--cuda-device-only -S`.  Units pair by object name, and within a pair
the assembly is compared function by function, so the order of the functions in a unit may differ: the numbers that LLVM
gives a function's local labels by its position in the unit (.LBB12_3, .Lfunc_end12) are taken out, with the padding of the
comments behind them, and a kernel's entry in .amdgpu_metadata goes with the kernel.  `.file` and `.ident` lines and the `__hip_cuid_<hash>` symbol, a hash of the source
path, are dropped.  One line per unit: functions, identical, differing; every differing function is named.  Exit status 0:
the same units, the same symbols in each, every function identical."""
import argparse
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile


def load_build(root):
    spec = importlib.util.spec_from_file_location("fmcmc_build_%x" % abs(hash(root)), os.path.join(root, "fmcmc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def commands(root, asmdir):
    """{unit name: (compile command, assembly file)} of a checkout"""
    B = load_build(root)
    us = B.units() if hasattr(B, "units") else [(s, None, os.path.splitext(os.path.basename(s))[0] + ".o", []) for s in B.sources()]
    out = {}
    for src, _part, obj, unit_flags in us:
        name = os.path.splitext(os.path.basename(obj))[0]
        asm = os.path.join(asmdir, name + ".s")
        out[name] = ([B.HIPCC] + list(B.FLAGS) + list(unit_flags) + ["--cuda-device-only", "-S", src, "-o", asm], asm)
    return out


LOCAL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b")   # .LBB12_3, .Lfunc_end12, and BB12_3 in the loop comments
LEAD = ("\t.globl", "\t.protected", "\t.weak", "\t.hidden", "\t.p2align", "\t.section", "\t.text")


def split(asm):
    """{symbol: lines} of an assembly file, functions and variables; '<unit>' holds what belongs to none"""
    chunks = {"<unit>": []}
    cur = chunks["<unit>"]
    lines = [l.rstrip("\n") for l in open(asm)]
    i, meta = 0, False
    while i < len(lines):
        l = lines[i]
        i += 1
        if l.startswith(("\t.file", "\t.ident")) or "__hip_cuid_" in l:
            continue
        if l.startswith("\t.amdgpu_metadata"):
            meta, cur = True, chunks["<unit>"]
        if meta:
            if l.startswith("  - ."):                 # one kernel's entry: to the kernel, by its .name
                j = i
                while j < len(lines) and not lines[j].startswith(("  - .", "amdhsa.", "...")):
                    j += 1
                entry = [l] + lines[i:j]
                name = [m.group(1) for e in entry for m in [re.match(r"\s+\.name:\s+(\S+)", e)] if m]
                chunks.setdefault(name[0] if name else "<unit>", []).extend(entry)
                i = j
            else:
                cur.append(l)
            continue
        if l.startswith("\t.section\t.AMDGPU.gpr_maximums"):   # (what follows the last function, from the padding of the text's end)
            pad = []
            while cur and cur[-1].startswith(("\t.text", "\t.p2alignl", "\t.fill")):
                pad.append(cur.pop())
            cur = chunks["<unit>"]
            cur.extend(reversed(pad))
        m = re.match(r"\t\.type\t(\S+),@(?:function|object)", l)
        if m:
            lead = []
            while cur and cur[-1].startswith(LEAD):   # (the directives in front of a function or a variable belong to it)
                lead.append(cur.pop())
            cur = chunks.setdefault(m.group(1), [])
            cur.extend(reversed(lead))
        # (the padding in front of a comment depends on the width of the label's number)
        cur.append(re.sub(r"\s+;", " ;", LOCAL.sub(lambda k: k.group(1) + (k.group(2) or ""), l)))
    return chunks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="keep the assembly files in DIR/a and DIR/b")
    ap.add_argument("--only", default="", help="only the units whose name matches this regular expression")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="isa_diff_")
    sides = []
    for tag, root in (("a", args.a), ("b", args.b)):
        os.makedirs(os.path.join(tmp, tag), exist_ok=True)
        sides.append({n: c for n, c in commands(os.path.abspath(root), os.path.join(tmp, tag)).items() if re.search(args.only, n)})
    with concurrent.futures.ThreadPoolExecutor(max_workers=args.jobs) as ex:
        list(ex.map(lambda c: subprocess.run(c[0], check=True, capture_output=True), [c for s in sides for c in s.values()]))
    A, Bs = sides
    bad = 0
    for name in sorted(set(A) - set(Bs)):
        print("%-12s only in %s" % (name, args.a))
    for name in sorted(set(Bs) - set(A)):
        print("%-12s only in %s" % (name, args.b))
    bad += len(set(A) ^ set(Bs))
    n_fun = n_same = 0
    for name in sorted(set(A) & set(Bs)):
        fa, fb = split(A[name][1]), split(Bs[name][1])
        kernels = sum(1 for f in fa.values() if any(x.startswith("\t.amdhsa_kernel") for x in f))
        only = sorted(set(fa) ^ set(fb))
        diff = sorted(f for f in set(fa) & set(fb) if fa[f] != fb[f])
        same = len(set(fa) & set(fb)) - len(diff)
        n_fun += len(set(fa) | set(fb))
        n_same += same
        bad += len(only) + len(diff)
        print("%-12s functions %3d (kernels %3d)  identical %3d  differing %d  in one only %d" % (name, len(fa) - 1, kernels, same - ("<unit>" not in diff), len(diff), len(only)))
        for f in diff:
            print("    differs: %s" % f)
        for f in only:
            print("    only in %s: %s" % (args.a if f in fa else args.b, f))
    print("%d units paired by name, %d functions and unit remainders, %d identical: %s" % (len(set(A) & set(Bs)), n_fun, n_same, "SAME DEVICE CODE" if not bad else "%d DIFFERENCES" % bad))
    if not args.keep:
        shutil.rmtree(tmp)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
