"""Builds the HIP engine in-tree: fmcmc_amd/lib/libfmcmc_amd.so (gfx950 only).

The library is several translation units compiled in parallel into build/*.o and linked by hipcc (units()): csrc/mh_engine.hip
= C-ABI + launches, with its own headers mh_route.hpp = kernel selection, mh_prep.hpp = data-preparation kernels, mh_host.hpp =
host-pointer staging; the diagnostics csrc/gelman.hip, csrc/summary.hip, csrc/raftery.hip with the header they share,
csrc/diag_common.hpp; and csrc/k_*.hip = one kernel template each.  A k_*.hip whose template has too many instantiations for one
compile names its parts on its FMH_PARTS line (csrc/mh_parts.hpp) and is compiled once per part, with -DFMH_PART=<part> into
build/k_<part>.o.  A unit is recompiled when a file it includes (unit_deps) is newer than its object, or when its command line
is not the one stored beside the object (build/<unit>.o.cmd: other flags, another HIPCC)."""
import concurrent.futures
import glob
import os
import re
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libfmcmc_amd.so")
OBJDIR = os.path.join(HERE, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-Wno-unused-value", "-Wno-unused-result"]
# units by compile time, longest first: the units that instantiate the most kernels decide the wall time when they start last
HEAVY = ("k_lat_l2a", "k_lat_l1a", "k_wide", "k_spec_a", "k_lat2a", "k_lat1a", "k_lat2c", "k_lat_l2b", "k_lat_l1b", "k_lat1c", "k_mfma_ad", "k_spec_l2", "k_spec_w1", "k_spec_w3", "k_spec_lw1", "k_spec_lw2", "k_lat_l3a", "k_lat_l3b", "k_lat3a", "k_lat3b", "k_logit1", "k_lat_l2c", "k_lat_l1c", "k_lat2b", "k_lat1b", "k_lat2d", "k_lat1d", "k_logit2", "k_mfma2", "k_mfma1", "k_general", "k_logit0", "k_spec_r")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def deps():
    return sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))


def parts(src):
    """the part names of a source's FMH_PARTS line; None: the source is one unit"""
    m = re.search(r"^#define FMH_PARTS\(X\)(.*)$", open(src).read(), flags=re.M)
    return re.findall(r"X\((\w+)\)", m.group(1)) if m else None


def unit_name(obj):
    return os.path.splitext(os.path.basename(obj))[0]


def units(objdir=OBJDIR):
    """the translation units of the library: (source, part or None, object path, extra flags)"""
    out = []
    for src in sources():
        ps = parts(src)
        if ps is None:
            out.append((src, None, os.path.join(objdir, unit_name(src) + ".o"), []))
        else:
            out += [(src, p, os.path.join(objdir, "k_%s.o" % p), ["-DFMH_PART=" + p]) for p in ps]
    names = [unit_name(u[2]) for u in out]
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise RuntimeError("two units would share an object: %s" % twice)
    stale = [h for h in HEAVY if h not in names]
    if stale:
        raise RuntimeError("build.HEAVY names no unit: %s" % stale)
    return out


def unit_deps(src, _seen=None):
    """the files a translation unit includes (quoted includes, followed recursively)"""
    seen = _seen if _seen is not None else set()
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(src).read(), flags=re.M):
        f = os.path.normpath(os.path.join(os.path.dirname(src), inc))
        if os.path.exists(f) and f not in seen:
            seen.add(f)
            unit_deps(f, seen)
    return seen


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(f) > t for f in sorted({u[0] for u in units()}) + deps())


def _compile(cmd, verbose):
    """cmd: the compile of one unit, its object last"""
    if verbose:
        print(" ".join(cmd), flush=True)
    t0 = time.time()
    subprocess.check_call(cmd)
    return time.time() - t0


def _link(objs, out, verbose):
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _stored(path):
    return open(path).read() if os.path.exists(path) else None


def build(force=False, verbose=False, extra_flags=(), out=None, jobs=None):
    """extra_flags / out: diagnostic variants next to the product library, loaded through FMCMC_AMD_LIB (e.g. -DFMCMC_STAMP ->
    lib/libfmcmc_amd_stamp.so, tools/stamp_wide.py); their objects go to build/<name of out>/.  Returns the library path;
    build.last_times holds the compile seconds per unit (the object's name without .o) of the last call."""
    out = out or OUT
    if not force and not extra_flags and not needs_build():
        return out
    variant = "" if out == OUT else os.path.splitext(os.path.basename(out))[0]
    objdir = os.path.join(OBJDIR, variant) if variant else OBJDIR
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    todo, objs = [], []
    for src, _part, obj, unit_flags in units(objdir):
        objs.append(obj)
        cmd = [HIPCC] + FLAGS + list(extra_flags) + unit_flags + ["-c", src, "-o", obj]
        dep_t = max(os.path.getmtime(f) for f in [src] + sorted(unit_deps(src)))
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < dep_t or _stored(obj + ".cmd") != "\n".join(cmd):
            todo.append(cmd)
    todo.sort(key=lambda cmd: HEAVY.index(unit_name(cmd[-1])) if unit_name(cmd[-1]) in HEAVY else len(HEAVY))

    def one(cmd):
        if os.path.exists(cmd[-1] + ".cmd"):
            os.remove(cmd[-1] + ".cmd")       # (a compile that fails leaves no object that looks current)
        dt = _compile(cmd, verbose)
        open(cmd[-1] + ".cmd", "w").write("\n".join(cmd))
        return unit_name(cmd[-1]), dt

    jobs = jobs or int(os.environ.get("FMCMC_BUILD_JOBS", "0")) or min(8, os.cpu_count() or 1)
    t0 = time.time()
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        times = dict(ex.map(one, todo))
    _link(objs, out, verbose)
    times["_wall"] = time.time() - t0
    build.last_times = times
    if verbose:
        print("compile seconds per unit:", {k: round(v, 1) for k, v in sorted(times.items())}, flush=True)
    return out


build.last_times = {}

if __name__ == "__main__":
    build(force=True, verbose=True)
