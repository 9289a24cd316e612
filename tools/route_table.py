#!/usr/bin/env python3
"""The pinned shape -> route table (tests/golden/route_table.json) and the route of one shape.

    python tools/route_table.py --write              regenerate the fixture from the library as built
    python tools/route_table.py p=48 n=10000 kind=4 chains=512 knobs=wide2=0     the route of one shape (keys: DEFAULT below)

fmcmc_plan_route needs no GPU: it validates the call, normalises it and runs mh_route.hpp's plan_route.  The cases are a
deterministic sample (no random numbers): a mixed-radix enumeration of AXES walked with a stride co-prime to every axis size,
the hand-written EDGES, and a sub-grid in which every FMCMC_AMD_DEBUG knob appears at its documented values next to the same
case without it.  tests/test_route_host.py imports cases() and route_of() from here.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_table.json")

LINREG, LOGISTIC, IID = 1, 2, 3
DBL_MAX = float(np.finfo(np.float64).max)
N_AXIS = sorted({512 * s + d for s in (1, 2, 4, 6, 8, 10, 12, 16, 20, 40, 48, 96) for d in (-1, 0, 1)}
                | {100, 200, 2500, 5000, 10 ** 4, 2 * 10 ** 4, 10 ** 5})
# (name, values): the order is the order of the digits, least significant first
AXES = [
    ("fam", [LINREG, IID, LOGISTIC]),
    ("p", [0, 1, 3, 4, 5, 7, 8, 11, 12, 15, 16, 49, 50, 62, 63]),
    ("intercept", [1, 0]),
    ("n", N_AXIS),
    ("kind", [1, 2, 3, 4, 5, 6, 7, 8]),
    ("scheme", [0, 1, 2, 3]),            # joint, ordered, random, explicit
    ("fix1", [0, 1]),                    # the first parameter fixed
    ("bounded", [0, 1]),                 # the last parameter bounded
    ("constr", [0, 1]),
    ("bw", [0, 5]),
    ("freq", [1, 2, 8, 9]),
    ("chains", [1, 2, 4, 64, 128, 255, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048, 2049, 4096]),
    ("nsteps", [100, 300000]),           # inside one step window / across several
    ("fed", [0, 1]),
    ("ncu", [256, 128]),
]
DEFAULT = dict(fam=LINREG, p=3, intercept=1, n=10000, kind=1, scheme=0, fix1=0, bounded=0, constr=0, bw=0, freq=1, chains=1024,
               nsteps=100, fed=0, ncu=256, burnin=0, thin=1, ld_rows=0, knobs="")
KEYS = list(DEFAULT)
STRIDE = 1000000007          # a prime beyond every axis size: co-prime to their product
N_SAMPLE = 800
KNOBS = ["streamed=1", "cw=1", "cw=2", "cw=4", "cw=8", "pipe=0", "lat=0", "lat=1", "lat=2", "lat=3", "mfma=0", "shard=0", "shard=1",
         "shard_mfma=0", "wide2=0", "wide2=1", "groups=4", "tiles=0", "window=64", "t10=0", "shadow=0", "speclogit=0", "speclogit=2",
         "specbnd=0", "specmirror=0", "tinymfma=0", "specwide=0", "specp0=0", "turn=0", "bigkhbm=1", "mode=2"]
# knobs the launchers read, not the planner: the table pins that they change no route
LAUNCH_ONLY_KNOBS = ("turn", "mode")


def E(**kw):
    c = dict(DEFAULT)
    c.update(kw)
    return c


def _edges():
    out = []
    # more parameters than a wavefront has lanes (k = p + 2): the LDS form, the HBM form, what validation refuses
    for p, kind in ((63, 1), (126, 1), (126, 6), (131, 3), (132, 3), (181, 4), (182, 4), (254, 4), (254, 1), (255, 1), (126, 7)):
        out.append(E(p=p, kind=kind, chains=64))
    out += [E(p=131, kind=3, freq=2, chains=64), E(p=126, kind=1, scheme=1, chains=64), E(p=126, kind=4, bounded=1, chains=64),
            E(p=126, kind=1, knobs="bigkhbm=1", chains=64), E(p=126, kind=1, fix1=1, chains=64)]
    # the register-resident variants and their neighbours
    for n in (512, 513, 1000, 2048, 2049):
        out.append(E(p=1, n=n))
        out.append(E(p=1, n=n, knobs="pipe=0"))
    for n in (9000, 10240, 10241):
        out.append(E(p=3, n=n, knobs="pipe=0"))
        out.append(E(p=3, n=n, knobs="mfma=0"))
    # the latency forms, one to four chains per compute unit, both families
    for chains in (64, 256, 257, 512, 513, 768, 769, 1024, 1025):
        for fam, p, n in ((LINREG, 3, 10000), (LINREG, 1, 1000), (LINREG, 7, 1000), (LINREG, 12, 1000), (LOGISTIC, 4, 100), (LOGISTIC, 4, 5000),
                          (LOGISTIC, 12, 200)):
            for kind, scheme in ((1, 0), (1, 1), (3, 0), (4, 0)):
                out.append(E(fam=fam, p=p, n=n, chains=chains, kind=kind, scheme=scheme))
    # wide linear models: chain-sharded, observation-sharded (scalar and matrix-core), dataflow; 128 workgroups of four lanes
    for n in (1000, 2500, 5000, 10000, 20000, 24576, 24577, 50000):
        for kind in (1, 4):
            for chains in (64, 256, 512, 1024, 2048):
                out.append(E(p=48, n=n, kind=kind, chains=chains))
    for kn in ("shard=1", "shard_mfma=0", "wide2=0", "wide2=1", "groups=4", "tiles=0", "t10=0", "shard=0"):
        for kind in (1, 4):
            out.append(E(p=48, n=10000, kind=kind, chains=512, knobs=kn))
            out.append(E(p=48, n=5000, kind=kind, chains=256, knobs=kn))
    out += [E(p=30, n=1000, kind=4, chains=64), E(p=60, n=10000, kind=4, chains=512), E(p=62, n=10000, kind=1, chains=512),
            E(p=48, n=10000, kind=4, chains=512, constr=1), E(p=48, n=10000, kind=4, chains=512, bounded=1),
            E(p=16, n=2500, kind=1, chains=256, knobs="shard=1,shard_mfma=0"), E(p=48, n=5000, kind=1, chains=256, knobs="shard=1,shard_mfma=0")]
    # the dataflow form with one chain per compute unit or fewer, and what each knob of the wide forms does to it
    for chains in (2, 3, 37, 255, 256, 257):
        out.append(E(p=20, n=6000, kind=4, chains=chains))
    for kn in ("wide2=0", "groups=4", "tiles=0", "shard_mfma=0", "shard=0", "cw=1"):
        out.append(E(p=20, n=6000, kind=4, chains=256, knobs=kn))
    # the register forms' own knobs: the bounded kernel_ram, the mirror kernels, 8 .. 15 covariates, no covariate, tiny data
    out += [E(kind=4, bounded=1, n=1000), E(kind=4, bounded=1, n=1000, knobs="specbnd=0"),
            E(fam=LOGISTIC, p=4, kind=4, bounded=1, n=1000), E(fam=LOGISTIC, p=4, kind=4, bounded=1, n=1000, knobs="specbnd=0"),
            E(kind=7, n=1000), E(kind=7, n=1000, knobs="specmirror=0"), E(kind=8, n=300, p=12), E(kind=8, n=300, p=12, knobs="specmirror=0"),
            E(kind=3, p=12, n=1000), E(kind=3, p=12, n=1000, knobs="specwide=0"), E(kind=1, p=12, n=1000, chains=256),
            E(kind=1, p=12, n=1000, chains=256, knobs="specwide=0"), E(fam=LOGISTIC, kind=3, p=12, n=200), E(fam=LOGISTIC, kind=3, p=12, n=200, knobs="specwide=0"),
            E(fam=IID, p=0, kind=3, n=1000), E(fam=IID, p=0, kind=3, n=1000, knobs="specp0=0"), E(fam=IID, p=0, kind=7, n=300), E(fam=IID, p=0, kind=7, n=300, knobs="specp0=0"),
            E(kind=1, p=12, n=300), E(kind=1, p=12, n=300, knobs="tinymfma=0"), E(kind=3, p=12, n=300, knobs="specwide=0"),
            E(kind=3, p=12, n=300, knobs="specwide=0,tinymfma=0"), E(kind=8, n=300, p=12, knobs="specmirror=0,tinymfma=0"),
            E(kind=7, n=300, p=15), E(kind=7, n=300, p=15, knobs="tinymfma=0")]
    # the logistic family: chain-sharded, observation-sharded with and without the shadow form, long data
    for n in (1000, 5000, 20000, 100000):
        for chains in (1, 16, 64, 256, 1024, 4096):
            for kind in (1, 3, 4):
                out.append(E(fam=LOGISTIC, p=5, n=n, kind=kind, chains=chains))
    for kn in ("shadow=0", "shard=0", "shard=1", "speclogit=0", "speclogit=2", "turn=0"):
        out.append(E(fam=LOGISTIC, p=5, n=100000, chains=1024, knobs=kn))
        out.append(E(fam=LOGISTIC, p=4, n=100, chains=512, knobs=kn))
    # long data, few chains (linear model)
    for n in (4095, 4096, 20000, 100000, 1000000):
        for chains in (1, 4, 64, 65):
            for p in (3, 7, 12, 48):
                out.append(E(p=p, n=n, chains=chains))
    # the size guards: 32-bit offsets inside a chain's block, barrier epochs, the mirror kernels' stream
    for nsteps in (29999999, 30000000, 100000000, (1 << 28) - 1, 1 << 28, (1 << 30) - 1, 1 << 30):
        out.append(E(nsteps=nsteps, thin=1000, chains=4))
        out.append(E(fam=LOGISTIC, p=4, n=1000, nsteps=nsteps, thin=1000, chains=4))
        out.append(E(p=48, kind=4, nsteps=nsteps, thin=1000, chains=512))
        out.append(E(n=100000, nsteps=nsteps, thin=1000, chains=1))
    out += [E(nsteps=200000000, chains=4), E(nsteps=100000, ld_rows=200000000, chains=4), E(kind=7, nsteps=300000, chains=1024),
            E(kind=7, nsteps=100000, chains=256), E(kind=3, freq=2, nsteps=300000, chains=1024), E(kind=3, freq=2, nsteps=300000, chains=1024, fed=1),
            E(kind=3, freq=8, knobs="window=64"), E(kind=3, freq=8, nsteps=65, knobs="window=64"), E(kind=3, freq=8, nsteps=66, knobs="window=64")]
    # calls fmcmc_validate refuses
    out += [E(burnin=100), E(thin=101), E(chains=0), E(kind=3, bw=5, freq=1, p=126), E(kind=9), E(fam=LOGISTIC, p=0, intercept=0)]
    return out


def cases():
    """The list of cases, each a dict with KEYS.  Deterministic: the fixture records its length and checksum."""
    total = 1
    for _, vals in AXES:
        total *= len(vals)
    sample = []
    for j in range(N_SAMPLE):
        idx, c = (17 + j * STRIDE) % total, dict(DEFAULT)
        for name, vals in AXES:
            c[name] = vals[idx % len(vals)]
            idx //= len(vals)
        sample.append(c)
    out = sample + _edges()
    # the knob sub-grid: knob i on every case of the list so far whose position is i modulo a stride, next to the case without it
    base = [c for c in out if not c["knobs"]]
    step = 2 * len(KNOBS) + 1
    for i, kn in enumerate(KNOBS):
        for c in base[i::step]:
            out.append(dict(c, knobs=kn))
    return out


def checksum(cs):
    return hashlib.sha256(json.dumps([[c[k] for k in KEYS] for c in cs]).encode()).hexdigest()


_DUMMY = np.zeros(8)


def specs(abi, c):
    """(Model, Kernel, Run, keep-alive) of a case.  The data and stream pointers are never read by the plan: a dummy."""
    fam, p, ic = c["fam"], c["p"], c["intercept"]
    k = 2 if fam == IID else p + ic + (1 if fam == LINREG else 0)
    kk = max(k, 1)
    fixed = np.zeros(kk, np.uint8)
    lb, ub = np.full(kk, -DBL_MAX), np.full(kk, DBL_MAX)
    if c["fix1"] and kk >= 2:
        fixed[0] = 1
    if c["bounded"]:
        lb[kk - 1], ub[kk - 1] = -10.0, 10.0
    free = np.flatnonzero(fixed == 0).astype(np.int32)
    one = np.ones(kk)
    keep = [fixed, lb, ub, free, one]
    d = _DUMMY.ctypes.data
    m = abi.Model(fam, p, c["n"], d, d, ic, 1, 0.0)
    kn = abi.Kernel(c["kind"], k, d, one.ctypes.data, lb.ctypes.data, ub.ctypes.data, fixed.ctypes.data, c["scheme"], c["freq"],
                    max(c["bw"], 0), c["bw"], float("inf"), 1e-4, 0.234, 0.0, free.ctypes.data, len(free), 0,
                    d if c["constr"] else None)
    r = abi.Run(c["chains"], c["nsteps"], c["burnin"], c["thin"], 1, 0, 0, 1 if c["fed"] else 0, 0,
                d if c["fed"] else None, d if c["fed"] else None)
    return m, kn, r, keep


def route_of(abi, c):
    """The route line of a case, or `refused=<code> <message>` for a call fmcmc_validate refuses."""
    if os.environ.get("FMCMC_AMD_DEBUG", "") != c["knobs"]:
        if c["knobs"]:
            os.environ["FMCMC_AMD_DEBUG"] = c["knobs"]
        else:
            os.environ.pop("FMCMC_AMD_DEBUG", None)
    m, kn, r, keep = specs(abi, c)
    rc, line = abi.plan_route(m, kn, r, c["ld_rows"], c["ncu"])
    return line if rc == abi.OK else "refused=%d %s" % (rc, abi.last_error())


def table(abi):
    """(cases, lines) with the environment variable restored."""
    before = os.environ.get("FMCMC_AMD_DEBUG")
    try:
        cs = cases()
        return cs, [route_of(abi, c) for c in cs]
    finally:
        os.environ.pop("FMCMC_AMD_DEBUG", None)
        if before is not None:
            os.environ["FMCMC_AMD_DEBUG"] = before


def pack(line):
    """A route line without its keys (they are the same in every line; the fixture holds them once)."""
    return line if line.startswith("refused=") else " ".join(kv.split("=", 1)[1] for kv in line.split(" "))


def unpack(keys, packed):
    return packed if packed.startswith("refused=") else " ".join("%s=%s" % kv for kv in zip(keys, packed.split(" ")))


def load_abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


def main(argv):
    abi = load_abi()
    if argv == ["--write"]:
        cs, lines = table(abi)
        keys = next([kv.split("=", 1)[0] for kv in ln.split(" ")] for ln in lines if not ln.startswith("refused="))
        routes = sorted(set(pack(ln) for ln in lines))
        pos = {r: i for i, r in enumerate(routes)}
        with open(FIXTURE, "w") as f:
            json.dump({"cases": len(cs), "checksum": checksum(cs), "keys": keys, "routes": routes,
                       "index": [pos[pack(ln)] for ln in lines]}, f, separators=(",", ":"))
            f.write("\n")
        print("%d cases, %d routes, %d bytes, sha256 %s" % (len(cs), len(routes), os.path.getsize(FIXTURE),
                                                              hashlib.sha256(open(FIXTURE, "rb").read()).hexdigest()))
        return 0
    c = dict(DEFAULT)
    for a in argv:
        key, _, val = a.partition("=")
        if key not in c:
            print(__doc__)
            return 2
        c[key] = val if key == "knobs" else int(val)
    print(route_of(abi, c))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
