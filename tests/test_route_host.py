"""The shape -> route table of mh_route.hpp's plan_route, pinned without a GPU: fmcmc_plan_route validates a call, normalises
it and plans it with no device call.  tests/golden/route_table.json holds the route of every case of tools/route_table.py's
deterministic sample; `python tools/route_table.py --write` regenerates it after a deliberate routing change."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 160 * 1024


def _load_tool():
    spec = importlib.util.spec_from_file_location("route_table", os.path.join(ROOT, "tools", "route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RT = _load_tool()


@pytest.fixture(scope="module")
def abi():
    return RT.load_abi()


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(RT.FIXTURE))


@pytest.fixture(scope="module")
def planned(abi):
    """(cases, lines) as the library plans them now; computed once, read-only."""
    return RT.table(abi)


@pytest.fixture(scope="module")
def pinned(fixture):
    """the fixture's line of every case"""
    return [RT.unpack(fixture["keys"], fixture["routes"][i]) for i in fixture["index"]]


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split(" "))


def kernel_name_tables():
    """The names of kernel_name() in mh_route.hpp: one per Form value, and the register forms by chains per workgroup."""
    src = open(os.path.join(ROOT, "fmcmc_amd", "csrc", "mh_route.hpp")).read()
    body = src[src.index("static const char* kernel_name("):]
    name = re.search(r"name\[\]\s*=\s*\{(.*?)\};", body, flags=re.S).group(1)
    by_cw = re.search(r"by_cw\[4\]\[4\]\s*=\s*\{(.*?)\};", body, flags=re.S).group(1)
    return re.findall(r'"([^"]+)"', name), re.findall(r'"([^"]+)"', by_cw)


def test_the_generator_has_not_drifted(fixture):
    cs = RT.cases()
    assert len(cs) == fixture["cases"] == len(fixture["index"])
    assert RT.checksum(cs) == fixture["checksum"], "tools/route_table.py generates other cases than the fixture was written for"
    assert os.path.getsize(RT.FIXTURE) <= 192 * 1024


def test_every_case_takes_its_pinned_route(planned, pinned):
    cs, lines = planned
    bad = [(c, old, new) for c, old, new in zip(cs, pinned, lines) if old != new]
    for c, old, new in bad[:10]:
        print("case   %s\npinned %s\nnow    %s\n" % (" ".join("%s=%s" % (k, c[k]) for k in RT.KEYS), old, new))
    assert not bad, "%d of %d cases changed their route" % (len(bad), len(cs))


def test_the_table_covers_every_form_and_knob(fixture, pinned):
    cs = RT.cases()
    routes = [fields(ln) for ln in pinned if not ln.startswith("refused=")]
    forms = {r["form"] for r in routes}
    names, by_cw = kernel_name_tables()
    assert len(names) == 19 and len(by_cw) == 16
    # (the register forms report their by_cw name; two forms are only ever set at run time: logistic-shadow by launch_logistic,
    #  long-sharded by try_launch_long once the cooperative launch the plan prepared -- kfn_long -- has run)
    plain = set(names) - {"lat", "lat-logit", "spec", "spec-logit", "logistic-shadow", "long-sharded"}
    assert plain <= forms, sorted(plain - forms)
    for base in ("streamed-logistic", "streamed-wide", "mfma-streamed"):      # the long-data form over both families
        assert any(r["kfn_long"] == "1" and int(r["lcg"]) >= 1 and r["form"] == base for r in routes), base
    assert set(by_cw) <= forms, sorted(set(by_cw) - forms)
    # (no call fmcmc_validate accepts exceeds the LDS: the chain blocks of k <= 64 take at most ~74 KiB at one chain per workgroup
    #  and a sample tile of one row, the big-k forms keep O(k) vectors and at most k (k + 1) doubles of matrices below the 160 KiB
    #  at which the HBM form takes over -- lds_exceeded is a guard, and the table pins that nothing sets it)
    assert not any(r["lds_exceeded"] == "1" or r["no_kernel"] == "1" for r in routes)
    assert "big-k-hbm" in forms and "big-k" in forms
    assert any(ln.startswith("refused=") for ln in pinned)
    # every knob changes the route of a case relative to the same case without it -- except the two the launchers read
    # (turn: logit_shard's timing; mode: SweepArgs.debug), which change none
    unset = {tuple(c[k] for k in RT.KEYS if k != "knobs"): ln for c, ln in zip(cs, pinned) if not c["knobs"]}
    changed, seen = set(), set()
    for c, ln in zip(cs, pinned):
        twin = unset.get(tuple(c[k] for k in RT.KEYS if k != "knobs"))
        if c["knobs"] and "," not in c["knobs"] and twin is not None:
            seen.add(c["knobs"])
            if twin != ln:
                changed.add(c["knobs"])
    assert seen == set(RT.KNOBS)
    launch_only = {kn for kn in RT.KNOBS if kn.split("=")[0] in RT.LAUNCH_ONLY_KNOBS}
    assert changed == set(RT.KNOBS) - launch_only, sorted((set(RT.KNOBS) - launch_only) ^ changed)
    # the knob list is the library's: every name of read_knobs' table appears
    src = open(os.path.join(ROOT, "fmcmc_amd", "csrc", "mh_route.hpp")).read()
    declared = set(re.findall(r"\bX\((\w+), -?\d+\)", src)) or set(re.findall(r'\{"(\w+)", &K\.\w+\}', src))
    assert declared and declared == {kn.split("=")[0] for kn in RT.KNOBS}


def test_invariants_of_every_planned_route(planned):
    cs, lines = planned
    checked = 0
    for c, ln in zip(cs, lines):
        if ln.startswith("refused="):
            continue
        r = fields(ln)
        if r["lds_exceeded"] == "1":
            continue
        checked += 1
        ctx = (c, ln)
        assert int(r["lds"]) <= LDS_MAX and int(r["lds_run"]) <= LDS_MAX, ctx
        # (the fp64-MFMA forms choose their handle per launch: mh_engine.hip, launch_stream_fed)
        assert r["kfn"] == "1" or r["form"] in ("mfma", "mfma-streamed"), ctx
        assert int(r["cw"]) in (1, 2, 4, 8), ctx
        if re.match(r"(lat|lat-logit|spec|spec-logit)(-lat)?\d?$", r["form"]):
            assert int(r["pipe_opt"]) > 0 and int(r["pipe_opt"]) % 2 == 0, ctx
        assert int(r["ch_launch"]) >= 1 or r["form"].startswith("big-k"), ctx
        if "sharded" in r["form"] and r["form"] != "long-sharded" or r["form"] == "wide-dataflow":
            assert int(r["nb_launch"]) in (128, 256), ctx
    assert checked > len(cs) // 2


def test_a_refused_call_is_refused_alike(abi, planned):
    """fmcmc_plan_route returns fmcmc_validate's code and message; neither needs a device."""
    cs, lines = planned
    refused = [(c, ln) for c, ln in zip(cs, lines) if ln.startswith("refused=")]
    assert len(refused) >= 6
    for c, ln in refused:
        m, kn, r, keep = RT.specs(abi, c)
        rc = abi.lib().fmcmc_validate(C.byref(m), C.byref(kn), C.byref(r))
        assert rc != abi.OK
        assert ln == "refused=%d %s" % (rc, abi.last_error()), c
    for c, ln in zip(cs[:50], lines[:50]):
        if not ln.startswith("refused="):
            m, kn, r, keep = RT.specs(abi, c)
            assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kn), C.byref(r)) == abi.OK
    m, kn, r, keep = RT.specs(abi, RT.DEFAULT)
    assert abi.lib().fmcmc_plan_route(C.byref(m), C.byref(kn), C.byref(r), 0, 256, C.create_string_buffer(16), 16) == abi.ERR_ARG
