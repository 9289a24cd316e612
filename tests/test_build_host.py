"""fmcmc_amd/build.py without a compiler: which units it builds, and when it builds them again.  The compile and the link are
replaced by functions that record their call and touch the file they would write."""
import os

import pytest

from fmcmc_amd import build as B

# the objects of the library: one per part of a k_*.hip with an FMH_PARTS line, one per other source
OBJECTS = sorted(
    ["k_lat1a", "k_lat1b", "k_lat1c", "k_lat1d", "k_lat2a", "k_lat2b", "k_lat2c", "k_lat2d", "k_lat3a", "k_lat3b",
     "k_lat_l1a", "k_lat_l1b", "k_lat_l1c", "k_lat_l2a", "k_lat_l2b", "k_lat_l2c", "k_lat_l3a", "k_lat_l3b",
     "k_spec_a", "k_spec_n", "k_spec_m", "k_spec_r", "k_spec_w1", "k_spec_w2", "k_spec_w3", "k_spec_w4",
     "k_spec_l1", "k_spec_l2", "k_spec_lw1", "k_spec_lw2", "k_mfma1", "k_mfma2", "k_mfma_ext",
     "k_general", "k_wide", "k_logit0", "k_logit1", "k_logit2", "k_logit3", "k_mfma_ad", "k_wide2", "k_fun",
     "mh_engine", "gelman", "summary", "raftery"])


@pytest.fixture
def fake(monkeypatch):
    """the commands build() would have run: fake.compiled (object names), fake.linked (object lists)"""
    class Rec:
        compiled, linked = [], []

    def compile_(cmd, verbose):
        assert cmd[-2] == "-o" and cmd[0] == B.HIPCC
        open(cmd[-1], "w").close()
        Rec.compiled.append(os.path.basename(cmd[-1]))
        return 0.0

    def link(objs, out, verbose):
        assert all(os.path.exists(o) for o in objs)
        open(out, "w").close()
        Rec.linked.append([os.path.basename(o) for o in objs])

    monkeypatch.setattr(B, "_compile", compile_)
    monkeypatch.setattr(B, "_link", link)
    monkeypatch.setattr(B, "OBJDIR", None)      # (set by the tests: nothing may land in the tree's build/)
    return Rec


def build(tmp_path, monkeypatch, fake, flags):
    monkeypatch.setattr(B, "OBJDIR", str(tmp_path / "build"))
    del fake.compiled[:]
    B.build(out=str(tmp_path / "lib" / "libvariant.so"), extra_flags=flags, jobs=4)
    return sorted(fake.compiled)


def test_units_are_the_46_objects_one_per_part():
    us = B.units()
    assert sorted(B.unit_name(u[2]) for u in us) == OBJECTS and len(OBJECTS) == 46
    assert set(B.HEAVY) <= set(OBJECTS) and len(set(B.HEAVY)) == len(B.HEAVY)
    for src, part, obj, flags in us:
        assert os.path.exists(src) and os.path.dirname(obj) == B.OBJDIR
        if part is None:
            assert flags == [] and B.unit_name(obj) == B.unit_name(src)
        else:
            assert flags == ["-DFMH_PART=" + part] and B.unit_name(obj) == "k_" + part
    # the part names are written in the source only: build.py has them from its FMH_PARTS line
    assert [u[1] for u in us if os.path.basename(u[0]) == "k_mfma.hip"] == ["mfma1", "mfma2", "mfma_ext"]
    assert {os.path.basename(u[0]) for u in us if u[1] is None} == {"k_mfma_ad.hip", "k_wide2.hip", "k_fun.hip", "mh_engine.hip", "gelman.hip",
                                                                    "summary.hip", "raftery.hip"}


def test_a_second_build_with_the_same_flags_compiles_nothing(tmp_path, monkeypatch, fake):
    all_objs = sorted(o + ".o" for o in OBJECTS)
    assert build(tmp_path, monkeypatch, fake, ["-DA"]) == all_objs
    assert sorted(fake.linked[-1]) == all_objs
    assert sorted(os.listdir(str(tmp_path / "build" / "libvariant"))) == sorted(all_objs + [o + ".cmd" for o in all_objs])
    assert build(tmp_path, monkeypatch, fake, ["-DA"]) == []
    assert len(fake.linked) == 2
    assert set(B.build.last_times) == {"_wall"}


def test_other_flags_or_another_hipcc_compile_every_unit_again(tmp_path, monkeypatch, fake):
    all_objs = sorted(o + ".o" for o in OBJECTS)
    assert build(tmp_path, monkeypatch, fake, ["-DA"]) == all_objs
    assert set(B.build.last_times) == set(OBJECTS) | {"_wall"}
    assert build(tmp_path, monkeypatch, fake, ["-DB"]) == all_objs
    assert build(tmp_path, monkeypatch, fake, ["-DB"]) == []
    monkeypatch.setattr(B, "HIPCC", "/somewhere/else/hipcc")
    assert build(tmp_path, monkeypatch, fake, ["-DB"]) == all_objs
    assert build(tmp_path, monkeypatch, fake, ["-DB"]) == []


def test_a_header_newer_than_the_objects_compiles_the_units_that_include_it(tmp_path, monkeypatch, fake):
    build(tmp_path, monkeypatch, fake, ["-DA"])
    hdr = os.path.join(B.CSRC, "mh_lat.hpp")
    includes_it = []
    for src, _part, obj, _flags in B.units(str(tmp_path / "build" / "libvariant")):
        # (no file of the tree is touched: the objects get the times instead, a second after their newest input or ten before the header)
        t = max(os.path.getmtime(f) for f in [src] + sorted(B.unit_deps(src))) + 1
        if hdr in B.unit_deps(src):
            includes_it.append(os.path.basename(obj))
            t = os.path.getmtime(hdr) - 10
        os.utime(obj, (t, t))
    assert sorted(includes_it) == sorted(o + ".o" for o in OBJECTS if o.startswith("k_lat") or o == "mh_engine")
    assert build(tmp_path, monkeypatch, fake, ["-DA"]) == sorted(includes_it)


def test_a_header_included_by_a_header_is_a_dependency_of_every_unit_behind_it():
    # mh_owner.hpp is included by headers only: a unit reaches it through mh_spec.hpp, mh_mfma.hpp or mh_lat.hpp
    hdr = os.path.join(B.CSRC, "mh_owner.hpp")
    assert hdr in B.deps()
    through = {os.path.join(B.CSRC, h) for h in ("mh_spec.hpp", "mh_mfma.hpp", "mh_lat.hpp")}
    reached = set()
    for src in B.sources():
        d = B.unit_deps(src)
        assert (hdr in d) == bool(through & d), src
        if hdr in d:
            reached.add(os.path.basename(src))
    assert {"k_spec.hip", "k_mfma_ad.hip", "k_logit2.hip", "k_mfma.hip", "k_lat.hip"} <= reached
    assert "k_fun.hip" not in reached and "gelman.hip" not in reached


def test_heavy_orders_the_compiles_and_a_stale_name_in_it_raises(tmp_path, monkeypatch, fake):
    build(tmp_path, monkeypatch, fake, ["-DA"])
    monkeypatch.setattr(B, "HEAVY", ("k_fun", "k_spec_m", "gelman"))
    monkeypatch.setattr(B, "OBJDIR", str(tmp_path / "build"))
    del fake.compiled[:]
    B.build(out=str(tmp_path / "lib" / "libvariant.so"), extra_flags=["-DC"], jobs=1)
    assert fake.compiled[:3] == ["k_fun.o", "k_spec_m.o", "gelman.o"] and len(fake.compiled) == 46
    monkeypatch.setattr(B, "HEAVY", ("k_fun", "k_lat9z"))
    with pytest.raises(RuntimeError, match="k_lat9z"):
        B.units()
    with pytest.raises(RuntimeError, match="k_lat9z"):
        B.build(out=str(tmp_path / "lib" / "libvariant.so"), extra_flags=["-DC"], jobs=1)
