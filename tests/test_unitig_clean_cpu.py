"""CPU: the cleaning rule of kmx_unitig_graph_clean (include/kmx.h) restated in plain Python (tests/unitig_clean_ref.py) has the
four consequences the rule lists on every case and every hand-built shape, equals its fixture, and gives the figures the
rule was introduced with; the facade program compiles against include/kmodel.hpp; the driver and the new entry points refuse
what they must before they need a device."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import unitig_clean_ref as CL
import unitigs_ref as U
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_unitig_clean_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitig_clean_golden.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("key", [key for key, (name, how) in G.names().items() if how is not None or not name.startswith("reads")])
def test_consequences_and_fixture(key, fixture):
    """no junction orphaned, the uncleaned capacities suffice, original coordinates and counts, a no-op is exact, and
    UL.check_links on the output (CL.check_clean); statistics, log and the six outputs are the fixture's"""
    k, thr, km, cnt, p, res = G.compute(key)
    CL.check_clean(km, cnt, k, thr, *p, res)
    assert G.entry(k, thr, km, cnt, res) == fixture[key]


def test_fixture_holds_every_case_and_the_quoted_figures(fixture):
    assert sorted(fixture) == sorted(G.names())
    r = fixture["reads_thr1_at_thr2"]                              # 53 unitigs, N50 385 -> one round -> 1 unitig, N50 4980
    assert (r["unitigs_before"], r["n50_before"], r["unitigs_after"], r["n50_after"]) == (53, 385, 1, 4980)
    assert [(e["tips"], e["islands"], e["bubbles"]) for e in r["log"]] == [(15, 7, 5), (0, 0, 0)] and r["stats"]["rounds_run"] == 2
    assert [e["unitigs"] for e in fixture["k7_half_thr3"]["log"]] == [2082, 1039, 908, 891] and fixture["k7_half_thr3"]["stats"]["converged"] == 1
    s = fixture["k11_sparse"]
    assert [e["unitigs"] for e in s["log"]] == [31382, 160, 71] and s["log"][0]["islands"] > 0 and s["log"][1]["tips"] == 0 and s["log"][1]["islands"] > 0
    for name in ("k5_complete", "k7_complete", "k5_loops_hairpins", "k7_cycles_2_32_30_and_line"):
        assert fixture[name]["stats"]["n_kmers_removed"] == 0 and fixture[name]["stats"]["rounds_run"] == 1, name
    assert fixture["k7_tenth"]["thr"] == 1                          # the case's own thr is 0, which the rule refuses


def test_crafted_shapes_do_what_they_are_named_for():
    got = {name: CL.clean_case(name) for name in CL.CLEAN_CASES}
    k, thr, km, cnt, p, res = got["y_two_equal_short_lower_index_survives"]
    strs0, recs0 = U.unitigs(km, cnt, k, thr)
    tips = [u for u, r in enumerate(recs0) if r["n_kmers"] == 10]
    assert len(tips) == 2 and recs0[tips[0]]["sum_count"] == recs0[tips[1]]["sum_count"]
    gone = {u for u, s in enumerate(strs0) if res["removed"][km.index(U.canon(s[:k]))]}
    assert gone == {tips[1]}                                       # equal keys: the lower index survives
    k, thr, km, cnt, p, res = got["y_equal_length_sum_decides"]
    strs0, recs0 = U.unitigs(km, cnt, k, thr)
    tips = sorted((u for u, r in enumerate(recs0) if r["n_kmers"] == 10), key=lambda u: recs0[u]["sum_count"])
    gone = {u for u, s in enumerate(strs0) if res["removed"][km.index(U.canon(s[:k]))]}
    assert recs0[tips[0]]["sum_count"] < recs0[tips[1]]["sum_count"] and gone == {tips[0]}
    res = got["snp_bubble_unequal"][5]
    assert res["stats"]["n_bubbles"] == 1 and res["recs"][0]["min_count"] == 2      # the arm seen once went
    assert got["snp_bubble_equal"][5]["stats"]["n_bubbles"] == 1
    assert got["tip_on_a_cycle_closes_it"][5]["recs"][0]["circular"] == 1
    assert got["tip_of_exactly_max_tip"][5]["stats"]["n_tips"] == 1 and got["tip_of_max_tip_plus_one"][5]["stats"]["n_tips"] == 0
    assert got["stem_merges_three"][5]["recs"] == [{"n_kmers": 169, "sum_count": 507, "min_count": 3, "max_count": 3, "first_node": got["stem_merges_three"][5]["recs"][0]["first_node"],
                                                    "circular": 0, "n_pred": 0, "n_succ": 0, "first_fwd": got["stem_merges_three"][5]["recs"][0]["first_fwd"]}]
    res = got["hairpin_and_self_loop_arms_stay"][5]
    arms = [u for u, r in enumerate(res["recs"]) if CL.arm(r, 2 * 21)]
    assert len(arms) == 2 and all(any(t >> 1 == u for t in res["rows"][2 * u] + res["rows"][2 * u + 1]) for u in arms)
    assert got["k63_y_and_bubble"][5]["stats"]["n_tips"] == 1 and got["k63_y_and_bubble"][5]["stats"]["n_bubbles"] == 1


def test_max_rounds_prefixes_of_the_restatement():
    k, thr, km, cnt = G.listing("k7_half_thr3")
    full = CL.clean(km, cnt, k, thr)
    for mr, conv in ((1, 0), (2, 0), (3, 0), (4, 1)):
        res = CL.clean(km, cnt, k, thr, max_rounds=mr)
        assert (res["stats"]["rounds_run"], res["stats"]["converged"]) == (mr, conv)
        assert res["removed"] == [r if r <= mr else 0 for r in full["removed"]]
        CL.check_clean(km, cnt, k, thr, 7, 2 * k, 2 * k, mr, res)


def _compile(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), source,
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    return exe


def test_facade_program_compiles(tmp_path):
    """tests/facade_unitig_clean.cpp compiles against include/kmodel.hpp as C++11; the part of it that needs no device (the
    sizes of the two structs and the constants) runs"""
    src = os.path.join(ROOT, "tests", "facade_unitig_clean.cpp")
    assert subprocess.check_output([_compile(tmp_path, src, "facade_unitig_clean", extra=("-Wall", "-Werror")), "--compile-only"]).decode() == "ok\n"


def test_driver_refuses_cleaning_without_a_threshold(tmp_path):
    exe = _compile(tmp_path, os.path.join(ROOT, "examples", "kmcex_main.cpp"), "kmcEx")
    for args in (["-g", "-C", "-k31"], ["-g", "-u0", "-C", "-k31"], ["-g", "-u2", "-C0", "-k31"], ["-g", "-u2", "-Cx", "-k31"]):
        r = subprocess.run([exe, *args, "in.fa", "out", str(tmp_path)], capture_output=True)
        assert r.returncode == 2 and b"-C<len>" in r.stdout, args


def test_entry_points_refuse_a_null_handle():
    """argument checks that need no device: every new entry point answers a null handle with KMX_E_ARG"""
    L = api.load_library()
    nu, nb, nl = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    counts = (C.byref(nu), C.byref(nb), C.byref(nl))
    P = api.CleanParams(7, 42, 42, 16)
    assert C.sizeof(api.CleanParams) == 16 and C.sizeof(api.CleanStats) == 64
    assert L.kmx_unitig_graph_clean(None, 31, None, None, 0, 1, C.addressof(P), None, 0, None, None, 0, None, None, 0, *counts, None, None) == -1
    assert L.kmx_unitig_graph_clean_dev(None, 31, None, None, 0, 1, C.addressof(P), None, 0, None, None, 0, None, None, 0, *counts, None, None) == -1
    assert L.kmx_count_unitig_graph_clean(None, 1, C.addressof(P), None, 0, None, None, 0, None, None, 0, *counts, None, None) == -1
    assert L.kmx_count_unitig_graph_clean_dev(None, 1, C.addressof(P), None, 0, None, None, 0, None, None, 0, *counts, None, None) == -1
    assert L.kmx_unitig_clean_last_phases(None, None, None) == -1
    assert b"null" in L.kmx_last_error()
    assert api.UNITIG_CLEAN_PHASES[:5] == api.UNITIG_GRAPH_PHASES and len(api.UNITIG_CLEAN_PHASES) == 6
    assert (api.CLEAN_TIPS, api.CLEAN_ISLANDS, api.CLEAN_BUBBLES, api.CLEAN_MAX_ROUNDS) == (1, 2, 4, 64)


def test_all_twelve_unitig_entry_points_refuse_a_null_handle():
    """one table over the three tiers and their four routes: a null handle is KMX_E_ARG whatever else is given, and neither
    the counters nor the stats are written"""
    L = api.load_library()
    P = api.CleanParams(7, 42, 42, 16)
    for tier, base in enumerate(("unitigs", "unitig_graph", "unitig_graph_clean")):
        for counted in (False, True):
            for dev in (False, True):
                ctr = [C.c_uint64(7) for _ in range(3 if tier else 2)]
                st = api.CleanStats(*[9] * 8)
                args = [None] + ([] if counted else [31, None, None, 0]) + [1] + ([C.addressof(P)] if tier == 2 else []) + [None, 0, None, None, 0]
                args += ([None, None, 0] if tier else []) + [C.byref(c) for c in ctr] + ([None, C.addressof(st)] if tier == 2 else [])
                name = "kmx_" + ("count_" if counted else "") + base + ("_dev" if dev else "")
                assert getattr(L, name)(*args) == -1, name
                assert b"null" in L.kmx_last_error(), name
                assert [c.value for c in ctr] == [7] * len(ctr) and all(getattr(st, f) == 9 for f, _ in api.CleanStats._fields_), name
