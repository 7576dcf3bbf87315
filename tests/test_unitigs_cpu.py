"""CPU: the unitig rule of include/kmx.h restated in plain Python (tests/unitigs_ref.py) has the properties the rule promises on
every case, equals its fixture, and the library's new entry points refuse bad arguments before they need a device."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import unitigs_ref as U
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitigs_golden.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", list(U.CASES))
def test_properties_and_fixture(name, fixture):
    """every node in exactly one unitig, consecutive k-mers linked, no node twice or in both orientations, links symmetric,
    maximality, the order (U.check), on a listing that is one (strictly ascending, canonical); and the output is the fixture's"""
    from make_unitigs_golden import entry
    k, thr, km, cnt, strs, recs = U.case(name)
    assert all(a < b for a, b in zip(km, km[1:])) and all(len(x) == k and U.canon(x) == x for x in km), "the case is no listing"
    U.check(km, cnt, k, thr, strs, recs)
    got = entry(name)
    assert got == fixture[name]


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture) == sorted(U.CASES)
    for name, e in fixture.items():
        assert e["k"] % 2 == 1 and e["unitigs"] >= 1
    assert fixture["k7_cycle30"]["circular"] == 1 and fixture["k7_cycle30"]["longest"] == 30
    assert fixture["k7_two_cycles_and_line"]["circular"] == 2
    for name, m in (("k5_cycle2", 2), ("k7_cycle2", 2), ("k7_cycle32", 32), ("k9_cycle64", 64)):   # cycles of 2^j nodes
        assert (fixture[name]["unitigs"], fixture[name]["circular"], fixture[name]["longest"]) == (1, 1, m)
    assert fixture["k7_cycle2_and_line"]["circular"] == 1 and fixture["k7_cycles_2_32_30_and_line"]["circular"] == 3
    assert fixture["k15_long_path"]["longest"] > 4096              # more than 12 doubling rounds
    assert fixture["reads_thr1"]["unitigs"] > 100 * fixture["reads_thr3"]["unitigs"]


@functools.lru_cache(maxsize=None)
def case(name):
    """U.case, computed once for the tests below that only read it"""
    return U.case(name)


def shapes(name):
    """(self-loops, hairpin edges, branching nodes) among the nodes of a case, an edge counted once"""
    k, thr, km, cnt, _, _ = case(name)
    g = U.Graph(km, cnt, k, thr)
    loops = hairpins = branching = 0
    for x in g.idx:
        loops += x in g.succ(x)                                # (rc(x) -> rc(x) is the same edge)
        hairpins += (U.rc(x) in g.succ(x)) + (x in g.succ(U.rc(x)))
        branching += len(g.succ(x)) > 1 or len(g.pred(x)) > 1
    return loops, hairpins, branching


DENSE = ("k5_complete", "k5_dense_thr3", "k7_complete", "k7_half_thr1", "k7_half_thr3", "k7_tenth", "k9_dense", "k11_sparse")


def test_dense_cases_hold_what_they_are_for(fixture):
    """the complete graph is the tight case of "rec_capacity = the nodes and seq_capacity = nodes * k always suffice"; the random
    subsets have every local shape, and counts at both ends of their range"""
    e = fixture["k5_complete"]
    assert (e["n"], e["nodes"], e["unitigs"], e["longest"], e["bases"]) == (512, 512, 512, 1, 512 * 5)
    assert fixture["k7_complete"]["n"] == fixture["k7_complete"]["unitigs"] == 4 ** 7 // 2
    assert 35000 < fixture["k11_sparse"]["n"] < 45000
    assert fixture["k7_tenth"]["thr"] == 0 and fixture["k9_dense"]["thr"] == 0xFFFFFFFF
    assert 0 in case("k7_tenth")[3] and fixture["k7_tenth"]["nodes"] == fixture["k7_tenth"]["n"]
    assert 0 < fixture["k9_dense"]["nodes"] < fixture["k9_dense"]["n"] // 3
    loops = hairpins = 0
    recs = []
    for name in DENSE:
        lo, ha, _ = shapes(name)
        loops, hairpins = loops + lo, hairpins + ha
        recs += case(name)[5]
    assert loops >= 1 and hairpins >= 1
    assert any(r["n_kmers"] >= 2 for r in recs) and any(r["first_fwd"] == 0 for r in recs)
    assert any(r["sum_count"] >= 2 ** 32 for r in recs)
    assert any(r["min_count"] == 0 for r in recs) and any(r["max_count"] == 0xFFFFFFFF for r in recs)


@pytest.mark.parametrize("k", [31, 33, 35, 47, 61, 63])
def test_tangles_hold_every_local_shape(k, fixture):
    recs = case(f"tangle_k{k}_thr1")[5]
    loops, hairpins, branching = shapes(f"tangle_k{k}_thr1")
    assert sum(r["circular"] for r in recs) >= 5 and sum(r["first_fwd"] == 0 for r in recs) >= 10
    assert loops >= 1 and hairpins >= 1 and branching >= 20
    assert fixture[f"tangle_k{k}_thr2"]["circular"] >= 1 and fixture[f"tangle_k{k}_thr2"]["longest"] > 100


def test_cycle_cases(fixture):
    """every cycle length from 2 to 130 in one listing; a cycle that exists at one threshold only; one bucket of the index"""
    e = fixture["k31_all_cycles"]
    recs = case("k31_all_cycles")[5]
    assert (e["n"], e["unitigs"], e["circular"]) == (9184, 130, 129)
    assert sorted(r["n_kmers"] for r in recs if r["circular"]) == list(range(2, 131))
    assert [r["n_kmers"] for r in recs if not r["circular"]] == [670]
    assert fixture["cycle_only_above_thr_at1"]["circular"] == 0 and fixture["cycle_only_above_thr_at1"]["nodes"] > 40
    e = fixture["cycle_only_above_thr"]
    assert (e["thr"], e["nodes"], e["unitigs"], e["circular"], e["longest"]) == (2, 40, 1, 1, 40)
    km = case("one_bucket")[2]
    assert sum(x.startswith("A" * 20) for x in km) >= 600 and km[-1].startswith("T" * 13)


@pytest.mark.parametrize("k", [5, 31, 33, 63])
def test_periodic_spells_a_cycle_below_k(k):
    for L in (2, 3, 4, 5, 7, 8, 9):
        s = U.periodic(L, k, L)
        km, cnt = U.listing_of(U.count_kmers([s], k))
        strs, recs = U.unitigs(km, cnt, k, 1)
        U.check(km, cnt, k, 1, strs, recs)
        assert len(s) == L + k - 1 and len(km) == L and [(r["n_kmers"], r["circular"]) for r in recs] == [(L, 1)]


def test_hand_built_graphs():
    """cases small enough to read: a hairpin and a self-loop are edges but never links; a bubble makes four unitigs"""
    k = 5
    # AAAAA -> AAAAA (self-loop) and AAAAC: the homopolymer has two successors and two predecessors
    km, cnt = U.listing_of(U.count_kmers(["AAAAAAC"], k))
    strs, recs = U.unitigs(km, cnt, k, 1)
    U.check(km, cnt, k, 1, strs, recs)
    assert "AAAAA" in strs and all(r["circular"] == 0 for r in recs)
    # ACGTA -> CGTAC -> GTACG = rc(CGTAC): a hairpin, never a link
    km, cnt = U.listing_of(U.count_kmers(["ACGTACG"], k))
    strs, recs = U.unitigs(km, cnt, k, 1)
    U.check(km, cnt, k, 1, strs, recs)
    g = U.Graph(km, cnt, k, 1)
    assert g.succ("CGTAC") == ["GTACG"] and g.link_out("CGTAC") is None
    # a bubble: two paths between the same ends
    a, b = "TTGCAGGTCA", "CCATGAGTTC"
    km, cnt = U.listing_of(U.count_kmers([a + "A" + b, a + "C" + b], 7))
    strs, recs = U.unitigs(km, cnt, 7, 1)
    U.check(km, cnt, 7, 1, strs, recs)
    assert len(strs) == 4
    # thr removes the rarer branch: one unitig
    km, cnt = U.listing_of(U.count_kmers([a + "A" + b, a + "A" + b, a + "C" + b], 7))
    strs, recs = U.unitigs(km, cnt, 7, 2)
    U.check(km, cnt, 7, 2, strs, recs)
    assert strs in ([a + "A" + b], [U.rc(a + "A" + b)]) and recs[0]["min_count"] == 2


def test_pack_round_trip():
    for k in (5, 31, 33, 63):
        km, _ = U.listing_of(U.count_kmers([U.rand_seq(200, k)], k))
        p = U.pack(km, k)
        assert U.unpack(p, k) == km and p.shape == ((len(km),) if k <= 32 else (len(km), 2))
        v = api.UNITIG_DTYPE
        assert v == U.UNITIG_DTYPE and v.itemsize == 40 == C.sizeof(api.Unitig)


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", sizeof(kmx_unitig), '
                   'offsetof(kmx_unitig, first_node), offsetof(kmx_unitig, circular), offsetof(kmx_unitig, first_fwd)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [40, 24, 32, 35]
    assert [api.UNITIG_DTYPE.fields[f][1] for f in ("first_node", "circular", "first_fwd")] == [24, 32, 35]


def test_entry_points_refuse_a_null_handle():
    """argument checks that need no device: every new entry point answers a null handle with KMX_E_ARG"""
    L = api.load_library()
    nu, nb = C.c_uint64(7), C.c_uint64(7)
    assert L.kmx_unitigs(None, 31, None, None, 0, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    assert L.kmx_unitigs_dev(None, 31, None, None, 0, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    assert L.kmx_count_unitigs(None, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    assert L.kmx_count_unitigs_dev(None, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    assert L.kmx_unitigs_last_phases(None, None, None) == -1
    assert b"null" in L.kmx_last_error()


def _compile(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), source,
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    return exe


def test_facade_program_and_fasta_writer(tmp_path):
    """tests/facade_unitigs.cpp compiles against include/kmodel.hpp with the reference's flags; its FASTA writer, which needs
    no device, formats one record per unitig with n_kmers, the mean count and circular (also under the host sanitizers)"""
    want = ">u0 n_kmers=3 mean_count=3.33 circular=0\nACGTACG\n>u1 n_kmers=3 mean_count=1.00 circular=1\nTTTTTGA\n"
    src = os.path.join(ROOT, "tests", "facade_unitigs.cpp")
    assert subprocess.check_output([_compile(tmp_path, src, "facade_unitigs"), "--fasta-only"]).decode() == want
    exe = _compile(tmp_path, src, "facade_unitigs_san", extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert subprocess.check_output([exe, "--fasta-only"]).decode() == want


def test_driver_refuses_unitigs_without_gpu_counting_or_with_even_k(tmp_path):
    exe = _compile(tmp_path, os.path.join(ROOT, "examples", "kmcex_main.cpp"), "kmcEx")
    for args in (["-u2", "-k31"], ["-g", "-u2", "-k30"], ["-g", "-u-5", "-k31"], ["-g", "-ux", "-k31"], ["-g", "-u4294967296", "-k31"]):
        r = subprocess.run([exe, *args, "in.fa", "out", str(tmp_path)], capture_output=True)
        assert r.returncode == 2 and b"-u<thr>" in r.stdout
