"""CPU: the rule of kmx_unitig_graph (include/kmx.h) restated in plain Python (tests/unitig_links_ref.py) has every consequence
the rule lists on every case, equals its fixture, gives the rows written out here for graphs small enough to read; the GFA
writer of the facade formats them as the restatement does; the driver and the new entry points refuse what they must before
they need a device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import unitig_links_ref as UL
import unitigs_ref as U
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitig_links_golden.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", list(U.CASES))
def test_consequences_and_fixture(name, fixture):
    """out-degrees are the records' n_succ / n_pred, n_links their sum, mirror symmetry, no edge twice, the k - 1 overlap, node
    edges = links inside unitigs + reported edges (UL.check_links); and the two arrays are the fixture's"""
    from make_unitig_links_golden import entry
    computed = UL.case_links(name)
    k, thr, km, cnt, strs, recs, off, lk = computed
    assert off.dtype == np.uint64 and lk.dtype == np.uint32
    UL.check_links(km, cnt, k, thr, strs, recs, off, lk)
    assert entry(name, computed) == fixture[name]


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture) == sorted(U.CASES)
    assert fixture["k5_complete"]["n_links"] == 8 * 512 and fixture["k7_complete"]["n_links"] == 8 * 8192   # link_capacity = 8 * nodes is tight
    for name in ("k7_cycle30", "k5_cycle2", "k33_cycle400"):       # a lone cycle: its closing link, once per orientation
        assert (fixture[name]["unitigs"], fixture[name]["n_links"]) == (1, 2)
    assert fixture["k15_long_path"]["n_links"] == 0 and fixture["reads_thr1"]["n_links"] > 1000


def graph(seqs, k, thr=1):
    km, cnt = U.listing_of(U.count_kmers(seqs, k))
    strs, recs = U.unitigs(km, cnt, k, thr)
    off, lk = UL.flat_links(UL.links(km, cnt, k, thr, strs))
    UL.check_links(km, cnt, k, thr, strs, recs, off, lk)
    return strs, recs, off, lk


def l_lines(text):
    return [line for line in text.splitlines() if line.startswith("L")]


def test_hand_built_homopolymer():
    """AAAAA alone at k = 5: the self-loop, once per orientation"""
    strs, recs, off, lk = graph(["AAAAA"], 5)
    assert strs == ["AAAAA"] and (recs[0]["n_pred"], recs[0]["n_succ"], recs[0]["circular"]) == (1, 1, 0)
    assert UL.rows_of(off, lk) == [[0], [1]]
    assert UL.gfa(strs, recs, off, lk, 5) == "H\tVN:Z:1.0\nS\tu0\tAAAAA\tLN:i:5\tKC:i:1\nL\tu0\t+\tu0\t+\t4M\n"


def test_hand_built_hairpin():
    """a palindromic junction h + rc(h): the last k-mer of h is followed by its own reverse complement; the edge is its own
    mirror and makes one L line"""
    k = 5
    h = "GATTCAG"
    strs, recs, off, lk = graph([h + U.rc(h)], k)
    half = (h + U.rc(h))[:len(h) + k // 2]                         # up to the k-mer that straddles the junction evenly: CAGCT, then rc(CAGCT)
    assert strs in ([half], [U.rc(half)])                          # one unitig: the second half of the sequence is its mirror
    d = 0 if strs[0] == half else 1                                # the orientation that ends at the junction
    rows = UL.rows_of(off, lk)
    assert rows[d] == [d ^ 1] and rows[d ^ 1] == []
    assert (recs[0]["n_succ"], recs[0]["n_pred"]) == ((1, 0) if d == 0 else (0, 1))
    sign = "+-"[d], "+-"[d ^ 1]
    assert l_lines(UL.gfa(strs, recs, off, lk, k)) == [f"L\tu0\t{sign[0]}\tu0\t{sign[1]}\t4M"]


def test_hand_built_y():
    """one path into two: the stem has out-degree 2, each branch in-degree 1, and the mirrors lead back"""
    k = 7
    stem, a, b = "TTGCAGGTCA", "ACCATGAG", "CGTTCACT"
    strs, recs, off, lk = graph([stem + a, stem + b], k)
    assert strs == ["AGGTCAACCATGAG", "AGGTCACGTTCACT", "TGACCTGCAA"]   # the branches as given, the stem reversed
    assert UL.rows_of(off, lk) == [[], [4], [], [4], [], [0, 2]]
    assert [(r["n_pred"], r["n_succ"]) for r in recs] == [(1, 0), (1, 0), (2, 0)]
    rows = UL.rows_of(off, lk)
    ori = UL.oriented(strs)
    o_stem = next(o for o, s in enumerate(ori) if s == stem)
    o_a = next(o for o, s in enumerate(ori) if s == stem[-(k - 1):] + a)
    o_b = next(o for o, s in enumerate(ori) if s == stem[-(k - 1):] + b)
    assert rows[o_stem] == [o_a, o_b]                              # the order of the appended base: A before C
    assert rows[o_a ^ 1] == [o_stem ^ 1] and rows[o_b ^ 1] == [o_stem ^ 1]
    assert rows[o_stem ^ 1] == [] and rows[o_a] == [] and rows[o_b] == []
    deg = sorted(len(r) for r in rows)
    assert deg == [0, 0, 0, 1, 1, 2] and len(lk) == 4
    assert len(l_lines(UL.gfa(strs, recs, off, lk, k))) == 2


def test_hand_built_cycle_of_two():
    """ACACAC at k = 5: ACACA <-> CACAC, a circular unitig of 2 whose closing link is reported once per orientation"""
    strs, recs, off, lk = graph(["ACACAC"], 5)
    assert strs == ["ACACAC"] and (recs[0]["circular"], recs[0]["n_kmers"]) == (1, 2)
    assert UL.rows_of(off, lk) == [[0], [1]]
    assert l_lines(UL.gfa(strs, recs, off, lk, 5)) == ["L\tu0\t+\tu0\t+\t4M"]


def _compile(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), source,
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    return exe


def test_facade_program_and_gfa_writer(tmp_path):
    """tests/facade_unitig_graph.cpp compiles against include/kmodel.hpp as C++11; its GFA writer, which needs no device,
    writes what UL.gfa writes for the program's hand-made graph (a mirror pair once, a hairpin once, a self-loop once, a
    sum_count above 2^32), also under the host sanitizers"""
    strs = ["ACGTACG", "TTTTTGA", "CCCCC"]
    recs = [{"sum_count": 10}, {"sum_count": 3}, {"sum_count": 3 * 2 ** 32}]
    off, lk = [0, 2, 2, 3, 4, 6, 7], [2, 5, 3, 1, 4, 1, 5]
    want = UL.gfa(strs, recs, off, lk, 5)
    assert want == ("H\tVN:Z:1.0\nS\tu0\tACGTACG\tLN:i:7\tKC:i:10\nS\tu1\tTTTTTGA\tLN:i:7\tKC:i:3\nS\tu2\tCCCCC\tLN:i:5\tKC:i:12884901888\n"
                    "L\tu0\t+\tu1\t+\t4M\nL\tu0\t+\tu2\t-\t4M\nL\tu1\t+\tu1\t-\t4M\nL\tu2\t+\tu2\t+\t4M\n")
    src = os.path.join(ROOT, "tests", "facade_unitig_graph.cpp")
    assert subprocess.check_output([_compile(tmp_path, src, "facade_unitig_graph"), "--gfa-only"]).decode() == want
    exe = _compile(tmp_path, src, "facade_unitig_graph_san", extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert subprocess.check_output([exe, "--gfa-only"]).decode() == want


def test_driver_refuses_the_graph_without_unitigs(tmp_path):
    exe = _compile(tmp_path, os.path.join(ROOT, "examples", "kmcex_main.cpp"), "kmcEx")
    for args in (["-G", "-k31"], ["-g", "-G", "-k31"]):
        r = subprocess.run([exe, *args, "in.fa", "out", str(tmp_path)], capture_output=True)
        assert r.returncode == 2 and b"-G" in r.stdout and b"unitigs.gfa" in r.stdout


def test_entry_points_refuse_a_null_handle():
    """argument checks that need no device: every new entry point answers a null handle with KMX_E_ARG"""
    L = api.load_library()
    nu, nb, nl = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    counts = (C.byref(nu), C.byref(nb), C.byref(nl))
    assert L.kmx_unitig_graph(None, 31, None, None, 0, 1, None, 0, None, None, 0, None, None, 0, *counts) == -1
    assert L.kmx_unitig_graph_dev(None, 31, None, None, 0, 1, None, 0, None, None, 0, None, None, 0, *counts) == -1
    assert L.kmx_count_unitig_graph(None, 1, None, 0, None, None, 0, None, None, 0, *counts) == -1
    assert L.kmx_count_unitig_graph_dev(None, 1, None, 0, None, None, 0, None, None, 0, *counts) == -1
    assert L.kmx_unitig_graph_last_phases(None, None, None) == -1
    assert b"null" in L.kmx_last_error()
    assert api.UNITIG_GRAPH_PHASES[:4] == api.UNITIG_PHASES and len(api.UNITIG_GRAPH_PHASES) == 5
