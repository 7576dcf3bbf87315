"""CPU: the plain-Python restatement of kmx_unitig_contigs (tests/unitig_contigs_ref.py) equals its golden digests and satisfies the
consequences include/kmx.h states, on every case and parameter pair the GPU tests compare the library with: the no-op, a contig
as a path of the node graph, mirror invariance, place as the inverse of steps; the strings against an independent spelling; the
cut cases against the sequence they were cut from; the record layouts; the text the facade and the driver write."""
import json
import os

import numpy as np
import pytest

import unitig_contigs_ref as G
import unitig_walk_ref as W
import unitigs_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitig_contigs_golden.json")) as f:
        return json.load(f)


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture["listed"]) == sorted(G.LISTED_CASES)
    assert len(fixture["cut"]) == 2 * len(G.CUT_K) * len(G.CUT_N)
    assert set(W.WALK_CASES) <= set(G.LISTED_CASES) and G.RING in G.LISTED_CASES


@pytest.mark.parametrize("name", G.LISTED_CASES)
def test_restatement_equals_golden_and_keeps_its_promises(name, fixture):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    g = fixture["listed"][name]
    assert (g["k"], g["n_unitigs"], g["n_links"]) == (k, len(strs), sum(map(len, rows)))
    for which in ("exact", "bridged"):
        hits = list(G.hits_of(name, which))
        assert g["hits"][which] == sum(hits)
        for pair in G.PARAMS:
            res = G.want(name, which, *pair)
            assert g[f"{which} {pair[0]},{pair[1]}"] == [res["stats"][f] for f in G.STAT_FIELDS] + [G.digest(res)]
            G.check(k, strs, recs, rows, res, noop=pair == (0, 0))   # consequences (a), (b), (d)
            for c, r in zip(res["cstrs"], res["crecs"]):             # the strings, spelled independently
                mine = res["steps"][r["first_step"]:r["first_step"] + r["n_steps"]]
                assert c == G.rc_spelled(strs, mine, k) == W.spell(strs, mine, k)
            mirrored = G.contigs(k, strs, recs, rows, G.mirrored_hits(rows, hits), *pair)
            assert mirrored == res, "consequence (c): the hits of every edge on its mirror instead change nothing"
            flat = G.flat(res)
            assert flat[2].dtype.itemsize == 64 and flat[4].dtype.itemsize == 8 and len(flat[8]) == 8
            if recs is not None:
                without = G.contigs(k, strs, None, rows, hits, *pair)
                assert [dict(r, sum_count=0, min_count=0, max_count=0) for r in res["crecs"]] == without["crecs"] and without["steps"] == res["steps"]


def test_the_figures_of_the_cases():
    """what makes the cases worth running: merges, reverse steps, the ratio path, cycles of one and of two steps"""
    t = G.want("k31_tangle", "exact", 2, 0)
    assert (len(G.listed_case("k31_tangle")[4]), t["stats"]["n_links"], t["stats"]["n_contigs"], t["stats"]["n_multi"]) == (103, 228, 64, 7)
    assert max(r["n_steps"] for r in t["crecs"]) == 14 and sum(o & 1 for o in t["steps"]) == 24
    c = G.want("k5_complete", "exact", 1, 0)["stats"]
    assert (c["n_links"], c["n_contigs"], c["n_multi"]) == (4096, 392, 46)
    e = G.want("k21_every_kind", "exact", 2, 4)
    assert (e["stats"]["n_links"], e["stats"]["n_contigs"], e["stats"]["n_below_ratio"], max(r["n_steps"] for r in e["crecs"])) == (52, 13, 24, 10)
    e0 = G.want("k21_every_kind", "exact", 2, 0)["stats"]
    assert (e0["n_contigs"], e0["n_below_ratio"]) == (25, 0)         # the ratio path is exercised by (2, 4) alone
    a = G.want("k31_all_cycles", "exact", 1, 0)
    assert len(G.listed_case("k31_all_cycles")[4]) == 130 and a["stats"]["n_links"] == 258
    assert [r["n_steps"] for r in a["crecs"] if r["circular"]] == [1] * 10
    for name in ("k33_cycle400", "k21_cycle_and_tip"):
        one = G.want(name, "exact", 1, 0)
        assert [(r["circular"], r["n_steps"]) for r in one["crecs"]] == [(1, 1)]
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(G.RING)
    ring = G.want(G.RING, "exact", 1, 0)
    assert (k, len(strs), sum(map(len, rows)), len(reads)) == (21, 4, 8, 42)
    assert ring["stats"]["n_contigs"] == 3 and [(r["circular"], r["n_steps"]) for r in ring["crecs"] if r["n_steps"] > 1] == [(1, 2)]
    assert sorted(len(s) for s in ring["cstrs"]) == [60, 60, 320]  # the two tips and the ring of 300, spelled open


@pytest.mark.parametrize("ring", (False, True), ids=("line", "ring"))
@pytest.mark.parametrize("k", G.CUT_K)
def test_cut_cases_give_back_the_sequence(k, ring, fixture):
    for n in G.CUT_N:
        kk, strs, rows, hits, text = G.cut_case(n, k, ring)
        res = G.want_cut(n, k, ring)
        assert fixture["cut"][f"{'ring' if ring else 'line'} k{k} n{n}"] == [len(res["cstrs"][0]), sum(o & 1 for o in res["steps"]), G.digest(res)]
        G.check(k, strs, None, rows, res, node_graph=False)
        assert len(res["cstrs"]) == 1 and res["crecs"][0]["circular"] == int(ring) and res["crecs"][0]["n_steps"] == n
        assert res["cstrs"][0] == G.cut_expected(n, k, ring) == G.rc_spelled(strs, res["steps"], k)
        if not ring or res["steps"][0] == 0 and strs[0] == text[:len(strs[0])]:
            assert res["cstrs"][0] == text
        else:                                                    # the reverse complement of the ring read from unitig 1 on, spelled open
            total = len(text) - k + 1
            twice = U.rc(res["cstrs"][0])[:total] * 2
            assert text[:total] in twice and res["steps"][0] == 0
        assert G.contigs(k, strs, None, rows, G.mirrored_hits(rows, hits), 1, 0) == res
        assert sum(o & 1 for o in res["steps"]) in (n // 2, n - n // 2)
        if n > 1:
            assert len({len(s) for s in strs}) > 1 or n < 4
    k_, strs, rows, hits, text = G.cut_case(1000, k, ring)
    assert sum(len(s) for s in strs) > 200 * 4096 // 4            # hundreds of emit tiles


def test_support_rules_on_a_graph_built_by_hand():
    """a hairpin counts its hits once and is never a chain link; min_reads and ratio drop what they say, symmetrically; a contig's
    record and the contig graph on four unitigs"""
    k = 5
    strs = ["ACGTAC", "CGTACG", "GTACGT", "TTTTTA"]                 # the bytes do not matter to the verdicts, and the overlaps do not hold
    rows = [[2, 4], [0], [], [1], [6], [1], [], [5]]                # 0 -> 2 | 3 -> 1, 0 -> 4 | 5 -> 1, 4 -> 6 | 7 -> 5, and the hairpin 1 -> 0
    loff = G.offsets_of(rows)
    e = lambda a, b: loff[a] + rows[a].index(b)
    assert G.mirror_index(rows, loff, 1, 0) == e(1, 0) and G.mirror_index(rows, loff, 0, 1) == e(5, 1)
    hits = [0] * loff[-1]
    hits[e(0, 2)], hits[e(3, 1)], hits[e(0, 4)], hits[e(5, 1)], hits[e(4, 6)], hits[e(7, 5)], hits[e(1, 0)] = 40, 2, 1, 0, 3, 4, 5
    sup = G.support(rows, hits)
    assert [sup[e(*x)] for x in ((0, 2), (3, 1), (0, 4), (5, 1), (4, 6), (7, 5), (1, 0))] == [42, 42, 1, 1, 7, 7, 5]
    res = G.contigs(k, strs, None, rows, hits, 2, 0)
    G.check(k, strs, None, rows, res, overlaps_hold=False)
    assert res["stats"] == {"n_links": 7, "n_kept": 5, "n_below_min": 2, "n_below_ratio": 0, "n_chain": 4, "n_contigs": 2, "n_circular": 0, "n_multi": 2}
    assert res["steps"] == [0, 2, 4, 6] and res["place"] == [(0, 0), (0, 2), (2, 0), (2, 2)]
    assert [(r["n_kmers"], r["n_pred"], r["n_succ"], r["min_support"], r["sum_support"]) for r in res["crecs"]] == [(4, 1, 0, 42, 42), (4, 0, 0, 7, 7)]
    assert res["crows"] == [[], [(0, 5)], [], []]                    # the hairpin, one level up: the mirror of contig 0 runs into contig 0
    assert res["cstrs"] == ["ACGTAC" + "CG", "GTACGT" + "TA"]      # a later step without its first k - 1 bytes, whatever they are
    by_ratio = G.contigs(k, strs, None, rows, hits, 0, 6)          # 7 * 6 = 42 is not below a best of 42; 1 * 6 is, from either side
    assert by_ratio["stats"]["n_below_ratio"] == 2 and by_ratio["stats"]["n_below_min"] == 0 and by_ratio["steps"] == res["steps"]
    assert G.contigs(k, strs, None, rows, hits, 0, 5)["stats"]["n_below_ratio"] == 2 and G.contigs(k, strs, None, rows, hits, 0, 42)["stats"]["n_below_ratio"] == 0
    none = G.contigs(k, strs, None, rows, hits, 0, 0)
    assert none["stats"]["n_chain"] == 2 and none["steps"] == [0, 2, 4, 6] and [r["n_steps"] for r in none["crecs"]] == [1, 1, 2]


def test_texts():
    name = G.RING
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    res = G.want(name, "exact", 1, 0)
    tsv = G.paths_tsv(res).splitlines()
    assert len(tsv) == len(strs) and tsv[0].split("\t")[:2] == ["c0", "0"]
    assert {x.split("\t")[2] for x in tsv} == {f"u{u}" for u in range(len(strs))}
    fa = G.fasta(res).splitlines()
    assert len(fa) == 2 * len(res["cstrs"]) and fa[0].startswith(">c0 ") and fa[1] == res["cstrs"][0]
    gfa = G.gfa(res, k).splitlines()
    assert gfa[0] == "H\tVN:Z:1.0" and sum(x.startswith("S\t") for x in gfa) == 3 and not any(x.startswith("P\t") for x in gfa)
    assert sum(x.startswith("L\t") for x in gfa) == 1 and all(x.split("\t")[5] == "20M" for x in gfa if x.startswith("L\t"))
    full = G.gfa(res, k, strs, recs).splitlines()
    assert sum(x.startswith("S\t") for x in full) == 7 and sum(x.startswith("P\t") for x in full) == 3
    two = [x for x in full if x.startswith("P\t") and "," in x.split("\t")[2]]
    assert len(two) == 1 and two[0].split("\t")[3] == "20M"
