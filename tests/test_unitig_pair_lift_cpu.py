"""The plain-Python restatement of the lift rule (tests/unitig_pair_lift_ref.py), checked without a GPU: against a closed form
(window pairs along a known sequence, placed by arithmetic on its unitigs and again on its contigs), on its consequences (a) to
(c) for random lists on random places, on the crafted classes, and on the acceptance case of the GPU test driven end to end
through the restatements, whose preconditions are asserted there."""
import random

import pytest

import unitig_pair_lift_ref as F
import unitig_pair_reduce_ref as X
import unitig_pairs_ref as P
import unitig_scaffold_ref as S

LENS = (21, 22, 42, 60)


@pytest.mark.parametrize("n", (7, 64, 300))
@pytest.mark.parametrize("m", (2, 5))
def test_lift_of_the_unitig_list_is_the_contig_list(n, m):
    """consequence (d) in closed form: every pair is placed by arithmetic at both levels, so every read is one walk and, with
    max_dist above the sequence, no pair is FAR"""
    k, mu, place, cm, upieces, cpieces, n_win = F.chain_pieces(n, 21, LENS, m)
    assert len(cm) > 2 and any(r > 1 for r in (sum(1 for p in place if p[0] >> 1 == c) for c in range(len(cm))))
    r = random.Random(n * 10 + m)
    span = min(n_win - 1, 400)
    pairs = []
    for _ in range(40 * n if n < 300 else 6000):
        p = r.randrange(n_win)
        q = min(n_win - 1, p + r.randrange(span + 1))
        pairs.append((p, q, r.random() < 0.5))
    max_dist = n_win + 1
    up, ulist, _, _, ust = F.window_pairs(k, upieces, 2 * len(mu), pairs, max_dist)
    cp, clist, _, _, cst = F.window_pairs(k, cpieces, 2 * len(cm), pairs, max_dist)
    assert ust["n_far"] == 0 == cst["n_far"] and ust["n_link"] > cst["n_link"] > 0 and cst["n_same"] > ust["n_same"] > 0
    assert ust["n_same"] + ust["n_link"] == len(pairs) == cst["n_same"] + cst["n_link"]
    res = F.check(mu, place, cm, ulist, max_dist)
    assert res["lout"] == clist
    st = res["stats"]
    assert st["n_same_back"] == 0 == st["n_far"] == st["n_inverted"] == st["n_ignored"]
    assert F.same_d(up) + st["sum_same_d"] == F.same_d(cp)
    assert ust["n_same"] + st["pairs_same"] == cst["n_same"] and st["pairs_link"] == cst["n_link"]


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 513))
def test_consequences_on_random_lists_and_places(n):
    for seed, n_contigs, max_dist in ((1, 1, F.ALL), (2, 12, 300), (3, 40, 0), (4, P.CRAFT_U, F.ALL)):
        mu, place, cm, pl = F.random_case(n, seed, n_contigs)
        res = F.check(mu, place, cm, pl, max_dist)
        if n_contigs == 1:
            assert res["stats"]["n_link"] == 0 == res["stats"]["n_far"] and not res["lout"]
    mu = F.random_places(P.CRAFT_U, 5, 9)[0]                       # (a) as the header states it
    pl = S.random_list(n, 5)
    ip, icm = F.identity_place(mu)
    res = F.lift(mu, ip, icm, pl, F.ALL)
    assert res["lout"] == pl and all(r["cls"] == F.LINK and r["shift"] == 0 and r["out"] == i and not r["flipped"] for i, r in enumerate(res["lrec"]))


def test_runs_fold_whatever_their_length():
    mu, place, cm, pl = F.runs_case(F.RUN_EDGES)
    res = F.check(mu, place, cm, pl, F.ALL)
    assert len(pl) == 513 and res["stats"]["n_link"] == 513 and [sum(1 for r in res["lrec"] if r["out"] == i) for i in range(res["stats"]["n_out"])] == list(F.RUN_EDGES)
    got = F.lift(*F.runs_case(F.RUN_EDGES, mirror_run=12)[:3], F.runs_case(F.RUN_EDGES, mirror_run=12)[3], F.ALL)
    assert got["lout"] == res["lout"] and sum(r["flipped"] for r in got["lrec"]) == F.RUN_EDGES[12]


def test_every_class_by_hand():
    for unplaced in (True, False):
        mu, place, cm, pl, want = F.classes_case(unplaced)
        res = F.check(mu, place, cm, pl, F.CLASSES_MAX_DIST, canonical=False)
        assert [r["cls"] for r in res["lrec"]] == want
        st = res["stats"]
        assert (st["n_same"], st["n_same_back"], st["n_far"], st["n_out"]) == (3, 1, 2, 3)
        assert res["lout"] == [(0, 2, 9, 740, 60, 110), (1, 2, 2, 90, 55, 35), (2, 4, 5, 6, 0, 2)]      # a mirror folded, min > max kept, the sums wrapped
        assert st["sum_same_d"] == 90 + 3 * 21 + 10 + 2 * 1
    for max_dist, n_link in ((0, 1), (1, 2), (54, 2), (55, 3), (59, 3), (60, 4), (90, 5), (139, 5), (140, 6), (F.ALL, 6)):    # lo = 0, 1, 55, 60, 90, 140
        assert F.lift(mu, place, cm, pl, max_dist)["stats"]["n_link"] == n_link, max_dist


@pytest.mark.parametrize("seed,holes", X.ISLAND_CASES)
def test_the_acceptance_case_through_the_restatements(seed, holes):
    """three islands, each cut into pieces: the lifted list is the list of the pairs mapped onto the three contigs, the SAME sums
    agree, and the scaffold of the lifted list after the reduction spells the genome with the holes as N"""
    c = F.islands_lifted(seed, holes)
    res, ctg = c["lifted"], c["ctg"]
    assert res["lout"] == c["clist"] and len(c["clist"]) == 3
    assert F.same_d(c["upairs"]) + res["stats"]["sum_same_d"] == F.same_d(c["cpairs"]) and res["stats"]["n_same_back"] == 0
    red = X.reduce(c["cm"], res["lout"], **X.ISLAND_PAR)
    sc = S.scaffold(c["k"], ctg["cstrs"], None, red["lout"], **X.SCAFFOLD_PAR)
    assert len(sc["sstrs"]) == 1
    s = sc["sstrs"][0] if sc["sstrs"][0][:50] == c["genome"][:50] else S.oriented(sc["sstrs"][0], 1)
    assert len(s) == X.ISLAND_GENOME and all(x == g for x, g in zip(s, c["genome"]) if x != "N") and all(s[lo:hi] == "N" * (hi - lo) for lo, hi in holes)
    assert F.lift_tsv(c["ulist"], res).count("\n") == len(c["ulist"])


def test_facade_writer(tmp_path):
    """tests/facade_unitig_pair_lift.cpp compiles against include/kmodel.hpp with the reference's flags; its writer, which needs no
    device, gives the restatement's text for a hand-made result (also under the host sanitizers)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    plinks = [(0, 4, 61, 3660, 60, 60), (0, 6, 21, 3990, 190, 190), (3, 9, 7, 70, 10, 10), (5, 5, 0, 0, 0, 0), (8, 2, 1, 5, 5, 5)]
    rec = lambda c, out, a, b, shift, fl: {"cls": c, "out": out, "A": a, "B": b, "shift": shift, "flipped": fl}
    res = {"lrec": [rec(F.LINK, 2, 7, 4, 160, 1), rec(F.SAME, F.NO_OUT, 0, 0, -33, 0), rec(F.FAR, F.NO_OUT, 1, 9, 4000000000, 0), rec(F.IGNORED, F.NO_OUT, 0, 0, 0, 0),
                    rec(F.INVERTED, F.NO_OUT, 6, 7, 0, 0)]}
    text = F.lift_tsv(plinks, res)
    assert text.splitlines()[0] == "0\tu0+\tu2+\t61\tLINK\tc3-\tc2+\t160\t2" and text.splitlines()[1] == "1\tu0+\tu3+\t21\tSAME\tc0+\tc0+\t-33\t*" and text.splitlines()[3].endswith("IGNORED\t*\t*\t0\t*")
    for name, extra in (("plain", ()), ("san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "facade_unitig_pair_lift.cpp"),
                               "-L" + os.path.join(root, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(root, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--text-only"]).decode() == text, name


def test_entry_points_refuse_a_null_handle():
    import ctypes as C
    from kmcex_amd import api
    from kmcex_amd.api import PairLiftParams, PairLiftStats
    L = api.load_library()
    n, par, st = C.c_uint64(0), PairLiftParams(300, 0), PairLiftStats()
    off = (C.c_uint64 * 1)(0)
    assert L.kmx_unitig_pair_lift(None, 21, off, 0, None, None, 0, None, 0, C.byref(par), None, None, 0, C.byref(n), C.byref(st)) == -1
    assert L.kmx_unitig_pair_lift_dev(None, 21, off, 0, 0, None, None, 0, None, 0, C.byref(par), None, None, 0, C.byref(n), C.byref(st)) == -1
    assert L.kmx_unitig_pair_lift_fold_variant(None, 0) == -1 and L.kmx_unitig_pair_lift_last_phases(None, None) == -1
    assert C.sizeof(PairLiftStats) == 128 and C.sizeof(PairLiftParams) == 8 and api.PAIR_LIFT_DTYPE.itemsize == 32 == F.PAIR_LIFT_DTYPE.itemsize
