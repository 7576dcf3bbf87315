"""CPU: the plain-Python restatement of kmx_unitig_pair_walks (tests/unitig_pairs_ref.py) satisfies the consequences include/kmx.h
states, on the cases the GPU tests compare the library with; the structs of kmx.h are laid out as the ctypes and NumPy mirrors
say; the facade's two writers give the restatement's text; and the two end-to-end cases come out as the rule promises: every pair
of a genome that is one unitig is SAME with the true fragment length, and the pairs across a gap in the coverage are LINKs whose
distance is the gap's."""
import ctypes as C
import os
import subprocess

import pytest

import unitig_pairs_ref as P
import unitigs_ref as U
from kmcex_amd import api
from kmcex_amd.api import PAIR_CLASSES, PAIR_DTYPE, PAIR_LINK_DTYPE, Pair, PairLink, PairParams, PairStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_pairs", P.CRAFT_SIZES)
def test_consequences_on_crafted_walks(n_pairs):
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    walks, wo, steps = P.crafted(n_pairs, 100 + n_pairs)
    seen = set()
    for params in P.CRAFT_PARAMS:
        pairs, plinks, hist, hits, st = P.check(k, mu, walks, wo, steps, rows, params)
        seen |= {r["cls"] for r in pairs}
        if n_pairs >= 255 and params == P.CRAFT_PARAMS[0]:
            assert st["n_negative"] > 0 and hist[-1] > 0 and st["n_adjacent"] > 0 and st["n_far"] > 0 and 0 < st["n_adjacent"] < st["n_link"]
            fourth = [r for r in pairs if r["edge"] != P.NO_EDGE and rows[r["oa"]].index(r["ob"]) == 3]
            assert fourth, "a target in the fourth entry of a row"
            ends = {r["oa"] >> 1 for r in pairs if r["cls"] == P.LINK} | {r["ob"] >> 1 for r in pairs if r["cls"] == P.LINK}
            assert {0, P.CRAFT_U - 1} <= ends
            assert any((r["oa"], r["ob"]) != P.canonical(r["oa"], r["ob"]) for r in pairs if r["cls"] == P.LINK)
            assert any((r["oa"], r["ob"]) == P.canonical(r["oa"], r["ob"]) for r in pairs if r["cls"] == P.LINK)
    if n_pairs >= 255:
        assert seen == set(range(6))


def test_anchor_rule():
    """the largest n_mapped wins, a tie goes to the lowest index, and a walk below min_mapped, without steps, with a last step
    >= 2 U or an off_last >= m_u is no candidate"""
    mu = [10, 3]
    w = P.a_walk
    steps = [0, 2, 2, 9, 1]
    walks = [w(5, 5, 0, 1, 4), w(8, 8, 1, 1, 2), w(8, 8, 2, 1, 1), w(50, 9, 3, 1, 0), w(60, 9, 4, 0, 0), w(70, 9, 0, 1, 10), w(3, 3, 4, 1, 9)]
    assert P.anchor(mu, walks, steps, 0, 7, 4) == (1, 2, 2, 8)
    assert P.anchor(mu, walks, steps, 2, 7, 4) == (2, 2, 1, 8)
    assert P.anchor(mu, walks, steps, 3, 7, 4) is None and P.anchor(mu, walks, steps, 3, 7, 3) == (6, 1, 9, 3)
    assert P.anchor(mu, walks, steps, 0, 0, 0) is None


def test_far_at_the_threshold_and_the_histogram_edges():
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    oa, ob = 2 * 3, 2 * 4                                       # m = 64 and 300
    walks, wo, steps = P.key_pairs([(oa, ob)], [50])
    for max_dist, cls in ((50, P.LINK), (49, P.FAR)):
        pairs, plinks, hist, hits, st = P.pair_walks(k, mu, walks, wo, steps, rows, 1, max_dist, 1, 1)
        assert pairs[0]["cls"] == cls and pairs[0]["d"] == 50 and len(plinks) == (cls == P.LINK)
    same = [P.a_walk(30, 30, 0, 1, 10), P.a_walk(30, 30, 1, 1, mu[4] - 1 - 20)]
    for bw, nb, want in ((1, 1, [1]), (10, 8, [0] * 7 + [1]), (10, 9, [0] * 8 + [1]), (100, 2, [1, 0])):
        pairs, plinks, hist, hits, st = P.pair_walks(k, mu, same, [0, 1, 2], [8, 9], rows, 1, 0, bw, nb)
        assert pairs[0]["cls"] == P.SAME and pairs[0]["d"] == 10 and pairs[0]["frag"] == 10 + 60 + k - 2 == 89 and hist == want
    neg = [P.a_walk(30, 0, 0, 1, 200), P.a_walk(30, 0, 1, 1, mu[4] - 1 - 20)]
    pairs, plinks, hist, hits, st = P.pair_walks(k, mu, neg, [0, 1, 2], [8, 9], rows, 1, 0, 1, 1)
    assert pairs[0]["frag"] == -180 + k - 2 and st["n_negative"] == 1 == st["n_same"] and hist == [0]


def test_merges():
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    (w1, o1, s1), (w2, o2, s2) = P.merge_case()
    par = (1, 2 ** 32 - 1, 10, 4)
    _, l1, _, _, st1 = P.pair_walks(k, mu, w1, o1, s1, rows, *par)
    assert len(l1) == 5000 and st1["n_link"] == 8000 == st1["n_pairs"]
    _, l11, _, _, _ = P.pair_walks(k, mu, w1, o1, s1, rows, *par, plinks=l1)          # every new key is already in the list
    assert [x[:2] for x in l11] == [x[:2] for x in l1] and all(b[2] == 2 * a[2] and b[3] == 2 * a[3] and b[4:] == a[4:] for a, b in zip(l1, l11))
    _, l12, _, _, st2 = P.pair_walks(k, mu, w2, o2, s2, rows, *par, plinks=l1)         # none is
    assert len(l12) == 5700 and st2["n_link"] == 700 and {x[:2] for x in l1} < {x[:2] for x in l12}


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(PairParams) == 16 and C.sizeof(Pair) == 64 == PAIR_DTYPE.itemsize and C.sizeof(PairLink) == 32 == PAIR_LINK_DTYPE.itemsize
    assert C.sizeof(PairStats) == 80 and [f for f, _ in PairStats._fields_] == list(P.STAT_FIELDS)
    assert PAIR_DTYPE == P.PAIR_DTYPE and PAIR_LINK_DTYPE == P.PAIR_LINK_DTYPE
    pf, lf = [f for f, _ in Pair._fields_], [f for f, _ in PairLink._fields_]
    assert pf == list(P.PAIR_DTYPE.names) and lf == list(P.PAIR_LINK_DTYPE.names)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu", sizeof(kmx_pair_params), sizeof(kmx_pair), sizeof(kmx_pair_link), '
                   'sizeof(kmx_pair_stats));\n' + "".join(f' printf(" %zu", offsetof(kmx_pair, {f}));\n' for f in pf) + "".join(f' printf(" %zu", offsetof(kmx_pair_link, {f}));\n' for f in lf)
                   + ' printf(" %zu %zu", offsetof(kmx_pair_params, n_bins), offsetof(kmx_pair_stats, reserved));\n'
                   + ' printf(" %d %d %d %d %d %d %d\\n", KMX_PAIR_NONE, KMX_PAIR_SINGLE, KMX_PAIR_SAME, KMX_PAIR_INVERTED, KMX_PAIR_LINK, KMX_PAIR_FAR, KMX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [16, 64, 32, 80]
    assert got[4:4 + len(pf)] == [PAIR_DTYPE.fields[f][1] for f in pf] == [getattr(Pair, f).offset for f in pf] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56]
    assert got[4 + len(pf):4 + len(pf) + len(lf)] == [PAIR_LINK_DTYPE.fields[f][1] for f in lf] == [getattr(PairLink, f).offset for f in lf] == [0, 4, 8, 16, 24, 28]
    assert got[-9:] == [12, 72, P.NONE, P.SINGLE, P.SAME, P.INVERTED, P.LINK, P.FAR, 5] and sorted(PAIR_CLASSES) == list(range(6))
    assert "kmx_unitig_pair_walks" in api.ABI_SYMBOLS and "kmx_unitig_pair_walks_dev" in api.ABI_SYMBOLS
    assert all(callable(getattr(api.KModel, f)) for f in ("unitig_pairs_flat", "unitig_pairs_dev", "seq_to_pairs"))


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    n, par, st = C.c_uint64(0), PairParams(1, 100, 10, 10), PairStats()
    assert L.kmx_unitig_pair_walks(None, None, 0, None, 0, None, 0, None, None, 0, C.byref(par), None, None, None, None, 0, C.byref(n), C.byref(st)) == -1
    assert L.kmx_unitig_pair_walks_dev(None, None, 0, None, 0, None, 0, None, None, 0, C.byref(par), None, None, None, None, 0, C.byref(n), C.byref(st)) == -1
    assert b"null" in L.kmx_last_error()


def test_facade_writers(tmp_path):
    """tests/facade_unitig_pairs.cpp compiles against include/kmodel.hpp with the reference's flags; its two writers, which need no
    device, give the restatement's text for a hand-made list and histogram (also under the host sanitizers)"""
    rows = [[2, 5], [], [0, 1, 3, 4, 7], [6], [], [], [], []]
    plinks = [(0, 5, 3, 100, 10, 60), (1, 6, 1, 0, 0, 0), (2, 7, 7, 31, 1, 9), (2, 4, 2 ** 33, 2 ** 35 + 5, 0, 4000000000), (3, 6, 2, 5, 2, 3)]
    hist = [0, 5, 0, 2 ** 40, 1]
    text = P.links_tsv(plinks, rows) + "#\n" + P.insert_tsv(hist, 25)
    assert text.splitlines()[0] == "u0+\tu2-\t3\t33.3\t10\t60\t1" and text.splitlines()[2] == "u1+\tu3-\t7\t4.4\t1\t9\t-" and text.endswith("100\t1\n")
    for name, extra in (("facade_unitig_pairs", ()), ("facade_unitig_pairs_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_pairs.cpp"),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--tsv-only"]).decode() == text, name


def test_one_unitig_every_pair_is_same_with_the_true_fragment():
    """consequence (d): k = 21, a random genome of 3000 bases, a fragment of 400 from every position, reads of 100"""
    k, km, cnt, strs, reads, rows, genome = P.case("one_unitig")
    assert len(strs) == 1 and len(reads) == 2 * 2601 and all(len(r) == 100 for r in reads)
    walks, wo, steps = P.walked("one_unitig")
    mu = [len(s) - k + 1 for s in strs]
    pairs, plinks, hist, hits, st = P.check(k, mu, walks, wo, steps, rows, P.READ_PARAMS)
    assert st["n_same"] == st["n_pairs"] == 2601 and not plinks and not hits
    assert all(r["cls"] == P.SAME and r["frag"] == 400 and r["d"] == 221 for r in pairs)
    assert hist[40] == 2601 and sum(hist) == 2601


def test_two_islands_the_pairs_across_the_gap_are_links_at_its_distance():
    k, km, cnt, strs, reads, rows, genome = P.case("two_islands")
    assert {min(x, U.rc(x)) for x in strs} == {min(x, U.rc(x)) for x in (genome[:950], genome[1050:])} and len(strs) == 2
    assert not any(rows)
    starts = P.kept_starts()
    walks, wo, steps = P.walked("two_islands")
    mu = [len(s) - k + 1 for s in strs]
    pairs, plinks, hist, hits, st = P.check(k, mu, walks, wo, steps, rows, P.READ_PARAMS)
    across = [r for s, r in zip(starts, pairs) if 750 <= s <= 850]
    G = P.island_gap()
    assert G == 121 and len(across) == 101 == st["n_link"] and st["n_adjacent"] == 0 == st["n_far"]
    assert all(r["cls"] == P.LINK and r["edge"] == P.NO_EDGE and 221 - r["d"] == G for r in across)
    assert len(plinks) == 1 and plinks[0][2] == 101 and plinks[0][3] == 101 * (221 - G) and plinks[0][4] == plinks[0][5] == 221 - G
    assert all(r["cls"] == P.SAME and r["frag"] == 400 for s, r in zip(starts, pairs) if not 750 <= s <= 850) and st["n_same"] == len(starts) - 101
    far = P.pair_walks(k, mu, walks, wo, steps, rows, 1, 221 - G - 1, 10, 64)
    assert far[4]["n_far"] == 101 and not far[1]
