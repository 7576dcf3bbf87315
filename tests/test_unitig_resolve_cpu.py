"""CPU: the plain-Python restatement of kmx_unitig_walk_through and kmx_unitig_resolve (tests/unitig_resolve_ref.py) equals its golden
digests and satisfies the consequences include/kmx.h states, on every case the GPU tests compare the library with: planted repeats
that become one contig, the listed cases of the contigs with their real walks, synthetic through matrices on real graphs, and the
emit geometry; the record layouts against the header; the refusal of a null handle."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import unitig_contigs_ref as G
import unitig_resolve_ref as X
import unitigs_ref as U
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitig_resolve_golden.json")) as f:
        return json.load(f)


def golden(k, strs, recs, rows, hits, t, g):
    assert g["through"] == [sum(1 for x in t if x), sum(t), X.digest([np.array(t, dtype=np.uint64)])]
    for p in X.PARAMS:
        res = X.resolve(k, strs, recs, rows, hits, list(t), *p)
        assert g[f"{p[0]},{p[1]}"] == [res["stats"][f] for f in X.RESOLVE_STAT_FIELDS] + [X.digest(X.flat(res))]


# what the planted cases must give at (2, 0): unitigs before and after, contigs before and after at (1, 0), the longest contig
PLANTED_FIGURES = {"k21_2x40": (530, 4, 5, 4, 1, 529), "k21_3x40": (720, 5, 7, 5, 1, 718), "k31_4x45": (930, 6, 9, 6, 1, 928), "k63_3x70": (810, 5, 7, 5, 1, 808)}


@pytest.mark.parametrize("name", sorted(X.PLANTED))
def test_planted_repeats(name, fixture):
    """a repeat shorter than a read ends every contig at both of its sides; resolved from the through hits of the same reads, the
    genome is one contig, a substring of it that lacks a base (the forced flank boundaries make the first or last window unique to a
    tip of one k-mer)"""
    k, genome, km, cnt, strs, recs, reads, rows, hits, t = X.planted_case(name)
    golden(k, strs, recs, rows, hits, t, fixture["planted"][name])
    before = G.contigs(k, strs, recs, rows, hits, 1, 0)
    res = X.resolve(k, strs, recs, rows, hits, t, 2, 0)
    X.check_resolved(k, strs, rows, res)
    after = G.contigs(k, res["rstrs"], res["rrecs"], res["rrows"], res["rlink_hits"], 1, 0)
    G.check(k, res["rstrs"], res["rrecs"], res["rrows"], after, node_graph=False)
    longest = max(after["cstrs"], key=len)
    assert longest in genome or U.rc(longest) in genome
    if name in PLANTED_FIGURES:
        assert (len(genome), len(strs), len(res["rstrs"]), len(before["cstrs"]), len(after["cstrs"]), len(longest)) == PLANTED_FIGURES[name]
        assert res["stats"]["n_resolved"] == 1 == res["stats"]["n_candidates"]
    elif name == "k21_2x120":                                    # a repeat no read spans: nothing resolved, the output is the input
        assert res["stats"]["n_unsupported"] == 1 == res["stats"]["n_candidates"] and res["rstrs"] == strs and len(after["cstrs"]) == len(before["cstrs"]) == 4
        assert after["cstrs"] == before["cstrs"]
    else:                                                        # k = 5: one repeat resolved among hairpins and self-loops
        assert name == "k5_2x9" and (len(strs), len(res["rstrs"])) == (70, 71)
        assert (res["stats"]["n_candidates"], res["stats"]["n_resolved"], res["stats"]["n_crossed"], res["stats"]["n_ambiguous"]) == (28, 1, 2, 25)
        assert any(x >> 1 == o >> 1 for o, row in enumerate(rows) for x in row), "the case holds hairpins or self-loops"


# the non-zero cells and the sum of through at (0, 0)
LISTED_FIGURES = {"k33_tangle": (58, 139), "k31_tangle": (58, 125), "k5_complete": (338, 344), "k21_noisy": (435, 952)}


@pytest.mark.parametrize("name", G.LISTED_CASES)
def test_listed_cases_with_their_real_walks(name, fixture):
    """consequences (a), (b), (c) of the through hits on the walks at (0, 0) and (k, 1), and the resolution on them: an exact no-op
    wherever nothing is resolved, and k21_noisy, where reads pair the two sides of two small bubbles' neighbours at (1, 0)"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    for which in X.WALK_PARAMS:
        t, st = X.listed_through(name, which)
        hits = list(G.hits_of(name, which))
        golden(k, strs, recs, rows, hits, t, fixture["listed"][name][which])
        X.check_through(rows, len(strs), list(t), st, hits)
        wm = X.listed_walks(name, which, True)
        tm, stm = X.through(wm[0], wm[2], rows, len(strs))
        assert tuple(tm) == t and stm["n_added"] == st["n_added"], "consequence (b): the reverse complements of all reads add to the same cells"
        if which == "exact" and name in LISTED_FIGURES:
            assert (sum(1 for x in t if x), sum(t)) == LISTED_FIGURES[name]
        for p in X.PARAMS:
            res = X.resolve(k, strs, recs, rows, hits, list(t), *p)
            X.check_resolved(k, strs, rows, res)
            assert res["stats"]["n_resolved"] == (2 if name == "k21_noisy" and p == (1, 0) else 0)
            if not res["stats"]["n_resolved"]:                   # consequence (a): byte for byte the input
                flat = X.flat(res)
                ubuf, uoff = X.R.join(strs)
                loff, lk = X.L.flat_links(rows)
                assert flat[0].tobytes() == ubuf.tobytes() and flat[1].tobytes() == uoff.tobytes() and flat[5].tobytes() == loff.tobytes() and flat[6].tobytes() == lk.tobytes()
                assert flat[2].tobytes() == U.flat(strs, recs)[2].tobytes() and flat[8].tolist() == hits
        zero = X.resolve(k, strs, recs, rows, hits, [0] * (16 * len(strs)), 1, 0)
        assert zero["stats"]["n_resolved"] == 0 and zero["rrows"] == [list(r) for r in rows] and zero["stats"]["n_unsupported"] == zero["stats"]["n_candidates"]


SYNTH_FIGURES = {"k5_complete": (448, (120, 120, 222)), "k31_tangle": (12, (1, 1, 5)), "k33_tangle": (15, (2, 2, 6)), "k21_every_kind": (4, (0, 0, 1))}


@pytest.mark.parametrize("name", X.SYNTH_CASES)
def test_synthetic_through_on_real_graphs(name, fixture):
    """every output is mirrored, has rows <= 4, no edge twice and the edge count of the input, and the contigs of the result pass the
    contigs' own check; k5_complete holds hundreds of edges between two resolved unitigs"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    t = list(X.synthetic_case(name))
    golden(k, strs, recs, rows, None, t, fixture["synthetic"][name])
    for i, p in enumerate(X.PARAMS):
        res = X.resolve(k, strs, recs, rows, None, t, *p)
        X.check_resolved(k, strs, rows, res)
        assert (res["stats"]["n_candidates"], res["stats"]["n_resolved"]) == (SYNTH_FIGURES[name][0], SYNTH_FIGURES[name][1][i])
        ct = G.contigs(k, res["rstrs"], res["rrecs"], res["rrows"], [1] * len(res["link_origin"]), 1, 0)
        G.check(k, res["rstrs"], res["rrecs"], res["rrows"], ct, node_graph=False)
        copies = [res["rplace"][u][1] for u in res["origin"]]
        between = sum(1 for a, row in enumerate(res["rrows"]) for b in row if copies[a >> 1] > 1 and copies[b >> 1] > 1)
        if name == "k5_complete":
            assert between == (224, 224, 798)[i]
        assert all(r["n_pred"] == r["n_succ"] == 1 for r, c in zip(res["rrecs"], copies) if c > 1)


def test_emit_geometry_by_hand():
    for length in X.GEOMETRY_LENGTHS:
        for shift in (0, 7, 15):
            k, strs, rows, t = X.geometry_case(length, shift)
            res = X.resolve(k, strs, None, rows, None, t, 2, 0)
            X.check_resolved(k, strs, rows, res, overlaps_hold=False)
            assert res["stats"]["n_resolved"] == 1 and res["rplace"][1] == (1, 4) and res["rstrs"][1:5] == [strs[1]] * 4 and len(res["rstrs"]) == 13
            assert [res["rrows"][2 * (1 + c)] for c in range(4)] == [[2 * (3 + 6 + b)] for b in (2, 0, 3, 1)]      # copy c leaves by way out pi(c)
            assert res["rrows"][2 * 5] == [2 * 1] and res["rrows"][2 * 9 + 1] == [2 * 2 + 1]                      # way in 0 enters copy 0 (new unitig 1); way out 0 is left by copy 1 (new unitig 2)


def test_verdicts_by_hand():
    rows = [[4, 6], [8, 10], [], [], [], [1], [], [1], [], [0], [], [0]]      # unitig 0: ways out 4 and 6, ways in from 9 and 11 (their mirrors 8 and 10)
    t = [0] * (16 * 6)
    v = lambda: X.verdict(rows, 0, t, 2, 1)
    assert v() == ("unsupported", None)
    t[0 + 1], t[4 + 0] = 2, 5
    assert v() == ("resolved", [1, 0])
    t[0] = 1
    assert v() == ("resolved", [1, 0]) and X.verdict(rows, 0, t, 2, 0)[0] == "crossed" and X.verdict(rows, 0, t, 1, 0)[0] == "ambiguous"
    t[0] = 2
    assert v()[0] == "ambiguous"
    t[0], t[4] = 0, 0
    assert v()[0] == "ambiguous"                                 # a row without a supported cell
    t[3] = 1 << 60                                               # a cell outside p x p is ignored
    t[4] = 2
    assert v() == ("resolved", [1, 0])
    assert X.verdict(rows, 0, t, 0, 0) == ("resolved", [1, 0])   # min_reads = 0 still asks for one read
    assert X.verdict([[0, 6], [8, 10]] + rows[2:], 0, t, 2, 1) == (None, None) and X.verdict([[4], [8, 10]] + rows[2:], 0, t, 2, 1) == (None, None)
    assert X.verdict(rows, 1, t, 2, 1) == (None, None)


def test_record_layouts_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(kmx_resolve_params), '
                   'sizeof(kmx_resolve_place), sizeof(kmx_through_stats), sizeof(kmx_resolve_stats), offsetof(kmx_through_stats, n_missing), offsetof(kmx_resolve_stats, n_unitigs_out), '
                   'offsetof(kmx_resolve_place, n_copies), KMX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [16, 8, 64, 64, 32, 48, 4, 5]
    assert C.sizeof(api.ResolveParams) == 16 and C.sizeof(api.ThroughStats) == 64 == C.sizeof(api.ResolveStats) and api.RESOLVE_PLACE_DTYPE.itemsize == 8
    assert api.RESOLVE_PLACE_DTYPE == X.RESOLVE_PLACE_DTYPE and [f for f, _ in api.ResolveStats._fields_] == list(X.RESOLVE_STAT_FIELDS)
    assert [f for f, _ in api.ThroughStats._fields_][:5] == list(X.THROUGH_STAT_FIELDS)
    for sym in ("kmx_unitig_walk_through", "kmx_unitig_walk_through_dev", "kmx_unitig_resolve", "kmx_unitig_resolve_dev", "kmx_unitig_resolve_last_phases"):
        assert sym in api.ABI_SYMBOLS
    assert all(callable(getattr(api.KModel, f)) for f in ("unitig_through_flat", "unitig_through_dev", "unitig_resolve_flat", "unitig_resolve_dev", "resolved_contigs_from_walks"))


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    st, rs, par = api.ThroughStats(), api.ResolveStats(), api.ResolveParams(2, 0)
    n, b = C.c_uint64(7), C.c_uint64(7)
    z = np.zeros(1, dtype=np.uint64)
    assert L.kmx_unitig_walk_through(None, None, 0, None, 0, z.ctypes.data, None, 0, 0, None, C.byref(st)) == -1
    assert L.kmx_unitig_walk_through_dev(None, None, 0, None, 0, z.ctypes.data, None, 0, 0, None, C.byref(st)) == -1
    assert L.kmx_unitig_resolve(None, 21, None, z.ctypes.data, 0, None, z.ctypes.data, None, 0, None, None, C.byref(par), None, 0, None, 0, None, None, None, None, None, None, None,
                                C.byref(n), C.byref(b), C.byref(rs)) == -1
    assert L.kmx_unitig_resolve_dev(None, 21, None, z.ctypes.data, 0, 0, None, z.ctypes.data, None, 0, None, None, C.byref(par), None, 0, None, 0, None, None, None, None, None, None, None,
                                    C.byref(n), C.byref(b), C.byref(rs)) == -1
    assert L.kmx_unitig_resolve_last_phases(None, None) == -1
    assert b"null" in L.kmx_last_error()
