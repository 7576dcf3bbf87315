"""CPU: the plain-Python restatement of kmx_unitig_pair_paths (tests/unitig_pair_paths_ref.py) on the acceptance case (a 150-base
repeat twice in 1800 bases, which no read crosses and every fragment does) gives the figures the rule was designed on, and
satisfies the consequences include/kmx.h states on the crafted graphs the GPU tests compare the library with; the structs of kmx.h
are laid out as the ctypes and NumPy mirrors say; the entry points refuse a null handle; the facade's writer gives the
restatement's text."""
import ctypes as C
import os
import subprocess

import pytest

import unitig_contigs_ref as G
import unitig_map_ref as R
import unitig_pair_paths_ref as Q
import unitig_pairs_ref as P
import unitig_resolve_ref as RS
import unitig_walk_ref as W
import unitigs_ref as U
from kmcex_amd import api
from kmcex_amd.api import PAIR_PATH_DTYPE, PairPathParams, PairPathStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_acceptance_case():
    k, genome, km, cnt, strs, reads, rows = Q.acceptance()
    assert len(genome) == 1800 and len(strs) == 4 and len(reads) == 2 * 1401
    mu = [len(s) - k + 1 for s in strs]
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    walks, wo, steps, hits, _ = W.walk_segs(k, strs, segs, so, rows, k, 0)
    t, _ = RS.through(walks, steps, rows, len(strs))
    rep = [u for u in range(4) if len(strs[u]) == 150]
    assert len(rep) == 1 and mu[rep[0]] == 130 and sum(t) == 0                    # no read crosses the repeat
    before = RS.resolve(k, strs, None, rows, hits, t, 2, 0)
    assert before["stats"]["n_unsupported"] == 1 and before["stats"]["n_resolved"] == 0
    assert len(G.contigs(k, before["rstrs"], None, before["rrows"], before["rlink_hits"], 1, 0)["cstrs"]) == 4
    pairs, plinks, hist, pair_hits, pst = P.pair_walks(k, mu, walks, wo, steps, rows, *P.READ_PARAMS)
    assert len(plinks) == 6 and {p["d"] for p in pairs if p["cls"] == P.SAME} == {221}
    for tol in (0, k):
        par = dict(Q.ACCEPT_PAR, tol=tol)
        res = Q.pair_paths(mu, rows, plinks, **par)
        Q.check(mu, rows, plinks, res, par)
        path = [(e, r) for e, r in zip(plinks, res["recs"]) if r[0] == Q.PATH]
        assert len(path) == 2 and all(e[2:4] == (91, 91 * 90) and r[1] == 1 and r[3] == 130 for e, r in path)
        assert [r[0] for r in res["recs"]].count(Q.ADJACENT) == 4 and {s >> 1 for s in res["psteps"]} == {rep[0]}
        assert sorted(x for x in res["through"] if x) == [91, 91] and res["stats"]["n_added"] == 2 and res["stats"]["n_missing"] == 0
    both_t = [x + y for x, y in zip(t, res["through"])]
    both_h = [x + y + z for x, y, z in zip(hits, pair_hits, res["path_hits"])]
    after = RS.resolve(k, strs, None, rows, both_h, both_t, 2, 0)
    assert after["stats"]["n_resolved"] == 1 and after["stats"]["n_unsupported"] == 0 and len(after["rstrs"]) == 5
    cstrs = G.contigs(k, after["rstrs"], None, after["rrows"], after["rlink_hits"], 1, 0)["cstrs"]
    assert len(cstrs) == 1 and len(cstrs[0]) == 1800 and cstrs[0] in (genome, U.rc(genome))


def test_consequences_on_the_crafted_graphs():
    g, named = Q.crafted()
    for name, (e, q, verdict) in named.items():
        par = dict(Q.PAR, **q)
        lst = e if name == "hub" else [e]
        res = Q.pair_paths(g.mu, g.rows, lst, **par)
        Q.check(g.mu, g.rows, lst, res, par)
        assert {r[0] for r in res["recs"]} == {verdict}, name
    res = Q.pair_paths(g.mu, g.rows, [named["loop_twice"][0]], **Q.PAR)
    assert res["psteps"][0] == res["psteps"][1] and len(res["psteps"]) == 2 and len({i for i, x in enumerate(res["through"]) if x}) == 2
    res = Q.pair_paths(g.mu, g.rows, [named["chain16"][0]], **dict(Q.PAR, max_steps=16))
    assert res["recs"][0][1] == 16 and res["stats"]["n_added"] == 16
    hub = Q.pair_paths(g.mu, g.rows, Q.hub_list(), **Q.PAR)
    assert hub["stats"]["n_path"] == 300 and max(hub["through"]) == sum(e[2] for e in Q.hub_list())    # every entry adds to one cell


@pytest.mark.parametrize("n", (1, 255, 256, 257, 513))
def test_consequences_on_mixed_lists(n):
    g, named = Q.crafted()
    lst = Q.crafted_list(n, n, Q.PAR)
    assert all((a[0], a[1]) < (b[0], b[1]) for a, b in zip(lst, lst[1:]))
    res = Q.pair_paths(g.mu, g.rows, lst, **Q.PAR)
    Q.check(g.mu, g.rows, lst, res, Q.PAR)
    if n >= 255:
        st = res["stats"]
        assert min(st[f] for f in ("n_ignored", "n_below_min", "n_no_path", "n_adjacent", "n_path", "n_ambiguous")) >= 1
    into = Q.pair_paths(g.mu, g.rows, lst, through=[7] * (16 * len(g.mu)), path_hits=[3] * len(res["path_hits"]), **Q.PAR)
    assert into["through"] == [x + 7 for x in res["through"]] and into["path_hits"] == [x + 3 for x in res["path_hits"]]


def test_the_window_arithmetic():
    e = lambda n, sm: (0, 2, n, sm, 0, 0)
    assert Q.bounds(e(91, 8190), 221, 21) == (130, 109, 151)
    assert Q.bounds(e(7, 7 * 226 + 6), 300, 0) == (73, 73, 73)                   # the division floors
    assert Q.bounds(e(1, 40), 30, 5) == (-11, -16, -6)                           # hi < 0
    assert Q.bounds(e(1, 2 ** 64 - 1), 0, 1) == (0, -1, 1)                       # D wraps to -1 as a signed value
    assert Q.search([5, 5], [[2], [], [], [1]], e(1, 40), 30, 5, 8, 4096) == (0, [])


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(PairPathParams) == 32 and C.sizeof(PairPathStats) == 80 and [f for f, _ in PairPathStats._fields_] == list(Q.STAT_FIELDS)
    assert PAIR_PATH_DTYPE == Q.PAIR_PATH_DTYPE and PAIR_PATH_DTYPE.itemsize == 32 and api.PAIR_PATH_MAX_STEPS == Q.MAX_STEPS
    assert [api.PAIR_PATH_VERDICTS[i] for i in range(7)] == list(Q.VERDICTS)
    fields = [("kmx_pair_path", f) for f in PAIR_PATH_DTYPE.names] + [("kmx_pair_path_params", f) for f, _ in PairPathParams._fields_] + [("kmx_pair_path_stats", f) for f in Q.STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %d %d %d %d %d %d %d %d %d", sizeof(kmx_pair_path_params), sizeof(kmx_pair_path), '
                   'sizeof(kmx_pair_path_stats), KMX_PATH_MAX_STEPS, KMX_ABI_VERSION, KMX_PATH_IGNORED, KMX_PATH_BELOW_MIN, KMX_PATH_NO_PATH, KMX_PATH_ADJACENT, KMX_PATH_PATH, KMX_PATH_AMBIGUOUS, '
                   'KMX_PATH_COMPLEX);\n' + "".join(f' printf(" %zu", offsetof({s}, {f}));\n' for s, f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:12] == [32, 32, 80, 16, 5, 0, 1, 2, 3, 4, 5, 6]
    want = [PAIR_PATH_DTYPE.fields[f][1] for f in PAIR_PATH_DTYPE.names] + [getattr(PairPathParams, f).offset for f, _ in PairPathParams._fields_] + [getattr(PairPathStats, f).offset for f in Q.STAT_FIELDS]
    assert got[12:] == want == [0, 4, 8, 16, 24, 28, 0, 8, 12, 16, 20, 24] + list(range(0, 80, 8))


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    n, par, st = C.c_uint64(0), PairPathParams(2, 300, 0, 8, 4096, 0), PairPathStats()
    assert L.kmx_unitig_pair_paths(None, 21, None, 0, None, None, 0, None, 0, C.byref(par), None, None, 0, C.byref(n), None, None, C.byref(st)) == -1
    assert L.kmx_unitig_pair_paths_dev(None, 21, None, 0, None, None, 0, None, 0, C.byref(par), None, None, 0, C.byref(n), None, None, C.byref(st)) == -1
    assert L.kmx_unitig_pair_paths_last_phases(None, None) == -1


def test_facade_writer(tmp_path):
    """tests/facade_unitig_pair_paths.cpp compiles against include/kmodel.hpp with the reference's flags; its writer, which needs no
    device, gives the restatement's text for a hand-made result (also under the host sanitizers)"""
    plinks = [(0, 4, 91, 8190, 90, 90), (0, 6, 130, 28600, 220, 220), (3, 9, 7, 70, 10, 10), (5, 5, 0, 0, 0, 0), (8, 2, 1, 5, 5, 5)]
    res = {"recs": [(Q.PATH, 1, 0, 130, 1, 2), (Q.ADJACENT, 0, 1, 0, 1, 1), (Q.PATH, 3, 1, 73, 1, 4), (Q.IGNORED, 0, 0, 0, 0, 0), (Q.BELOW_MIN, 0, 0, 0, 0, 0)], "psteps": [6, 11, 12, 15]}
    text = Q.paths_tsv(plinks, res)
    assert text.splitlines()[0] == "0\tu0+\tu2+\t91\tPATH\t130\t>u3" and text.splitlines()[2] == "2\tu1-\tu4-\t7\tPATH\t73\t<u5>u6<u7" and text.splitlines()[3].endswith("IGNORED\t0\t*")
    for name, extra in (("plain", ()), ("san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_pair_paths.cpp"),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--text-only"]).decode() == text, name
