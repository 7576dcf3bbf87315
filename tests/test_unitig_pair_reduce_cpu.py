"""The rule of kmx_unitig_pair_reduce without a GPU: the restatement (tests/unitig_pair_reduce_ref.py) against the consequences
the header states, on line lists that do hold transitive entries, at the edges of the tolerance and on a skip of three steps;
the acceptance case through the scaffold restatement; the Python layouts against the header; what the entry points refuse without
a handle; the facade's writer."""
import ctypes as C
import os
import subprocess

import pytest

import unitig_pair_reduce_ref as X
import unitig_pairs_ref as P
import unitig_scaffold_ref as S
from kmcex_amd import api
from kmcex_amd.api import PAIR_REDUCE_DTYPE, PairReduceParams, PairReduceStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", (3, 40, 300))
@pytest.mark.parametrize("tol", (0, 1, 40))
def test_consequences_on_line_lists(n, tol):
    mu, pl = X.line_list(n, X.LINE_SEEDS[n], 1)
    assert len(pl) == n and all(a[:2] < b[:2] for a, b in zip(pl, pl[1:])) and all(P.canonical(e[0], e[1]) == e[:2] for e in pl)
    res = X.check(mu, pl, dict(X.PAR, tol=tol))
    st = res["stats"]
    assert st["n_transitive"] * 10 >= n and st["n_kept"] * 10 >= n, "the list must hold both verdicts"
    assert st["n_ignored"] == st["n_below_min"] == st["n_complex"] == 0 and st["n_rows"] == 2 * n


def test_consequences_on_hubs_and_mixed_lists():
    for deg in (7, 8, 9, 65):
        mu, pl, i = X.hub_list(deg)
        for mr in (deg - 1, deg, deg + 1):
            r = X.check(mu, pl, dict(min_pairs=2, inner=2000, tol=1, max_row=mr))["rrecs"][i]
            assert r["verdict"] == (X.COMPLEX if mr < deg else X.TRANSITIVE) and r["side"] == 0
    mu, pl = X.line_list(40, 1, 1)
    res = X.check(mu, pl, dict(X.PAR, tol=1, min_pairs=5))
    assert res["stats"]["n_below_min"] > 0 and res["stats"]["n_transitive"] > 0
    full = X.reduce(mu, pl, **dict(X.PAR, tol=1))
    assert res["stats"]["n_transitive"] < full["stats"]["n_transitive"]          # an entry below min_pairs is no witness


def test_sides_and_duplicate_rows():
    mu, pl, i = X.hub_list(6, 20, 0)
    a = X.check(mu, pl, dict(min_pairs=2, inner=2000, tol=2, max_row=64))["rrecs"][i]
    mu, pl, i = X.hub_list(6, 0, 20)
    c = X.check(mu, pl, dict(min_pairs=2, inner=2000, tol=2, max_row=64))["rrecs"][i]
    assert (a["side"], c["side"]) == (1, 0) and a["n_via"] == c["n_via"] == 5 and a["via"] == c["via"]
    # duplicate keys: every row counts, first(x, y) is the smallest entry, and the delta reported is the first row's on side 0
    mu = [30, 40, 17]
    inner, G = 2000, 500
    pl = [X.entry(0, 2, G, inner), X.entry(0, 4, 7, inner), X.entry(0, 4, 8, inner), X.entry(4, 2, G - 7 - 17, inner, canonical=False), X.entry(4, 2, G - 8 - 17, inner, canonical=False)]
    r = X.reduce(mu, pl, 2, inner, 1, 64)["rrecs"][0]
    assert (r["verdict"], r["via"], r["n_via"], r["side"], r["delta"]) == (X.TRANSITIVE, 4, 2, 0, 0)      # rows (0, 4, 1) and (0, 4, 2) over first(4, 2) = entry 3: deltas 0 and -1
    pl = pl[:1] + pl[3:] + pl[1:3]                                  # the same with a -> b listed last: out(c ^ 1) is as long, side 0 stays
    r = X.reduce(mu, pl, 2, inner, 1, 64)["rrecs"][0]
    assert (r["n_via"], r["delta"]) == (2, 0)


@pytest.mark.parametrize("tol", (0, 5, 21))
def test_delta_at_the_tolerance(tol):
    for err, verdict in ((tol, X.TRANSITIVE), (-tol, X.TRANSITIVE), (tol + 1, X.KEPT), (-(tol + 1), X.KEPT)):
        mu, pl, i = X.hub_list(2, errs=(err,))
        r = X.check(mu, pl, dict(min_pairs=2, inner=2000, tol=tol, max_row=64))["rrecs"][i]
        assert r["verdict"] == verdict and (verdict == X.KEPT or (r["delta"], r["n_via"], r["via"]) == (-err, 1, 4)), (err, tol)


def test_a_skip_of_three_steps_stays():
    """a -> d with only a -> b -> c -> d: no single unitig explains it"""
    mu = [50, 60, 70, 80]
    inner, g = 1000, 30
    chain = [X.entry(0, 2, g, inner), X.entry(2, 4, g, inner), X.entry(4, 6, g, inner)]
    far = X.entry(0, 6, 3 * g + mu[1] + mu[2], inner)
    res = X.check(mu, sorted(chain + [far]), dict(min_pairs=2, inner=inner, tol=0, max_row=64))
    assert res["stats"]["n_kept"] == 4 and res["stats"]["n_transitive"] == 0
    mid = X.entry(0, 4, 2 * g + mu[1], inner)                     # with the intermediate skip both go
    res = X.check(mu, sorted(chain + [far, mid]), dict(min_pairs=2, inner=inner, tol=0, max_row=64))
    assert res["stats"]["n_transitive"] == 2 and sorted(e[:2] for e in res["lout"]) == sorted(e[:2] for e in chain)


def test_the_g_arithmetic():
    e = lambda n, sm: (0, 2, n, sm, 0, 0)
    assert X.g_of(e(61, 61 * 60), 221) == 160 and X.g_of(e(7, 7 * 226 + 6), 300) == 73          # the division floors
    assert X.g_of(e(1, 40), 30) == -11 and X.g_of(e(1, 2 ** 64 - 1), 0) == 0 and X.g_of(e(1, 2 ** 63), 0) == 2 ** 63 - 1


@pytest.mark.parametrize("seed,holes", X.ISLAND_CASES)
def test_three_islands_become_one_scaffold(seed, holes):
    """consequence (e): without the reduction three scaffolds, with it the genome with both holes as N of their true length"""
    k, strs, pl, genome = X.three_islands(seed, holes)
    assert sorted(map(len, strs)) == sorted([holes[0][0], holes[1][0] - holes[0][1], X.ISLAND_GENOME - holes[1][1]]) and len(pl) == 3
    mu = [len(s) - k + 1 for s in strs]
    assert len(S.scaffold(k, strs, None, pl, **X.SCAFFOLD_PAR)["sstrs"]) == 3
    for tol in (0, k):
        res = X.check(mu, pl, dict(X.ISLAND_PAR, tol=tol))
        skip = [r for r in res["rrecs"] if r["verdict"] == X.TRANSITIVE]
        assert len(skip) == 1 and skip[0]["delta"] == 0 and skip[0]["n_via"] == 1 and res["stats"]["n_kept"] == 2
        sc = S.scaffold(k, strs, None, res["lout"], **X.SCAFFOLD_PAR)
        S.check(k, strs, res["lout"], sc, X.SCAFFOLD_PAR["max_n"])
        assert len(sc["sstrs"]) == 1
        s = sc["sstrs"][0] if sc["sstrs"][0][:50] == genome[:50] else S.oriented(sc["sstrs"][0], 1)
        n_holes = sum(hi - lo for lo, hi in holes)
        assert len(s) == X.ISLAND_GENOME and s.count("N") == n_holes and n_holes == (20 if holes[0][1] == 910 else 56)
        assert all(c == g for c, g in zip(s, genome) if c != "N") and all(s[lo:hi] == "N" * (hi - lo) for lo, hi in holes)


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(PairReduceParams) == 24 and C.sizeof(PairReduceStats) == 80 and [f for f, _ in PairReduceStats._fields_] == list(X.STAT_FIELDS)
    assert PAIR_REDUCE_DTYPE == X.PAIR_REDUCE_DTYPE and PAIR_REDUCE_DTYPE.itemsize == 32 and api.PAIR_REDUCE_NO_VIA == X.NO_VIA
    assert [api.PAIR_REDUCE_VERDICTS[i] for i in range(5)] == list(X.VERDICTS)
    fields = [("kmx_pair_reduce", f) for f in PAIR_REDUCE_DTYPE.names] + [("kmx_pair_reduce_params", f) for f, _ in PairReduceParams._fields_] + [("kmx_pair_reduce_stats", f) for f in X.STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %d %d %d %d %d", sizeof(kmx_pair_reduce_params), sizeof(kmx_pair_reduce), '
                   'sizeof(kmx_pair_reduce_stats), KMX_REDUCE_IGNORED, KMX_REDUCE_BELOW_MIN, KMX_REDUCE_KEPT, KMX_REDUCE_TRANSITIVE, KMX_REDUCE_COMPLEX);'
                   + "".join(f' printf(" %zu", offsetof({s}, {f}));' for s, f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:8] == [24, 32, 80, 0, 1, 2, 3, 4]
    want = [PAIR_REDUCE_DTYPE.fields[f][1] for f in PAIR_REDUCE_DTYPE.names] + [getattr(PairReduceParams, f).offset for f, _ in PairReduceParams._fields_] + [getattr(PairReduceStats, f).offset for f in X.STAT_FIELDS]
    assert got[8:] == want == [0, 4, 8, 12, 16, 24, 0, 8, 12, 16, 20] + list(range(0, 80, 8))


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    n, par, st = C.c_uint64(0), PairReduceParams(2, 300, 0, 64, 0), PairReduceStats()
    assert L.kmx_unitig_pair_reduce(None, 21, None, 0, None, 0, C.byref(par), None, None, None, 0, C.byref(n), C.byref(st)) == -1
    assert L.kmx_unitig_pair_reduce_dev(None, 21, None, 0, 0, None, 0, C.byref(par), None, None, None, 0, C.byref(n), C.byref(st)) == -1
    assert L.kmx_unitig_pair_reduce_last_phases(None, None) == -1


def test_facade_writer(tmp_path):
    """tests/facade_unitig_pair_reduce.cpp compiles against include/kmodel.hpp with the reference's flags; its writer, which needs
    no device, gives the restatement's text for a hand-made result (also under the host sanitizers)"""
    plinks = [(0, 4, 61, 3660, 60, 60), (0, 6, 21, 3990, 190, 190), (3, 9, 7, 70, 10, 10), (5, 5, 0, 0, 0, 0), (8, 2, 1, 5, 5, 5)]
    rec = lambda v, via, n, side, g, d: {"verdict": v, "via": via, "n_via": n, "side": side, "g": g, "delta": d}
    res = {"rrecs": [rec(X.TRANSITIVE, 7, 2, 1, 160, -3), rec(X.KEPT, X.NO_VIA, 0, 0, 30, 0), rec(X.COMPLEX, X.NO_VIA, 0, 1, -12, 0), rec(X.IGNORED, X.NO_VIA, 0, 0, 0, 0), rec(X.BELOW_MIN, X.NO_VIA, 0, 0, 0, 0)]}
    text = X.reduce_tsv(plinks, res)
    assert text.splitlines()[0] == "0\tu0+\tu2+\t61\tTRANSITIVE\t<u3\t2\t160\t-3" and text.splitlines()[2] == "2\tu1-\tu4-\t7\tCOMPLEX\t*\t0\t-12\t0" and text.splitlines()[3].endswith("IGNORED\t*\t0\t0\t0")
    for name, extra in (("plain", ()), ("san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_pair_reduce.cpp"),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--text-only"]).decode() == text, name
