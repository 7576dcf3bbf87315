"""CPU: the plain-Python restatement of kmx_unitig_scaffold (tests/unitig_scaffold_ref.py) satisfies the consequences include/kmx.h
states, on the cases the GPU tests compare the library with; the structs of kmx.h are laid out as the ctypes and NumPy mirrors say;
the facade's three writers give the restatement's text; and the two islands of the pair tests come out as one scaffold with the
hole as 100 N."""
import ctypes as C
import os
import subprocess

import pytest

import unitig_pairs_ref as P
import unitig_scaffold_ref as S
import unitigs_ref as U
from kmcex_amd import api
from kmcex_amd.api import SCAFFOLD_DTYPE, SCAFFOLD_PLACE_DTYPE, SCAFFOLD_STEP_DTYPE, ScaffoldParams, ScaffoldStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAR = dict(min_pairs=2, ratio=0, inner=300, min_n=3, max_n=200)


def run(k, strs, plinks, recs=None, **par):
    q = dict(PAR, **par)
    res = S.scaffold(k, strs, recs, plinks, q["min_pairs"], q["ratio"], q["inner"], q["min_n"], q["max_n"])
    S.check(k, strs, plinks, res, q["max_n"])                     # consequence (c)
    return res


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 513))
def test_consequences_on_random_lists(n):
    k, km, strs, mu = P.craft_set()
    plinks = S.random_list(n, 40 + n)
    res = run(k, strs, plinks)
    st = res["stats"]
    assert st["n_entries"] == st["n_links"] == n and st["n_below_min"] + st["n_kept"] == n and st["n_scaffolds"] + st["n_chain"] - st["n_circular"] == len(strs)
    # (a) nothing kept: the input byte for byte
    for none in (run(k, strs, []), run(k, strs, plinks, min_pairs=41)):
        assert none["sstrs"] == strs and none["stats"]["n_multi"] == 0 and all(p == (2 * u, 0, 0) for u, p in enumerate(none["place"]))
        assert [s[0] for s in none["steps"]] == [2 * u for u in range(len(strs))]
    # (b) any entry mirrored: nothing but which entry is counted (the list is no longer sorted: the rule does not ask for it)
    mir = [S.mirrored(e) if i % 3 == 0 else e for i, e in enumerate(plinks)]
    assert run(k, strs, mir) == res
    # with a ratio fewer are kept, never more
    rat = run(k, strs, plinks, ratio=3)["stats"]
    assert rat["n_kept"] + rat["n_below_ratio"] == st["n_kept"] and rat["n_below_min"] == st["n_below_min"]


@pytest.mark.parametrize("n", range(2, 10))
@pytest.mark.parametrize("closed", (False, True))
def test_chains_and_cycles_of_every_length(n, closed):
    k, km, strs, mu = P.craft_set()
    order = [17, 3, 44, 9, 60, 2, 71, 30, 5][:n]
    flips = [1, 0, 0, 1, 1, 0, 1, 0, 0][:n]
    res = run(k, strs, S.chain_list(order, flips, closed))
    multi = [r for r in res["srecs"] if r["n_steps"] > 1]
    assert len(multi) == 1 and multi[0]["n_steps"] == n and multi[0]["circular"] == int(closed) and res["stats"]["n_chain"] == n - (0 if closed else 1)
    first = res["steps"][multi[0]["first_step"]]
    if closed:
        assert first[0] == 2 * min(order) and first[1] > 0        # orientation 0 at the smallest unitig, with the closing link's N, which are not spelled
        assert multi[0]["n_gap_bases"] == sum(s[1] for s in res["steps"][multi[0]["first_step"] + 1:multi[0]["first_step"] + n])
    else:
        assert first[0] >> 1 == min(order[0], order[-1]) and first[1:] == (0, 0)


def test_the_gap_arithmetic():
    k = 21
    e = lambda n, sm: (0, 2, n, sm, 0, 0)
    assert S.gap_of(k, e(101, 10100), 221, 0, 1000) == (100, 100)
    assert S.gap_of(k, e(3, 302), 100, 5, 50) == (100 - 1 - 100 - 20, 5)              # negative: the unitigs would overlap
    assert S.gap_of(k, e(1, 0), 2 ** 32 - 1, 0, 77) == (2 ** 32 - 2 - 20, 77)          # above max_n
    assert S.gap_of(k, e(1, 40), 30, 0, 0) == (-31, 0)                               # inner < D + 1, min_n = max_n = 0
    assert S.gap_of(k, e(1, 2 ** 64 - 1), 0, 1, 9) == (-20, 1)                         # D wraps to -1 as a signed value
    assert S.gap_of(k, e(2 ** 63, 2 ** 63), 221, 0, 1000)[0] == 221 - 1 - 1 - 20


def test_the_ratio_at_the_threshold_and_a_hub():
    k, km, strs, mu = P.craft_set()
    # best(0) = 12 from the entry (0, 4); (0, 2) holds 4 pairs: 4 * 3 == 12 is kept, 4 * 3 == 12 < 13 is not
    at = [(0, 2, 4, 40, 10, 10), (0, 4, 12, 120, 10, 10)]
    below = [(0, 2, 4, 40, 10, 10), (0, 4, 13, 130, 10, 10)]
    assert run(k, strs, at, ratio=3)["stats"]["n_kept"] == 2 and run(k, strs, below, ratio=3)["stats"]["n_below_ratio"] == 1
    # the one kept edge out of 0 after the drop is a chain link only while nothing else is kept INTO unitig 2 either
    assert run(k, strs, below, ratio=3)["stats"]["n_chain"] == 1 and run(k, strs, at, ratio=3)["stats"]["n_chain"] == 0
    big = [(0, 2, 2 ** 63, 2 ** 63, 1, 1)]
    r = run(k, strs, big, ratio=65536)
    assert r["stats"]["n_chain"] == 1 and r["srecs"][0]["min_pairs"] == r["srecs"][0]["sum_pairs"] == 2 ** 63
    # entries that are no pair links
    bad = [(0, 1, 5, 5, 1, 1), (0, 200, 5, 5, 1, 1), (200, 0, 5, 5, 1, 1), (4, 9, 0, 0, 0, 0)]
    assert run(k, strs, bad)["stats"]["n_ignored"] == 4 and run(k, strs, bad)["sstrs"] == strs


def test_two_islands_come_out_as_one_scaffold_with_the_hole_as_n():
    """consequence (d)"""
    k, strs, plinks, genome = S.two_islands()
    assert plinks == [(1, 2, 101, 10100, 100, 100)] and strs == [genome[1050:], U.rc(genome[:950])]
    q = S.TWO_ISLANDS_PARAMS
    res = S.scaffold(k, strs, None, plinks, q["min_pairs"], q["ratio"], q["inner"], q["min_n"], q["max_n"])
    S.check(k, strs, plinks, res, q["max_n"])
    assert res["sstrs"] == [U.rc(genome[1050:]) + "N" * 100 + U.rc(genome[:950])] and len(res["sstrs"][0]) == 2000   # the reverse complement of genome[:950] + N * 100 + genome[1050:]
    assert res["steps"] == [(1, 0, 0), (2, 100, 100)] and res["place"] == [(1, 0, 0), (0, 1, 1050)]
    assert res["srecs"][0]["n_gap_bases"] == 100 and res["srecs"][0]["min_pairs"] == res["srecs"][0]["sum_pairs"] == 101


def test_layouts_match_the_header(tmp_path):
    assert C.sizeof(ScaffoldParams) == 32 and C.sizeof(ScaffoldStats) == 80 and [f for f, _ in ScaffoldStats._fields_] == list(S.STAT_FIELDS)
    assert SCAFFOLD_DTYPE == S.SCAFFOLD_DTYPE and SCAFFOLD_STEP_DTYPE == S.STEP_DTYPE and SCAFFOLD_PLACE_DTYPE == S.PLACE_DTYPE and api.SCAFFOLD_CIRCULAR == S.CIRCULAR
    assert (SCAFFOLD_DTYPE.itemsize, SCAFFOLD_STEP_DTYPE.itemsize, SCAFFOLD_PLACE_DTYPE.itemsize) == (64, 16, 16)
    fields = [("kmx_scaffold", f) for f in SCAFFOLD_DTYPE.names] + [("kmx_scaffold_step", f) for f in SCAFFOLD_STEP_DTYPE.names] + [("kmx_scaffold_place", f) for f in SCAFFOLD_PLACE_DTYPE.names]
    fields += [("kmx_scaffold_params", f) for f, _ in ScaffoldParams._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %u %d", sizeof(kmx_scaffold_params), sizeof(kmx_scaffold), '
                   'sizeof(kmx_scaffold_step), sizeof(kmx_scaffold_place), sizeof(kmx_scaffold_stats), KMX_SCAFFOLD_CIRCULAR, KMX_ABI_VERSION);\n'
                   + "".join(f' printf(" %zu", offsetof({s}, {f}));\n' for s, f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:7] == [32, 64, 16, 16, 80, 0x80000000, 5]
    want = [SCAFFOLD_DTYPE.fields[f][1] for f in SCAFFOLD_DTYPE.names] + [SCAFFOLD_STEP_DTYPE.fields[f][1] for f in SCAFFOLD_STEP_DTYPE.names]
    want += [SCAFFOLD_PLACE_DTYPE.fields[f][1] for f in SCAFFOLD_PLACE_DTYPE.names] + [getattr(ScaffoldParams, f).offset for f, _ in ScaffoldParams._fields_]
    assert got[7:] == want == [0, 8, 16, 24, 28, 32, 36, 40, 48, 56, 0, 4, 8, 0, 4, 8, 0, 8, 12, 16, 20, 24]


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    ns, nb, par, st = C.c_uint64(0), C.c_uint64(0), ScaffoldParams(2, 0, 100, 0, 10, 0), ScaffoldStats()
    assert L.kmx_unitig_scaffold(None, 21, None, None, 0, None, None, 0, C.byref(par), None, 0, None, None, None, None, C.byref(ns), C.byref(nb), C.byref(st)) == -1
    assert L.kmx_unitig_scaffold_dev(None, 21, None, None, 0, 0, None, None, 0, C.byref(par), None, 0, None, None, None, None, C.byref(ns), C.byref(nb), C.byref(st)) == -1
    assert L.kmx_unitig_scaffold_last_phases(None, None, None) == -1


def test_facade_writers(tmp_path):
    """tests/facade_unitig_scaffold.cpp compiles against include/kmodel.hpp with the reference's flags; its three writers, which
    need no device, give the restatement's text for a hand-made result (also under the host sanitizers)"""
    strs = ["ACGTA", "CCGGT", "TTTGA"]
    res = S.scaffold(5, strs, None, [(0, 3, 5, 50, 10, 10)], 2, 0, 30, 0, 100)
    assert res["sstrs"] == ["ACGTA" + "N" * 15 + "ACCGG", "TTTGA"]
    text = S.fasta(res) + "#\n" + S.paths_tsv(res) + "#\n" + S.agp(res, strs)
    assert "s0\t6\t20\t2\tN\t15\tscaffold\tyes\tpaired-ends\n" in text and "s0\t21\t25\t3\tW\tu1\t1\t5\t-\n" in text
    for name, extra in (("plain", ()), ("san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_scaffold.cpp"),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        assert subprocess.check_output([exe, "--text-only"]).decode() == text, name
