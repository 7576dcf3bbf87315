"""CPU side of kmx_polish_seqs: the record's layout in the header and the NumPy dtype agree; the reference loop
(tests/seq_polish_ref.py) that retires every read once a pass finds nothing in it equals, byte for byte, the loop over the whole
batch; on the recipe's 608 reads the loop is worth having and ends (judged on the CPU ORACLE's result), and the result is the
one tests/golden/seq_polish_golden.json describes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seq_edit_ref as E
import seq_polish_ref as P
from common import GENOME_CASES
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
NAMES = [c[0] for c in GENOME_CASES]


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %d", sizeof(kmx_seq_polish), KMX_POLISH_MAX_PASSES);\n'
                   + "".join(f' printf(" %zu", offsetof(kmx_seq_polish, {f}));\n' for f in P.FIELDS) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, max_passes, *rest = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == 96 == api.SEQ_POLISH_DTYPE.itemsize and P.DTYPE == api.SEQ_POLISH_DTYPE
    assert max_passes == 16 == api.POLISH_MAX_PASSES == P.MAX_PASSES
    assert rest == [8 * i for i in range(12)] == [api.SEQ_POLISH_DTYPE.fields[f][1] for f in P.FIELDS]
    for s in ("kmx_polish_seqs", "kmx_polish_seqs_dev"):
        assert s in api.ABI_SYMBOLS


@functools.lru_cache(maxsize=None)
def _case(name):
    """reads, truths, flat reads, the oracle's callback (its results kept per batch) and the loop to convergence: computed
    once, shared, left unchanged"""
    import make_seq_polish_golden as G
    case = next(c for c in GENOME_CASES if c[0] == name)
    reads, truths, buf, off = G.reads_of(case, n_reads=G.TEST_READS)
    fn = P.oracle_fn(G.oracle_of(case), case[1], case[2], 1, 7, {})
    return case, reads, truths, buf, off, fn, P.polish(fn, buf, off, 8)


def _same(a, b):
    return np.array_equal(a["bases"], b["bases"]) and np.array_equal(a["offsets"], b["offsets"]) and E.same(a["records"], b["records"]) and a["passes_run"] == b["passes_run"]


@pytest.mark.parametrize("name", NAMES)
def test_the_loop_is_worth_having_and_ends(name):
    _, reads, truths, buf, off, fn, res = _case(name)
    assert len(reads) == 608
    whole = P.polish(fn, buf, off, 8, retire=False)
    assert _same(res, whole)                                     # retiring a read is exact
    h = res["history"]
    t = P.tallies(res, truths)
    print(name, t)
    assert len(h[0]["active"]) == 608 and h[1]["active"] == h[0]["edited"] and len(h[1]["edited"]) >= 20    # (observed 46 and 53)
    assert res["passes_run"] <= 3 and res["records"]["converged"].all() and not h[-1]["edited"]
    assert np.array_equal(np.diff(res["offsets"]), res["records"]["out_len"])
    assert t["reads_wrong_after_pass"][-1] <= t["reads_wrong_after_pass"][0] < P.wrong(reads, truths)
    was = [r == x for r, x in zip(reads, truths)]
    for p in h:                                                  # no read that equalled its truth stops doing so
        now = [r == x for r, x in zip(p["reads"], truths)]
        assert not any(a and not b for a, b in zip(was, now))
        was = now
    seen = [{r} for r in reads]                                  # no read returns to a string it held before
    for p in h:
        for i in p["edited"]:
            assert p["reads"][i] not in seen[i]
            seen[i].add(p["reads"][i])


@pytest.mark.parametrize("name", NAMES)
def test_max_passes_cuts_the_loop(name):
    case, reads, truths, buf, off, fn, res = _case(name)
    two = P.polish(fn, buf, off, 2)
    edited2 = res["history"][1]["edited"]
    assert two["passes_run"] == 2 and sorted(np.nonzero(two["records"]["converged"] == 0)[0].tolist()) == sorted(edited2)
    assert np.array_equal(two["bases"], res["bases"]) and np.array_equal(two["offsets"], res["offsets"])   # pass 3 edits nothing: their output is already final
    assert (two["records"]["n_passes"][edited2] == 2).all() and (res["records"]["n_passes"][edited2] == 3).all()
    for f in P.SUMS:
        assert np.array_equal(two["records"][f], res["records"][f])
    one = P.polish(fn, buf, off, 1)
    edits, rec = fn(buf, off)
    w_out, w_off = E.apply_edits(buf, off, edits)
    assert one["passes_run"] == 1 and np.array_equal(one["bases"], w_out) and np.array_equal(one["offsets"], w_off) and (one["records"]["n_passes"] == 1).all()
    for f in P.SUMS + P.LAST:
        assert np.array_equal(one["records"][f], rec[f]), f
    assert np.array_equal(one["records"]["converged"] == 0, (rec["n_sub"] + rec["n_del"] + rec["n_ins"]) > 0)


def test_result_is_the_golden():
    import make_seq_polish_golden as G
    with open(os.path.join(ROOT, "tests", "golden", "seq_polish_golden.json")) as f:
        sg = json.load(f)
    assert sorted(sg["cases"]) == sorted(NAMES) and sg["recipe"] == {"n_reads": 600}
    for name in NAMES:
        case, *_ = _case(name)
        assert G.entry(case, G.oracle_of(case)) == sg["cases"][name], name
        assert sorted(sg["cases"][name]["max_passes"]) == ["1", "2", "8"]


def test_empty_batches():
    fn = lambda b, o: (_ for _ in ()).throw(AssertionError("nothing to ask"))
    res = P.polish(fn, np.zeros(0, np.uint8), np.zeros(4, np.uint64), 3)
    want = np.zeros(3, P.DTYPE)
    want["n_passes"], want["converged"] = 1, 1
    assert E.same(res["records"], want) and not res["offsets"].any() and res["passes_run"] == 1
    assert P.polish(fn, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 3)["passes_run"] == 0


def test_facade_seq_polish_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_polish.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq_polish")])
