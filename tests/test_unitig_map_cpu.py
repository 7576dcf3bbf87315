"""The mapping rule of kmx_unitig_map_* without a GPU: the plain-Python restatement (tests/unitig_map_ref.py) against its
golden, the consequences the header names on every case, the record layouts, and the facade program's table writers."""
import ctypes as C
import json
import os
import subprocess

import pytest

import unitig_clean_ref as UC
import unitig_map_ref as R
import unitigs_ref as U
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def mapped(name):
    """(case, result of the restatement), computed once and left unchanged"""
    if name not in _cache:
        c = R.case(name)
        k, km, cnt, thr, strs, reads = c
        _cache[name] = (c, R.map_reads(km, k, strs, reads))
    return _cache[name]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "unitig_map_golden.json")) as f:
        return json.load(f)


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture) == sorted(R.MAP_CASES)


@pytest.mark.parametrize("name", sorted(R.MAP_CASES))
def test_restatement_equals_golden_and_keeps_its_promises(name, fixture):
    (k, km, cnt, thr, strs, reads), (segs, so, recs, hits) = mapped(name)
    g = fixture[name]
    assert (g["k"], g["thr"], g["n_listed"], g["n_unitigs"], g["reads"]) == (k, thr, len(km), len(strs), reads)
    assert g["segments"] == [[s["pos"], s["n_windows"], s["o"], s["off"]] for s in segs]
    assert g["seg_offsets"] == so and g["hits"] == hits
    assert g["records"] == [[r[f] for f in R.REC_FIELDS] for r in recs]
    R.check(k, strs, reads, segs, so, recs)                    # consequence (a), n_segments <= n_windows, the CSR against the records
    assert sum(hits) == sum(r["n_mapped"] for r in recs)
    f = R.flat(segs, so, recs, hits)
    assert f[0].dtype.itemsize == 24 and f[2].dtype.itemsize == 64 and f[1][-1] == len(segs)


def test_cases_hold_what_they_are_for():
    (k, _, _, _, strs, reads), (segs, so, recs, _) = mapped("k5_complete")
    assert all(len(s) == k for s in strs), "every window is its own unitig"
    assert len(segs) == sum(r["n_mapped"] for r in recs) > 300 and any(r["n_gaps"] for r in recs)
    (k, _, _, _, strs, reads), (segs, so, recs, _) = mapped("k33_cycle400")
    assert len(strs) == 1 and [s["off"] for s in segs[:3]][1:] == [0, 0] and recs[0]["n_segments"] == 3, "twice round a cycle: a new segment at off = 0"
    (_, _, _, _, _, reads), (_, _, recs, _) = mapped("k63_linear")
    assert {"n", "N", "R"} <= set("".join(reads)) and any(c.islower() for c in "".join(reads))
    assert sorted(len(r) for r in reads)[:4] == [0, 62, 63, 64]
    (_, _, _, _, strs, _), (segs, _, _, _) = mapped("k31_tangle")
    assert any(s["o"] & 1 for s in segs) and any(not s["o"] & 1 for s in segs)
    (_, _, _, _, _, _), (_, _, recs, _) = mapped("k21_noisy")
    assert max(r["n_segments"] for r in recs) >= 3


@pytest.mark.parametrize("name", sorted(R.MAP_CASES))
def test_reverse_complement_mirrors_the_segments(name):
    (k, km, cnt, thr, strs, reads), _ = mapped(name)
    pl = R.places(km, k, strs)
    tried = 0
    for read in reads:
        if len(read) < k or not set(read) <= set("ACGT"):
            continue
        segs = R.map_reads(km, k, strs, [read])[0]
        back = R.map_reads(km, k, strs, [U.rc(read)])[0]
        assert back == R.mirrored(k, strs, segs, len(read))
        tried += 1
        if tried == 12:
            break
    assert tried and pl


def test_counted_reads_map_onto_their_own_unitigs():
    """consequence (b): every counted window is mapped, and the hits of a unitig are the sum of its counts"""
    k = 21
    reads = U.noisy_reads(U.rand_seq(2000, 70), 400, 100, 0.01, 71)
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, urec = U.unitigs(km, cnt, k, 1)
    segs, so, recs, hits = R.map_reads(km, k, strs, reads)
    assert all(r["n_mapped"] == r["n_windows"] == len(read) - k + 1 for r, read in zip(recs, reads))
    assert hits == [r["sum_count"] for r in urec]
    assert all(r["n_gaps"] == 0 and r["first_mapped"] == 0 for r in recs)


def test_cleaned_graph_unmaps_exactly_what_was_removed():
    """consequence (c): on a cleaned graph a listed window is unmapped exactly when its entry was removed or lies below thr"""
    k, thr = 21, 2
    reads = U.noisy_reads(U.rand_seq(2000, 70), 400, 100, 0.01, 71)
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    res = UC.clean(km, cnt, k, thr)
    assert any(res["removed"]) and any(c < thr for c in cnt)
    idx = {x: i for i, x in enumerate(km)}
    pl = R.places(km, k, res["strs"])
    seen = [0, 0]
    for read in reads[:120]:
        for w, code in enumerate(R.window_codes(pl, res["strs"], k, read)):
            i = idx[U.canon(read[w:w + k])]
            gone = res["removed"][i] != 0 or cnt[i] < thr
            assert (code is None) == gone
            seen[gone] += 1
    assert min(seen) > 50


def test_invalid_sets_are_refused():
    k, thr, km, cnt, strs, _ = U.case("k7_linear300")
    R.places(km, k, strs)
    for bad in (strs + [strs[0]], strs[:-1] + [strs[-1].lower()], strs + ["ACGTAC"], strs + [U.rand_seq(40, 5)]):
        with pytest.raises(ValueError):
            R.places(km, k, bad)


def test_record_layouts_match_the_header(tmp_path):
    assert C.sizeof(api.MapSegment) == 24 == api.SEQ_SEGMENT_DTYPE.itemsize and C.sizeof(api.SeqMap) == 64 == api.SEQ_MAP_DTYPE.itemsize
    assert api.SEQ_SEGMENT_DTYPE == R.SEQ_SEGMENT_DTYPE and api.SEQ_MAP_DTYPE == R.SEQ_MAP_DTYPE
    assert [f for f, _ in api.SeqMap._fields_] == list(R.REC_FIELDS)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(kmx_map_segment), '
                   'offsetof(kmx_map_segment, n_windows), offsetof(kmx_map_segment, off), sizeof(kmx_seq_map), offsetof(kmx_seq_map, first_mapped), '
                   'offsetof(kmx_seq_map, longest), KMX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [24, 8, 16, 64, 32, 48, 5]
    assert [api.SEQ_SEGMENT_DTYPE.fields[f][1] for f in ("n_windows", "off")] == [8, 16]


def test_entry_points_refuse_a_null_handle():
    L = api.load_library()
    n = C.c_uint64(7)
    assert L.kmx_unitig_map_begin(None, 31, None, 0, None, None, 0) == -1
    assert L.kmx_unitig_map_begin_dev(None, 31, None, 0, None, None, 0, 0) == -1
    assert L.kmx_count_unitig_map_begin(None, None, None, 0) == -1
    assert L.kmx_count_unitig_map_begin_dev(None, None, None, 0, 0) == -1
    assert L.kmx_unitig_map_seqs(None, None, None, 0, None, 0, C.byref(n), None, None, None) == -1
    assert L.kmx_unitig_map_seqs_dev(None, None, None, 0, 0, None, 0, C.byref(n), None, None, None) == -1
    assert L.kmx_unitig_map_end(None) == -1
    assert b"null" in L.kmx_last_error()


def _compile(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O3", "-m64", *extra, "-std=c++11", "-I" + os.path.join(ROOT, "include"), source,
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    return exe


def test_facade_program_and_table_writers(tmp_path):
    """tests/facade_unitig_map.cpp compiles against include/kmodel.hpp with the reference's flags; its table writers, which need
    no device, write one line per segment and per unitig (also under the host sanitizers)"""
    want = "100\t3\t5\tu2\t+\t7\n102\t2\t1\tu0\t-\t0\nu0\t1\nu1\t0\nu2\t5\n"
    src = os.path.join(ROOT, "tests", "facade_unitig_map.cpp")
    assert subprocess.check_output([_compile(tmp_path, src, "facade_unitig_map"), "--tsv-only"]).decode() == want
    exe = _compile(tmp_path, src, "facade_unitig_map_san", extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    assert subprocess.check_output([exe, "--tsv-only"]).decode() == want


def test_driver_refuses_a_map_without_unitigs(tmp_path):
    exe = _compile(tmp_path, os.path.join(ROOT, "examples", "kmcex_main.cpp"), "kmcEx")
    for args in (["-g", "-M", "-k31"], ["-M", "-k31"], ["-g", "-M", "-u2", "-k30"]):
        r = subprocess.run([exe, *args, "in.fa", "out", str(tmp_path)], capture_output=True)
        assert r.returncode == 2 and b"-M" in r.stdout
