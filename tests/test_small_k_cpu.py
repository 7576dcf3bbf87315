"""Small k without a GPU: the CPU oracle reproduces every case of tests/golden/small_k_golden.json (recorded from the reference,
k = 4 ... 15), the reads the GPU tests count reproduce each listing under the numpy restatement of the counting rule, and the
oracle refuses k = 3, where the reference's rest table is undefined."""
import ctypes as C
import hashlib
import os
import tempfile

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import small_k as SK
from common import sha_file

GOLDEN = SK.load_golden()


def test_golden_covers_the_small_k_range():
    ks = {g["k"] for g in GOLDEN.values()}
    assert ks == set(range(4, 16))
    assert {g["ci"] for g in GOLDEN.values()} == {1, 2, 3}
    assert {g["nh"] for g in GOLDEN.values()} >= set(range(3, 13))
    assert {g["nb"] == 1 for g in GOLDEN.values()} == {True, False}
    for k in range(4, 8):                                       # a full rest table and a subset at every k <= 7
        assert {g["draws"] is None for g in GOLDEN.values() if g["k"] == k} == {True, False}
    assert sorted(GOLDEN) == sorted(SK.CASE)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_oracle_reproduces_golden(name):
    g = GOLDEN[name]
    _, k, ci, cs, nh, nb, draws, seed = SK.CASE[name]
    assert (g["k"], g["ci"], g["cs"], g["nh"], g["nb"], g["draws"], g["seed"]) == (k, ci, cs, nh, nb, draws, seed)
    km, cnt = SK.listing(name)
    assert len(km) == g["n_kmers"] and CR.listing_sha(km, cnt) == g["listing_sha256"]
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    with tempfile.TemporaryDirectory() as d:
        o.save(d)
        for f, h in g["files"].items():
            assert sha_file(os.path.join(d, f)) == h, f
    st = o.stats()
    for f, v in g["stats"].items():
        assert (list(getattr(st, f)) if f == "n_bf" else getattr(st, f)) == v, f
    q = SK.queries(k, km)
    assert len(q) == g["n_queries"] and (len(q) == 4 ** k) == (g["queries"] == "all")
    r = o.query_packed(k, q)
    assert hashlib.sha256(r.astype("<i4").tobytes()).hexdigest() == g["occ_sha256"]
    assert int(r.astype(np.int64).sum()) == g["occ_sum"] and int((r != 0).sum()) == g["occ_nonzero"]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_reads_count_to_the_listing(name):
    """what the GPU tests count: the restatement of the counting rule gives back the case's listing"""
    _, k, ci, cs, nh, nb, draws, seed = SK.CASE[name]
    km, cnt = SK.listing(name)
    buf, off = SK.reads_for_listing(km, cnt, k, ci, cs, seed)
    got_km, got_c = CR.count(buf, off, k, ci, cs)
    assert np.array_equal(got_km, km) and np.array_equal(got_c, cnt)


def test_oracle_refuses_k3():
    km = SK.all_canonical(4) >> np.uint64(2)                   # 3-mers (not all canonical: the refusal comes first)
    km = np.unique(km)
    cnt = np.ones(len(km), dtype=np.uint32)
    o = O.OracleModel(1, 255, 3, 1)
    with pytest.raises(RuntimeError):
        o.build(3, km, cnt)
    with pytest.raises(RuntimeError):
        o.build_declared(3, km, cnt, [len(km), 0, 0], len(km))
    nbf = (C.c_uint64 * 3)(len(km), 0, 0)
    shard_begin = o.L.kmo_shard_begin
    shard_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_uint64]
    assert shard_begin(o.h, 3, nbf, len(km)) == -1
    km4, cnt4 = SK.listing("k4_full")
    o.build(4, km4, np.minimum(cnt4, 255))                      # k = 4 is the smallest k a model takes
    assert o.stats().n_total == len(km4)
    assert shard_begin(o.h, 4, nbf, len(km)) == 0
