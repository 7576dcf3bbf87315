"""The rest table's device buffers and the scratch of its sort stay on the handle from build to build (grow-only).

A rebuild must see exactly the table a new handle would build, whatever the buffers still hold from the build before:
a smaller table after a larger one (stale rows behind `entries`), a larger one after a smaller one (the buffers grow), two-word
k-mers after one-word ones (another sort, another carve of the scratch), another prefix length (map_size 4^7 -> 4^4 -> 4^7:
hash2index and the next-group table are longer than what the build uses).  Each build is compared with the CPU oracle,
computed once per shape: statistics, the files `save` writes (rest.bin is the table), the answers to stored, reverse-
complemented and absent k-mers -- on the rebuilt handle and on a handle loaded from its files.
"""
import os

import numpy as np
import pytest

import oracle_lib as O
from common import sha_file
from kmcex_amd import KModel, synth

pytestmark = pytest.mark.gpu
CI, CS, NH, NB = 1, 1023, 7, 5                     # the handle's shape: k and n change from build to build
# (k, n): rest prefix of 7 bases at k = 31, 55 and 23, of 4 bases at k = 32 (rest.hpp:78-83)
SEQUENCE = [(31, 300000), (31, 20000), (55, 60000), (32, 40000), (31, 600000), (23, 30000)]

_cases = {}


def case(k, n):
    if (k, n) not in _cases:
        km, cnt = synth.make_stream(n, k, CI, CS, seed_k=1000 + k, seed_c=n)
        o = O.OracleModel(CI, CS, NH, NB)
        o.build(k, km, cnt)
        assert o.stats().rest_entries > 0, "an empty rest table checks nothing here"
        one = km.reshape(len(cnt), -1)
        q = np.concatenate([one, synth.revcomp(km, k).reshape(len(cnt), -1), synth.random_kmers(5000, k, seed_k=0xABCDEF0123).reshape(5000, -1)]).reshape(-1)
        _cases[(k, n)] = (km, cnt, o, q, o.query_packed(k, q))
    return _cases[(k, n)]


def check(m, k, n, tmp_path, tag):
    km, cnt, o, q, want = case(k, n)
    st, so = m.stats(), o.stats()
    assert (st.attempts, st.successes, st.rest_entries) == (so.attempts, so.successes, so.rest_entries), tag
    assert np.array_equal(m.kmer_to_occ_packed(q), want), f"{tag}: answers"
    d1, d2 = str(tmp_path / f"g_{tag}"), str(tmp_path / f"o_{tag}")
    os.makedirs(d1)
    os.makedirs(d2)
    m.save(d1)
    o.save(d2)
    for f in ("header", "km.bin", "rest.bin"):
        assert sha_file(os.path.join(d1, f)) == sha_file(os.path.join(d2, f)), f"{tag}: {f}"
    m2 = KModel.load(d1)
    assert np.array_equal(m2.kmer_to_occ_packed(q), want), f"{tag}: answers of the loaded model"
    m2.close()
    assert np.array_equal(m.kmer_to_occ_packed(q), want), f"{tag}: answers after save"


def test_rebuilds_on_one_handle_see_a_fresh_table(tmp_path):
    m = KModel(CI, CS, NH, NB)
    for step, (k, n) in enumerate(SEQUENCE):
        km, cnt = case(k, n)[:2]
        m.build_packed(k, km, cnt)
        check(m, k, n, tmp_path, f"{step}_k{k}_n{n}")
    m.close()


def test_streamed_rebuild_after_a_larger_table(tmp_path):
    """begin / insert_batch / finish on a handle whose last build left a larger table"""
    m = KModel(CI, CS, NH, NB)
    km, cnt = case(31, 300000)[:2]
    m.build_packed(31, km, cnt)
    km, cnt = case(55, 60000)[:2]
    m.begin(55, [int((cnt == CI).sum())], len(cnt))
    cut = len(cnt) // 3
    m.insert_batch(km.reshape(len(cnt), -1)[:cut].reshape(-1), cnt[:cut])
    m.insert_batch(km.reshape(len(cnt), -1)[cut:].reshape(-1), cnt[cut:])
    m.finish()
    check(m, 55, 60000, tmp_path, "streamed_k55")
    m.close()
