"""The front end of a build -- k_histogram, k_classify_count, k_scan_tiles -- at the shapes where its launch geometry can go
wrong: a workgroup of k_classify_count owns a span of S = 4 tiles of 2048 k-mers, reads its counts with 16-byte loads and
lists the span's Bloom-class k-mers in LDS; k_scan_tiles runs one workgroup per chunk of 2^23 k-mers; k_histogram reads
16-byte vectors from the first aligned count on.  Everything is compared with the CPU oracle, byte for byte."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from common import CASE
from kmcex_amd import KModel, api, synth

gpu = pytest.mark.gpu
TILE, S, CHUNK = 2048, 8192, 1 << 23
K, CS, NH, NB = 31, 1023, 7, 5
KMX_E_RANGE = -5
HIST_SIZES = [1, 3, 4, 5, 1023, 2 ** 20 + 3]
HIST_SEED = 5                                  # seed of the counts: Bloom-class counts at every size, for ci 1 and 2 (checked below)


@functools.lru_cache(maxsize=None)
def _stream(n, k=K, ci=1, cs=CS, seed_k=1):
    """the first n k-mers of one sorted listing (a prefix of a listing is a listing), D1 counts; read-only"""
    km, cnt = synth.make_stream(n + n // 64 + 64, k, ci, cs, seed_k=seed_k)
    assert len(cnt) >= n
    km, cnt = km[:n], cnt[:n]
    km.flags.writeable = False
    cnt.flags.writeable = False
    return km, cnt


def _upload(km, cnt):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(km).view(np.int64).copy()).cuda(),
            torch.from_numpy(np.ascontiguousarray(cnt, dtype=np.uint32).view(np.int32).copy()).cuda())


def _check(m, o, nb):
    st, so = m.stats(), o.stats()
    assert (st.n_km, list(st.n_bf), st.km_byte_size, st.byte_km_back) == (so.n_km, list(so.n_bf), so.km_byte_size, so.byte_km_back)
    for i in range(st.bf_num):
        assert np.array_equal(m.download("bf", i), o.array_bytes("bf", i)), f"bloom filter {i}"
        assert np.array_equal(m.download("bf_back", i), o.array_bytes("bf_back", i)), f"back filter {i}"
    assert np.array_equal(m.download("km_back"), o.array_bytes("km_back"))
    for a in range(nb):
        assert np.array_equal(m.download("tag", a), o.array_bytes("tag", a)), f"tag array {a}"
        assert np.array_equal(m.download("value", a), o.array_bytes("value", a)), f"value array {a}"
    assert (st.attempts, st.successes, st.rest_entries) == (so.attempts, so.successes, so.rest_entries)


def _build_dev_and_check(k, ci, cs, nh, nb, km, cnt, m=None):
    d_km, d_cnt = _upload(km, cnt)
    m = m or KModel(ci, cs, nh, nb)
    m.build_dev(k, d_km.data_ptr(), d_cnt.data_ptr(), len(cnt))
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, np.asarray(km), np.asarray(cnt))
    _check(m, o, nb)
    o.close()
    return m


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, S - 1, S, S + 1, 3 * S + 5])
def test_launch_edges(n):
    km, cnt = _stream(3 * S + 5)
    _build_dev_and_check(K, 1, CS, NH, NB, km[:n], cnt[:n]).close()


@gpu
@pytest.mark.parametrize("mix", ["all_bloom", "no_bloom", "one_in_last_tile"])
def test_class_mixtures(mix):
    """all_bloom: more than the span's list holds, so the span goes through it half by half; one_in_last_tile: a single hashing pass
    with one lane, in a partial span"""
    n = S + TILE + 5
    km, cnt = _stream(3 * S + 5)
    km, cnt = km[:n], np.maximum(cnt[:n], 2).astype(np.uint32)
    if mix == "all_bloom":
        cnt[:] = 1
    elif mix == "one_in_last_tile":
        cnt[n - 3] = 1
    _build_dev_and_check(K, 1, CS, NH, NB, km, cnt).close()


@gpu
def test_three_bloom_classes():
    """ci = 2: three Bloom classes, the class travels with the k-mer's offset through the span's list"""
    n = 3 * S + 5
    km, _ = _stream(n)
    cnt = synth.d1_counts(n, 2, CS)
    assert all((cnt == 2 + f).sum() > 256 for f in range(3))
    _build_dev_and_check(K, 2, CS, NH, NB, km, cnt).close()


@gpu
def test_two_word_kmers():
    _, k, ci, cs, nh, nb, n = CASE["k55_nh9_nb6"]
    km, cnt = synth.make_stream(n, k, ci, cs)
    _build_dev_and_check(k, ci, cs, nh, nb, km, cnt).close()


@gpu
def test_chunk_boundary():
    """Two chunks, the second one a tile, a k-mer and 77 more: a partial tile in a partial span, and the second workgroup of
    the scan.  Compared with the oracle at full size (8.4 million k-mers: a few seconds, most of them the oracle's)."""
    n = CHUNK + TILE + 1 + 77
    km, cnt = _stream(n, seed_k=5)
    _build_dev_and_check(K, 1, CS, NH, NB, km, cnt).close()


@gpu
def test_batches_cut_inside_a_tile_from_an_unaligned_pointer():
    """kmx_begin / insert_batch_dev / finish in two batches cut at an odd offset: the second batch's counts start at a pointer
    that is not a multiple of 16, so its workgroups take the count-by-count loads"""
    n, cut = 3 * S + 5, S + 1001
    km, cnt = _stream(n)
    d_km, d_cnt = _upload(km, cnt)
    assert (d_cnt.data_ptr() + 4 * cut) % 16
    m = KModel(1, CS, NH, NB)
    m.begin(K, [int((cnt == 1).sum()), 0, 0], n)
    m.insert_batch_dev(d_km.data_ptr(), d_cnt.data_ptr(), cut)
    m.insert_batch_dev(d_km.data_ptr() + 8 * cut, d_cnt.data_ptr() + 4 * cut, n - cut)
    m.finish()
    o = O.OracleModel(1, CS, NH, NB)
    o.build(K, np.asarray(km), np.asarray(cnt))
    _check(m, o, NB)
    m.close(); o.close()


@gpu
def test_bad_counts():
    n = 3 * S + 5
    km, good = _stream(n)
    bad = good.copy()
    bad[100] = 0                                               # below ci, first workgroup
    bad[S + 3000] = CS + 1                                     # above cs, another workgroup of both kernels
    d_km, d_bad = _upload(km, bad)
    m = KModel(1, CS, NH, NB)
    with pytest.raises(api.KmxError) as e:                     # the histogram finds them
        m.build_dev(K, d_km.data_ptr(), d_bad.data_ptr(), n)
    assert e.value.code == KMX_E_RANGE and "2 k-mers" in str(e.value)
    with pytest.raises(api.KmxError) as e:
        m.count_classes_dev(d_bad.data_ptr(), n)
    assert e.value.code == KMX_E_RANGE and "2 k-mers" in str(e.value)
    m.begin(K, [int((good == 1).sum()), 0, 0], n)              # no histogram on this way in: the front end finds them
    m.insert_batch_dev(d_km.data_ptr(), d_bad.data_ptr(), n)
    with pytest.raises(api.KmxError) as e:
        m.finish()
    assert e.value.code == KMX_E_RANGE and "2 k-mers" in str(e.value)
    _build_dev_and_check(K, 1, CS, NH, NB, km, good, m=m).close()     # a clean listing right after, on the same handle


def _hist_counts(n, ci):
    return synth.d1_counts(n + 1, ci, CS, seed_c=HIST_SEED)[1:]


@pytest.mark.parametrize("ci", [1, 2])
def test_histogram_inputs_have_bloom_class_counts(ci):
    for n in HIST_SIZES:
        c = _hist_counts(n, ci)
        assert len(c) == n and ((c >= ci) & (c < ci + (1 if ci == 1 else 3))).any(), n


@gpu
@pytest.mark.parametrize("ci", [1, 2])
@pytest.mark.parametrize("n", HIST_SIZES)
def test_histogram_alone_from_an_unaligned_pointer(n, ci):
    import torch
    c = _hist_counts(n, ci)
    d = torch.from_numpy(synth.d1_counts(n + 1, ci, CS, seed_c=HIST_SEED).view(np.int32).copy()).cuda()
    assert d.data_ptr() % 16 == 0
    m = KModel(ci, CS, NH, NB)
    got = m.count_classes_dev(d.data_ptr() + 4, n)
    bf_num = 1 if ci == 1 else 3
    exp = [int(x) for x in np.bincount(c.astype(np.int64), minlength=ci + 3)[ci:ci + bf_num]] + [0] * (3 - bf_num)
    assert got == exp
    m.close()
