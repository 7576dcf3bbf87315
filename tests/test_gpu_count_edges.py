"""The count ceiling of kmx_count_* on the MI355X (include/kmx.h): counts saturate at 2^32 - 1 and a k-mer is listed only if
ci <= c <= 10^9.  Homopolymer runs built on the device give one k-mer exactly 10^9 windows, another 10^9 + 1 and a third
2^32 + 5, split over many sequences, calls and pieces, so the large counts are carried by the merges across pieces
(SatAdd in count_device.hip) and judged by the filter (k_keep, kCountMax).  A few thousand ordinary reads go into every
session; the expected listing is their unfiltered count by the numpy restatement plus the runs, filtered and capped here,
and the model is compared with the CPU oracle built from it.  k = 31 (one-word keys) and k = 55 (two-word keys)."""
import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_reads as R
from kmcex_amd import KModel, synth

pytestmark = pytest.mark.gpu

CX = 10 ** 9
SAT = 2 ** 32 + 5                                              # wraps to 5 without the saturating sum
RUN_BYTES = 1 << 28                                            # one device buffer of a base, reused by every call
SEQ_LEN = 1 << 22                                              # 64 sequences of 4 Mi bases per call: ~2.7e8 windows
CI, CS, NH, NB = 2, 4095, 7, 3


def _run_offsets(windows, k, seq_len=SEQ_LEN, per_call=RUN_BYTES // SEQ_LEN):
    """offsets into the run buffer, one array per call, whose sequences hold `windows` windows of k bases in all"""
    full = seq_len - k + 1
    lens = [seq_len] * (windows // full)
    if windows % full:
        lens.append(windows % full + k - 1)
    calls = []
    for i in range(0, len(lens), per_call):
        off = np.zeros(len(lens[i:i + per_call]) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens[i:i + per_call], dtype=np.uint64)
        calls.append(off)
    assert sum(int(np.diff(o).astype(np.int64).sum() - (k - 1) * (len(o) - 1)) for o in calls) == windows
    return calls


def _count_runs_dev(m, base, windows, k):
    import torch
    run = torch.full((RUN_BYTES,), ord(base), dtype=torch.uint8, device="cuda")
    for off in _run_offsets(windows, k):
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        torch.cuda.synchronize()
        m.count_seqs_dev(run.data_ptr(), d_off.data_ptr(), len(off) - 1, int(off[-1]))
        torch.cuda.synchronize()
        del d_off
    del run
    torch.cuda.empty_cache()


def _count_runs_host(m, base, windows, k):
    run = np.full(RUN_BYTES, ord(base), dtype=np.uint8)
    for off in _run_offsets(windows, k):
        m.count_seqs(run, off)


def _count_reads_dev(m, buf, off):
    import torch
    d_b = torch.from_numpy(buf).cuda()
    d_o = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), len(off) - 1, int(off[-1]))
    torch.cuda.synchronize()


def _homopolymer(base, k):
    x = synth.from_strings([base * k], k)
    return CR.packed_to_int(synth.canonical(x, k))[0]


def _expected(buf, off, k, runs):
    """the reads counted without a filter, plus the runs' windows; then ci <= c <= 10^9 and min(c, cs)"""
    km, cnt = CR.count(buf, off, k, 1, 2 ** 32 - 1)
    c = dict(zip(CR.packed_to_int(km), (int(x) for x in cnt)))
    for key, w in runs:
        c[key] = c.get(key, 0) + w
    keep = sorted((key, min(v, CS)) for key, v in c.items() if CI <= v <= CX)
    keys = [key for key, _ in keep]
    counts = np.array([v for _, v in keep], dtype=np.uint32)
    if k <= 32:
        return np.array(keys, dtype=np.uint64), counts
    return np.array([[key >> 64, key & (2 ** 64 - 1)] for key in keys], dtype=np.uint64).reshape(-1, 2), counts


def _check_model(m, k, km, cnt):
    got_km, got_c = m.count_listing()
    assert got_km.shape == km.shape and np.array_equal(got_km, km), "listing k-mers differ"
    assert np.array_equal(got_c, cnt), "listing counts differ"
    o = O.OracleModel(CI, CS, NH, NB)
    o.build(k, km, cnt)
    for a in range(NB):
        assert np.array_equal(m.download("tag", a), o.array_bytes("tag", a)), f"tag array {a}"
        assert np.array_equal(m.download("value", a), o.array_bytes("value", a)), f"value array {a}"
    assert np.array_equal(m.download("km_back"), o.array_bytes("km_back"))
    for i in range(3):
        assert np.array_equal(m.download("bf", i), o.array_bytes("bf", i)), f"bf {i}"
        assert np.array_equal(m.download("bf_back", i), o.array_bytes("bf_back", i)), f"bf_back {i}"
    s, so = m.stats(), o.stats()
    for f in ("n_total", "n_km", "attempts", "successes", "rest_entries", "km_byte_size", "byte_km_back"):
        assert getattr(s, f) == getattr(so, f), f
    assert list(s.n_bf) == list(so.n_bf)


def _reads(k):
    return R.make_reads(6000, k, n_reads=3000, seed=k, long_read=2500)


def _finish_and_check(m, k, buf, off, runs):
    km, cnt = _expected(buf, off, k, runs)
    assert m.count_finish() == len(cnt)
    _check_model(m, k, km, cnt)
    return km, cnt


def _listed(km, k, key):
    return key in set(CR.packed_to_int(km))


@pytest.mark.parametrize("k", [31, 55])
def test_listed_up_to_ten_to_the_ninth(k):
    """one k-mer with exactly 10^9 windows is listed at min(10^9, cs); one with 10^9 + 1 is not"""
    reads = _reads(k)
    buf, off = R.flatten(reads)
    a, c = _homopolymer("A", k), _homopolymer("C", k)
    m = KModel(CI, CS, NH, NB)
    m.count_begin(k)
    _count_reads_dev(m, *R.flatten(reads[:len(reads) // 2]))
    _count_runs_dev(m, "A", CX, k)
    _count_runs_dev(m, "C", CX + 1, k)
    _count_reads_dev(m, *R.flatten(reads[len(reads) // 2:]))
    runs = [(a, CX), (c, CX + 1)]
    km, cnt = _finish_and_check(m, k, buf, off, runs)
    assert _listed(km, k, a) and not _listed(km, k, c)
    m.close()


@pytest.mark.parametrize("k", [31, 55])
def test_saturated_count_is_not_listed(k):
    """2^32 + 5 windows of one k-mer saturate at 2^32 - 1 (> 10^9): absent, where a wrapped count of 5 would be listed"""
    buf, off = R.flatten(_reads(k))
    g = _homopolymer("G", k)
    m = KModel(CI, CS, NH, NB)
    m.count_begin(k)
    _count_reads_dev(m, buf, off)
    _count_runs_dev(m, "G", SAT, k)
    km, cnt = _finish_and_check(m, k, buf, off, [(g, SAT)])
    assert not _listed(km, k, g)
    m.close()


def test_host_path_at_ten_to_the_ninth():
    k = 31
    buf, off = R.flatten(_reads(k))
    a, t = _homopolymer("A", k), _homopolymer("T", k)
    assert a == t                                              # poly-T is poly-A's reverse complement: one k-mer
    c = _homopolymer("C", k)
    m = KModel(CI, CS, NH, NB)
    m.count_begin(k)
    _count_runs_host(m, "T", CX, k)
    m.count_seqs(buf, off)
    _count_runs_host(m, "C", CX + 1, k)
    km, cnt = _finish_and_check(m, k, buf, off, [(a, CX), (c, CX + 1)])
    assert _listed(km, k, a) and not _listed(km, k, c)
    m.close()
