"""k_count_windows at its launch geometry (kmcex_amd/csrc/count_kernels.h): sequence boundaries and non-base bytes on the
edges of a lane's run of 16 windows, a wave's 1024 and a block's 4096, thousands of empty sequences inside one lane's
walk, misaligned device pointers and ragged ends, pieces that restart the kernel at every alignment, a host chunk whose
boundary area is full, and hostile offsets on the device.  The batches and their expected listings come from
tests/count_layouts.py (count_reads.count, checked there against the plain-Python dictionary count); every comparison is
exact equality of k-mers and counts.

The listings are taken with ci = 1 and a cs no count can reach, so nothing is filtered or capped away: a handle's cs is a
C int and sizes its cs + 1 occurrence table, so 2^32 - 1 cannot be asked of it; no session here counts more than CS
windows (asserted where the expected listing is made), which no count can then exceed."""
import ctypes as C

import numpy as np
import pytest

import count_layouts as CL
import count_reads as CR
import seq_reads as R
from kmcex_amd import KModel
from test_gpu_count import assert_same_model

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
CI, CS = 1, 65535
PAD = 256                                                      # guard bytes / words round a device buffer (keeps torch's alignment)


def _uncapped(cnt):
    assert int(cnt.astype(np.int64).sum()) <= CS                # the windows of the session: no count can pass CS
    return cnt


def on_device(buf, off, shift=0, off_guard=5000):
    """the bases at base + PAD + shift inside a larger tensor of 'A' (a read past either end would count poly-A windows) and
    the offsets in the middle of a larger tensor of `off_guard` (a read past either end would cut a sequence there)"""
    import torch
    hb = np.full(PAD + shift + len(buf) + PAD, ord("A"), dtype=np.uint8)
    hb[PAD + shift:PAD + shift + len(buf)] = buf
    ho = np.full(PAD + len(off) + PAD, off_guard, dtype=np.uint64)
    ho[PAD:PAD + len(off)] = off
    d_b = torch.from_numpy(hb).cuda()
    d_o = torch.from_numpy(ho.view(np.int64)).cuda()
    assert d_b.data_ptr() % 4 == 0 and d_o.data_ptr() % 8 == 0
    return (d_b, hb, d_o, ho), d_b.data_ptr() + PAD + shift, d_o.data_ptr() + 8 * PAD


def feed(m, buf, off, dev, shift=0, n_bases=None):
    """one kmx_count_seqs (host) or kmx_count_seqs_dev call; the device buffers are read back and must be unchanged"""
    if not dev:
        m.count_seqs(buf, off)
        return
    import torch
    n = int(off[-1]) if n_bases is None else n_bases
    (d_b, hb, d_o, ho), p_b, p_o = on_device(buf[:n], off, shift)
    torch.cuda.synchronize()
    m.count_seqs_dev(p_b, p_o, len(off) - 1, n)
    torch.cuda.synchronize()
    assert np.array_equal(d_b.cpu().numpy(), hb) and np.array_equal(d_o.cpu().numpy().view(np.uint64), ho)


_RC_OF_NOTHING = {}


def rc_of_nothing(k):
    """what kmx_build_dev answers for an empty listing: kmx_count_finish of nothing listed answers the same"""
    if k not in _RC_OF_NOTHING:
        m = KModel(CI, CS, NH, NB)
        _RC_OF_NOTHING[k] = m.L.kmx_build_dev(m.h, k, None, None, 0)
    return _RC_OF_NOTHING[k]


def finish_equals(m, k, km, cnt, what):
    """kmx_count_finish returns the length of the expected listing and kmx_count_listing is that listing, k-mers and counts"""
    n = C.c_uint64(12345)
    rc = m.L.kmx_count_finish(m.h, C.byref(n))
    assert n.value == len(km), what
    if len(km):
        assert rc == 0, what
        got_km, got_c = m.count_listing()
        assert got_km.shape == km.shape and np.array_equal(got_km, km), f"{what}: listing k-mers differ"
        assert np.array_equal(got_c, cnt), f"{what}: listing counts differ"
        return
    assert rc == rc_of_nothing(k), what
    if rc == 0:
        assert m.L.kmx_count_listing(m.h, None, None, 0, C.byref(n)) == 0 and n.value == 0, what


def count_once(k, buf, off, dev, shift=0):
    m = KModel(CI, CS, NH, NB)
    m.count_begin(k)
    feed(m, buf, off, dev, shift)
    return m


@pytest.mark.parametrize("k", [5, 16, 17, 31, 32, 33, 64])
def test_layouts_device_and_host(k):
    for name in CL.LAYOUTS:
        for dirty in (False, True):
            buf, off, km, cnt = CL.case(name, k, dirty)
            _uncapped(cnt)
            for dev in (True, False):
                m = count_once(k, buf, off, dev)
                finish_equals(m, k, km, cnt, (name, "dirty" if dirty else "clean", "device" if dev else "host"))


RAGGED = {k: [k - 1, k, k + 1, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 4096 + k, 2 * 4096 + k + 1] for k in (31, 55)}
_ragged_cache = {}


def ragged_case(k, n, random_cuts):
    """the first n bases as one sequence of the clean text, or under random_with_empties on the dirty text (whose N at
    4096 + k - 2 is then the last halo byte of the first tile when n = 4096 + k - 1)"""
    key = (k, n, random_cuts)
    if key not in _ragged_cache:
        if random_cuts:
            buf, off = CL.dirty_text(k)[:n], CL.clip(CL.layout("random_with_empties", k), n)
        else:
            buf, off = CL.text()[:n], np.array([0, n], dtype=np.uint64)
        km, cnt = CL.expected(buf, off, k)
        _ragged_cache[key] = (buf, off, km, _uncapped(cnt))
    return _ragged_cache[key]


@pytest.mark.parametrize("a", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 55])
def test_unaligned_device_pointer_and_ragged_end(k, a):
    """the bases at base + a: the byte-staging path in every block; a = 0 would take the dword path, which the ragged ends of
    test_ragged_end_aligned take with a tail of 1 to 3 bytes; 2 * 4096 + k + 1 leaves a last block of halo positions only"""
    listed = 0
    for n in RAGGED[k]:
        for random_cuts in (False, True):
            buf, off, km, cnt = ragged_case(k, n, random_cuts)
            listed += len(km)
            finish_equals(count_once(k, buf, off, True, shift=a), k, km, cnt, (n, random_cuts, a))
    assert listed > 6 * 1500


@pytest.mark.parametrize("k", [31, 55])
def test_ragged_end_aligned(k):
    """the same ragged ends at an aligned pointer: dword loads, then the 1 to 3 bytes left over (n % 4 takes every value)"""
    assert {n % 4 for n in RAGGED[k]} == {0, 1, 2, 3}
    for n in RAGGED[k]:
        for random_cuts in (False, True):
            buf, off, km, cnt = ragged_case(k, n, random_cuts)
            finish_equals(count_once(k, buf, off, True, shift=0), k, km, cnt, (n, random_cuts))


def _thirds(which):
    """the clean text, one sequence, with its first or its middle third N"""
    t = CL.text()
    third = CL.N // 3
    t[which * third:(which + 1) * third] = ord("N")
    return t, np.array([0, CL.N], dtype=np.uint64)


@pytest.mark.parametrize("k", [31, 55])
def test_piece_edges(k, monkeypatch):
    """KMX_COUNT_PIECE relaunches the kernel at p0 = a multiple of the piece: 4096 (block-aligned), 4095 and 4097 (odd and
    even alignments that drift), 1040 (65 runs); 17 is shorter than k - 1 (a host chunk shorter than k, a piece shorter than a
    lane's prologue); with a third of the input N, pieces that count nothing come between (or before) those that do"""
    inputs = [("cuts_round_block_edge", CL.case("cuts_round_block_edge", k, False)[:2], (4096, 4095, 4097, 1040)),
              ("dirty one_sequence", CL.case("one_sequence", k, True)[:2], (4096, 4095, 4097, 1040)),
              ("first 600 bases", (CL.dirty_text(k)[:600], np.array([0, 200, 200, 600], dtype=np.uint64)), (17,)),
              ("middle third N", _thirds(1), (1000,)),
              ("first third N", _thirds(0), (1000,))]
    for what, (buf, off), pieces in inputs:
        km, cnt = CL.expected(buf, off, k)
        _uncapped(cnt)
        assert len(km) >= CL.MIN_LISTED
        monkeypatch.delenv("KMX_COUNT_PIECE", raising=False)
        ref = count_once(k, buf, off, False)
        finish_equals(ref, k, km, cnt, (what, "no hook"))
        for piece in pieces:
            monkeypatch.setenv("KMX_COUNT_PIECE", str(piece))
            for dev in (True, False):
                m = count_once(k, buf, off, dev)
                finish_equals(m, k, km, cnt, (what, piece, "device" if dev else "host"))
                assert_same_model(ref, m, NB)


@pytest.mark.parametrize("k", [64, 31])
def test_boundary_slot_is_full_on_the_host_path(k, monkeypatch):
    """sequences of one base each: a host chunk of C windows carries C + k - 1 bases and so C + k boundaries, which for
    k = 64 is the whole boundary area of its slot (C + 64 words); a second call of ordinary reads follows in the same session"""
    buf, off, _, _ = CL.case("all_length_1", k, True)
    reads = R.make_reads(6000, k, n_reads=30, seed=5, long_read=900)
    rbuf, roff = R.flatten(reads)
    both = np.concatenate([buf, rbuf])
    both_off = np.concatenate([off, roff[1:] + off[-1]])
    km, cnt = CL.expected(both, both_off, k)
    _uncapped(cnt)
    assert len(km) > 1000
    for piece in (64, 1000):
        assert int(np.argmax(np.diff(off.astype(np.int64)) > 1)) > 4 * piece      # whole chunks of one-base sequences
        monkeypatch.setenv("KMX_COUNT_PIECE", str(piece))
        m = KModel(CI, CS, NH, NB)
        m.count_begin(k)
        m.count_seqs(buf, off)
        m.count_seqs(rbuf, roff)
        finish_equals(m, k, km, cnt, piece)


@pytest.mark.parametrize("k", [31, 33])
def test_many_calls_one_kmer_each(k):
    """300 calls of one k-base sequence each, device and host calls interleaved in one session: the same k-mer, its reverse
    complement or one of 5 others (k is odd: no k-mer is its own reverse complement)"""
    import torch
    rng = np.random.default_rng(900 + k)
    g = R.genome_ascii(400)
    seqs = [g[j * 50:j * 50 + k].copy() for j in range(6)]
    seqs.insert(1, R._COMP[seqs[0][::-1]])
    assert len({s.tobytes() for s in seqs}) == 7
    off = np.array([0, k], dtype=np.uint64)
    on_dev = [on_device(s, off) for s in seqs]
    torch.cuda.synchronize()
    picks = rng.integers(0, 7, size=300)
    picks[:4] = [0, 1, 0, 1]
    m = KModel(CI, CS, NH, NB)
    m.count_begin(k)
    for i, j in enumerate(picks):
        if i % 3 == 1:
            m.count_seqs(seqs[j], off)
        else:
            m.count_seqs_dev(on_dev[j][1], on_dev[j][2], 1, k)
    torch.cuda.synchronize()
    d = CR.dict_count([seqs[j].tobytes() for j in picks], k)
    assert len(d) == 6 and sum(d.values()) == 300 <= CS and max(d.values()) >= int((picks <= 1).sum())     # (nothing capped)
    assert m.count_finish() == 6
    km, cnt = m.count_listing()
    ints = CR.packed_to_int(km)
    assert ints == sorted(d) and [d[x] for x in ints] == cnt.tolist()


def test_bad_offsets_on_the_device():
    """include/kmx.h: "bad offsets miscount, never read outside the buffers".  k_count_windows reads offs only through
    seq_off (indices 0 .. n_seqs) and the bounded seq_upper, and bases only below b_end <= n_bases, whatever the offsets hold;
    every position is one lane's window at most once and a window is counted only after k bases in a row, so what is listed
    occurs in the buffer taken as one sequence, no more often than there.  The buffers lie inside larger tensors, which are
    unchanged afterwards, and a good session on the same handle is exact."""
    import torch
    k = 31
    buf, off, km, cnt = CL.case("random_with_empties", k, True)
    n, n_seqs = CL.N, len(off) - 1
    one_km, one_cnt = CL.case("one_sequence", k, True)[2:]
    bound = dict(zip(CR.packed_to_int(one_km), one_cnt.tolist()))
    _uncapped(one_cnt)                                           # a session lists no more than these windows: nothing capped
    _uncapped(cnt)
    mutations = {}
    bad = off.copy()
    bad[n_seqs // 2:] += np.uint64(n)
    mutations["past the end"] = (bad, n)
    bad = off.copy()
    bad[1:-1] = bad[1:-1][::-1]
    mutations["decreasing"] = (bad, n)
    bad = off.copy()
    bad[3::7] = np.uint64(2 ** 64 - 1)
    mutations["huge"] = (bad, n)
    bad = off.copy()
    i = int(np.argmax(np.diff(off.astype(np.int64)) > 100))
    bad[i], bad[i + 1] = off[i + 1], off[i]
    assert bad[i] > bad[i + 1]
    mutations["one swapped pair"] = (bad, n)
    bad = off.copy()
    bad[0] = 37
    mutations["offsets[0] > 0"] = (bad, n)
    mutations["n_bases past offsets[n_seqs]"] = (CL.clip(off, n - 500), n)
    m = KModel(CI, CS, NH, NB)
    for what, (bad, n_bases) in mutations.items():
        m.count_begin(k)
        feed(m, buf, bad, True, n_bases=n_bases)                # (asserts the tensors round the buffers unchanged)
        m.count_finish()
        got_km, got_c = m.count_listing()
        ints = CR.packed_to_int(got_km)
        assert ints == sorted(set(ints)), what
        for x, c in zip(ints, got_c.tolist()):
            assert 1 <= c <= bound.get(x, 0), (what, x, c)
    m.count_begin(k)
    feed(m, buf, off, True)
    finish_equals(m, k, km, cnt, "good offsets after the bad ones")
    torch.cuda.synchronize()
