"""kmx_unitigs*, kmx_count_unitigs* on the MI355X: strings, offsets and records equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitigs_ref.py) gives, for the host and the device variant, on every case of U.CASES (linear
pieces, isolated cycles, dense and complete graphs, tangles at one- and two-word k, extreme counts and thresholds, one bucket
of the index) and on sweeps that stay out of the fixture: every cycle length from 2 to 130 alone in its listing, paths of
exactly 2^j - 1, 2^j and 2^j + 1 nodes, listing sizes around the launch geometry; the documented round bounds; the tight
capacity of the complete graph; refusals of bad listings in one and two words; calls of every size and word count in turn on
one handle; a counted session; closure; allocation failure; the FASTA of the facade and the driver."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing


@functools.lru_cache(maxsize=None)
def ref(name):
    """(k, thr, packed k-mers, counts, k-mer strings, (buf, off, rec) of the restatement), computed once"""
    k, thr, km, cnt, strs, recs = U.case(name)
    return k, thr, U.pack(km, k), np.asarray(cnt, dtype=np.uint32), km, U.flat(strs, recs)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unitigs_golden.json")) as f:
        return json.load(f)["cases"]


def listed(seqs, k, thr=1):
    """(packed k-mers, counts, recs, (buf, off, rec)) of the restatement for sequences that are no case"""
    km, cnt = U.listing_of(U.count_kmers(seqs, k))
    strs, recs = U.unitigs(km, cnt, k, thr)
    return U.pack(km, k), np.asarray(cnt, dtype=np.uint32), recs, U.flat(strs, recs)


def lg(n):
    """ceil(log2 n)"""
    return (n - 1).bit_length()


def same(got, want, what=""):
    buf, off, rec = got
    wbuf, woff, wrec = want
    assert np.array_equal(np.asarray(off, dtype=np.uint64), woff), f"{what}: offsets differ"
    assert np.asarray(buf).tobytes() == wbuf.tobytes(), f"{what}: strings differ"
    assert np.asarray(rec).tobytes() == wrec.tobytes(), f"{what}: records differ"


def from_torch(got):
    buf, off, rec = got
    return buf.cpu().numpy(), off.cpu().numpy().view(np.uint64), rec.cpu().numpy().reshape(-1).view(UNITIG_DTYPE)


def run_dev(m, km, cnt, k, thr):
    import torch
    d_km = torch.from_numpy(np.ascontiguousarray(km).view(np.int64).reshape(-1)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    return from_torch(m.unitigs_dev(d_km, d_cnt, k, thr))


@pytest.mark.parametrize("name", [n for n in U.CASES if not n.startswith("reads")])
def test_equals_the_restatement(name):
    """small k with self-loops and hairpins; isolated cycles, alone and beside a path; linear pieces; one path of thousands of
    k-mers (more than 12 doubling rounds); two-word k-mers, circular and linear; the complete graphs of k = 5 and 7 and random
    subsets of every density down to 0.02 at k = 11, with counts of 0 and 0xFFFFFFFF, sums above 2^32, thr = 0 and
    thr = 0xFFFFFFFF; tangles (bubbles, tips, a hairpin, self-loops, nine cycles, the largest canonical k-mers) at k = 31 and in
    two words up to k = 63, at thr 1 and 2; every cycle length from 2 to 130 in one listing; a cycle that closes at thr = 2 only;
    a listing in one bucket of the index.  The rounds stay within the bounds of include/kmx.h: 2 ceil(log2 n) + 2, and
    ceil(log2 n) + 1 where nothing is circular (a path is never ranked twice)"""
    k, thr, km, cnt, _, want = ref(name)
    m = KModel(1, 1023, NH, NB)
    same(m.unitigs(km, cnt, k, thr), want, "host")
    rounds = m.unitigs_phases()["rounds"]
    assert rounds <= 2 * lg(len(cnt)) + 2, (rounds, len(cnt))
    if fixture()[name]["circular"] == 0:
        assert rounds <= lg(len(cnt)) + 1, (rounds, len(cnt))
    if name == "k15_long_path":
        assert rounds > 12
    same(run_dev(m, km, cnt, k, thr), want, "device")
    same(m.unitigs(km, cnt, k, thr), want, "second call on the same handle")


@pytest.mark.parametrize("k", [31, 33])
def test_every_cycle_length_alone(k):
    """a cycle of L nodes and nothing else, L = 2 .. 130 (below k the string is periodic): n = L, so the round limit is as tight
    as it gets, and the running minimum has to cover the cycle within it"""
    m = KModel(1, 1023, NH, NB)
    for L, s in U.all_cycles(k).items():
        km, cnt, recs, want = listed([s], k)
        assert len(cnt) == L and [(r["n_kmers"], r["circular"]) for r in recs] == [(L, 1)], L
        same(m.unitigs(km, cnt, k, 1), want, f"host, L = {L}")
        assert m.unitigs_phases()["rounds"] <= 2 * lg(L) + 2, L
        same(run_dev(m, km, cnt, k, 1), want, f"device, L = {L}")


PATH_LENGTHS = (1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)


@pytest.mark.parametrize("k", [15, 31, 33, 63])
def test_exact_path_lengths(k):
    """a path of exactly m nodes and nothing else: it settles within ceil(log2 m) + 1 rounds (the last one moves nothing) and is
    not taken for a cycle, also where m = n = 2^j"""
    m = KModel(1, 1023, NH, NB)
    for n in PATH_LENGTHS:
        km, cnt, recs, want = listed([U.rand_seq(n + k - 1, 5000 + n)], k)
        assert len(cnt) == n and [(r["n_kmers"], r["circular"]) for r in recs] == [(n, 0)], n
        got = m.unitigs(km, cnt, k, 1)
        same(got, want, f"host, m = {n}")
        assert int(got[2]["circular"].sum()) == 0
        assert m.unitigs_phases()["rounds"] <= lg(max(n, 2)) + 1, n
        same(run_dev(m, km, cnt, k, 1), want, f"device, m = {n}")


def test_listing_sizes_at_the_launch_edges():
    """n + 1 threads in blocks of 256 (index, mark, emit), 32 entries per block (adjacency): the first n entries of a dense
    listing, which are a listing"""
    k, thr, km, cnt, km_s, _ = ref("k7_half_thr1")
    m = KModel(1, 1023, NH, NB)
    for n in (1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513):
        want = U.flat(*U.unitigs(km_s[:n], cnt[:n].tolist(), k, thr))
        same(m.unitigs(km[:n], cnt[:n], k, thr), want, f"host, n = {n}")
        same(run_dev(m, km[:n], cnt[:n], k, thr), want, f"device, n = {n}")


def test_the_tight_capacity():
    """the complete graph: every node its own unitig of k bytes, so rec_capacity = nodes and seq_capacity = nodes * k are
    needed in full; they suffice, and one less of either is KMX_E_RANGE with nothing written"""
    import torch
    k, thr, km, cnt, _, (wbuf, woff, wrec) = ref("k5_complete")
    m = KModel(1, 1023, NH, NB)
    d_km = torch.from_numpy(km.view(np.int64)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    args = (k, d_km.data_ptr(), d_cnt.data_ptr(), len(cnt), thr)
    nu = len(cnt)
    nb = nu * k
    assert (len(wrec), len(wbuf)) == (nu, nb)
    rc, gu, gb, seq, offs, rec = raw(m, m.L.kmx_unitigs_dev, args, nb, nu)
    assert (rc, gu, gb) == (0, nu, nb)
    assert seq[:nb].tobytes() == wbuf.tobytes() and np.all(seq[nb:] == 0xA5)
    assert np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(offs[nu + 1:] == -6)
    assert rec[:nu * 40].tobytes() == wrec.tobytes() and np.all(rec[nu * 40:] == 0xA5)
    for sc, rcap in ((nb - 1, nu), (nb, nu - 1)):
        rc, gu, gb, seq, offs, rec = raw(m, m.L.kmx_unitigs_dev, args, sc, rcap)
        assert (rc, gu, gb) == (-5, nu, nb)
        assert np.all(seq == 0xA5) and np.all(offs == -6) and np.all(rec == 0xA5)


@pytest.mark.parametrize("thr", [1, 3])
def test_thr_on_a_counted_session(thr):
    """reads at 20x with 1 % errors over a 5000-base genome, counted through kmx_count_*: count_unitigs == unitigs on the
    downloaded listing == the device variants == the restatement; the model the session built answers as before"""
    k, _, km, cnt, km_s, want = ref(f"reads_thr{thr}")
    reads = U.CASES[f"reads_thr{thr}"]()[2]
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    assert m.count_finish() == len(cnt)
    lk, lc = m.count_listing()
    assert np.array_equal(lk, km) and np.array_equal(lc, cnt), "the listing is not the restatement's"
    probe = km_s[:: max(len(km_s) // 200, 1)]
    before = m.kmer_to_occ(probe)
    got = m.count_unitigs(thr)
    same(got, want, "count_unitigs")
    assert (len(got[1]) - 1 > 1000) if thr == 1 else (len(got[1]) - 1 < 10)
    same(from_torch(m.count_unitigs_dev(thr)), want, "count_unitigs_dev")
    same(m.unitigs(lk, lc, k, thr), want, "unitigs on the downloaded listing")
    same(run_dev(m, lk, lc, k, thr), want, "unitigs_dev on the downloaded listing")
    assert m.kmer_to_occ(probe) == before
    lk2, lc2 = m.count_listing()
    assert np.array_equal(lk2, lk) and np.array_equal(lc2, lc), "the listing changed"


def test_closure_at_2e5_nodes():
    """counting the k-mers of the emitted unitigs (ci = 1) lists exactly the node set"""
    k, thr = 31, 2
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = acgt[rng.integers(0, 4, 200000)]
    g2 = g.copy()
    hit = rng.random(g2.size) < 0.002                            # a second copy with substitutions: its own k-mers count 1
    g2[hit] = acgt[(np.searchsorted(acgt, g2[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    buf = np.concatenate([g, g, g2])
    off = np.array([0, g.size, 2 * g.size, 3 * g.size], dtype=np.uint64)
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(buf, off)
    m.count_finish()
    km, cnt = m.count_listing()
    nodes = km[cnt >= thr]
    assert 180000 < len(nodes) < len(km)
    ubuf, uoff, rec = m.count_unitigs(thr)
    assert int(rec["n_kmers"].sum()) == len(nodes) and int(rec["sum_count"].sum()) == int(cnt[cnt >= thr].sum())
    assert np.array_equal(np.diff(uoff.astype(np.int64)), rec["n_kmers"].astype(np.int64) + k - 1)
    assert np.all(np.diff(rec["first_node"].astype(np.int64)) > 0)
    m2 = KModel(1, 1023, NH, NB)
    m2.count_begin(k)
    m2.count_seqs(ubuf, uoff)
    m2.count_finish()
    km2, cnt2 = m2.count_listing()
    assert np.array_equal(km2, nodes), "the unitigs' k-mers are not the node set"
    assert np.all(cnt2 == 1), "a node lies in two unitigs, or twice in one"


def raw(m, fn, args, seq_cap, rec_cap, with_rec=True, canary=0xA5, give_seq=True):
    """one call on device buffers that are longer than the capacities it is told: -> (rc, n_unitigs, n_bases, seq, offs, rec)"""
    import torch
    seq = torch.full((seq_cap + 64,), canary, dtype=torch.uint8, device="cuda")
    offs = torch.full((rec_cap + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    rec = torch.full(((rec_cap + 2) * 40,), canary, dtype=torch.uint8, device="cuda")
    nu, nb = C.c_uint64(0), C.c_uint64(0)
    rc = fn(m.h, *args, seq.data_ptr() if give_seq else None, seq_cap, offs.data_ptr(), rec.data_ptr() if with_rec else None, rec_cap, C.byref(nu), C.byref(nb))
    torch.cuda.synchronize()
    return rc, nu.value, nb.value, seq.cpu().numpy(), offs.cpu().numpy(), rec.cpu().numpy()


def test_capacities_sizing_and_canaries():
    import torch
    k, thr, km, cnt, _, (wbuf, woff, wrec) = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    d_km = torch.from_numpy(km.view(np.int64)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    args = (k, d_km.data_ptr(), d_cnt.data_ptr(), len(cnt), thr)
    nu, nb = len(wrec), len(wbuf)
    fn = m.L.kmx_unitigs_dev
    # the sizing call: counts only
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu, give_seq=False)
    assert (rc, gu, gb) == (0, nu, nb) and np.all(seq == 0xA5) and np.all(offs == -6) and np.all(rec == 0xA5)
    # exact capacities: everything inside, nothing behind
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu)
    assert (rc, gu, gb) == (0, nu, nb)
    assert seq[:nb].tobytes() == wbuf.tobytes() and np.all(seq[nb:] == 0xA5)
    assert np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(offs[nu + 1:] == -6)
    assert rec[:nu * 40].tobytes() == wrec.tobytes() and np.all(rec[nu * 40:] == 0xA5)
    # rec == NULL
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu, with_rec=False)
    assert rc == 0 and seq[:nb].tobytes() == wbuf.tobytes() and np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(rec == 0xA5)
    # one short in each dimension: KMX_E_RANGE, exact needs, nothing at or behind a capacity
    for sc, rcap in ((nb - 1, nu), (nb, nu - 1)):
        rc, gu, gb, seq, offs, rec = raw(m, fn, args, sc, rcap)
        assert (rc, gu, gb) == (-5, nu, nb)
        assert np.all(seq[sc:] == 0xA5) and np.all(offs[rcap + 1:] == -6) and np.all(rec[rcap * 40:] == 0xA5)
    # the host variant reports the same
    obuf = np.full(nb + 8, 0xA5, dtype=np.uint8)
    ooff = np.zeros(nu + 1, dtype=np.uint64)
    cu, cb = C.c_uint64(0), C.c_uint64(0)
    rc = m.L.kmx_unitigs(m.h, k, km.ctypes.data, cnt.ctypes.data, len(cnt), thr, obuf.ctypes.data, nb - 1, ooff.ctypes.data, None, nu, C.byref(cu), C.byref(cb))
    assert (rc, cu.value, cb.value) == (-5, nu, nb) and np.all(obuf[nb - 1:] == 0xA5)


def test_empty_and_thr_above_every_count():
    import torch
    k, _, km, cnt, _, _ = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    for kk, cc, thr in ((km[:0], cnt[:0], 1), (km, cnt, int(cnt.max()) + 1)):
        buf, off, rec = m.unitigs(kk, cc, k, thr)
        assert len(buf) == 0 and len(rec) == 0 and off.tolist() == [0]
        d_km = torch.from_numpy(np.ascontiguousarray(kk).view(np.int64)).cuda()
        d_cnt = torch.from_numpy(np.ascontiguousarray(cc).view(np.int32)).cuda()
        rc, gu, gb, seq, offs, _ = raw(m, m.L.kmx_unitigs_dev, (k, d_km.data_ptr() or None, d_cnt.data_ptr() or None, len(cc), thr), 4, 4)
        assert (rc, gu, gb) == (0, 0, 0) and offs[0] == 0 and np.all(offs[1:] == -6) and np.all(seq == 0xA5)


def test_bad_listings_and_arguments():
    k, _, km, cnt, km_s, want = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    swapped = km.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    dup = km.copy()
    dup[20] = dup[19]
    noncanon = km.copy()
    i = next(j for j, s in enumerate(km_s) if (j == 0 or U.rc(s) > km_s[j - 1]) and (j + 1 == len(km_s) or U.rc(s) < km_s[j + 1]))
    noncanon[i] = U.pack([U.rc(km_s[i])], k)[0]                    # still ascending, no longer canonical
    assert np.all(np.diff(noncanon.astype(np.int64)) > 0)
    wide = km.copy()
    wide[-1] |= np.uint64(1) << np.uint64(2 * k + 3)
    for bad in (swapped, dup, noncanon, wide):
        with pytest.raises(KmxError) as e:
            m.unitigs(bad, cnt, k, 1)
        assert e.value.code == -1
    for kk in (4, 6, 30, 32, 64, 3, 65):                            # even, or out of range
        with pytest.raises(KmxError) as e:
            m.unitigs(np.zeros(2 * ((kk + 31) // 32), np.uint64), np.ones(2, np.uint32), kk, 1)
        assert e.value.code == -1
    nu, nb = C.c_uint64(0), C.c_uint64(0)
    assert m.L.kmx_unitigs_dev(m.h, 31, None, None, 1 << 31, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    same(m.unitigs(km, cnt, k, 1), want, "after the refusals")       # the handle is still usable


def refused(m, km, cnt, k, what):
    for call in (m.unitigs, lambda *a: run_dev(m, *a)):
        with pytest.raises(KmxError) as e:
            call(np.ascontiguousarray(km), cnt[:len(km)], k, 1)
        assert e.value.code == -1, what


@pytest.mark.parametrize("k", [33, 63])
def test_bad_listings_in_two_words(k):
    """the order lies in the high words alone, or in the low words alone; the first, the last and the entries on both sides of a
    block of 256 threads; the mask of the high word.  KMX_E_ARG from both variants, and the handle answers the next call"""
    seq = U.rand_seq(300 + k - 1, 70 + k)
    km, cnt, _, want = listed([seq], k)
    km_s = U.unpack(km, k)
    assert km.shape == (300, 2)
    m = KModel(1, 1023, NH, NB)
    i, j = next((i, j) for i in range(300) for j in range(i + 1, 300) if km[i, 0] < km[j, 0] and km[i, 1] > km[j, 1])
    refused(m, km[[j, i]], cnt, k, "high words descending, low words ascending")
    same(m.unitigs(km[[i, j]], cnt[:2], k, 1), U.flat(*U.unitigs([km_s[i], km_s[j]], [1, 1], k, 1)), "the two in their order")
    a, b = U.equal_high_words(k, k)
    pair = U.pack([a, b], k)
    assert pair[0, 0] == pair[1, 0] and pair[0, 1] < pair[1, 1]
    refused(m, pair[[1, 0]], cnt, k, "equal high words, low words descending")
    same(m.unitigs(pair, cnt[:2], k, 1), U.flat(*U.unitigs([a, b], [1, 1], k, 1)), "the two in their order")
    dup = km.copy()
    dup[-1] = dup[-2]
    refused(m, dup, cnt, k, "the last two entries equal")
    for x in (0, 255):
        swapped = km.copy()
        swapped[[x, x + 1]] = swapped[[x + 1, x]]
        refused(m, swapped, cnt, k, f"entries {x} and {x + 1} swapped")
    noncanon = km.copy()
    i = next(j for j, s in enumerate(km_s) if (j == 0 or U.rc(s) > km_s[j - 1]) and (j + 1 == len(km_s) or U.rc(s) < km_s[j + 1]))
    noncanon[i] = U.pack([U.rc(km_s[i])], k)[0]                    # still ascending, no longer canonical
    assert U.unpack(noncanon, k) == sorted(U.unpack(noncanon, k))
    refused(m, noncanon, cnt, k, "not canonical")
    wide = km.copy()
    wide[-1, 0] |= np.uint64(1) << np.uint64(2 * k - 64)             # bit 2k of the k-mer, the lowest the mask cuts: 66 or 126
    refused(m, wide, cnt, k, "bit 2k")
    if k == 63:
        top = km.copy()
        top[-1, 0] |= np.uint64(1) << np.uint64(63)                  # bit 127, the highest of the two words
        refused(m, top, cnt, k, "bit 127")
    same(m.unitigs(km, cnt, k, 1), want, "host after the refusals")
    same(run_dev(m, km, cnt, k, 1), want, "device after the refusals")


def test_bad_listing_bit_62_at_k31():
    """bit 62 is bit 2k at the widest one-word k: the one-word mask stops right below it"""
    k = 31
    km, cnt, _, want = listed([U.rand_seq(300 + k - 1, 70 + k)], k)
    m = KModel(1, 1023, NH, NB)
    wide = km.copy()
    wide[-1] |= np.uint64(1) << np.uint64(62)
    refused(m, wide, cnt, k, "bit 62")
    same(m.unitigs(km, cnt, k, 1), want, "host after the refusal")
    same(run_dev(m, km, cnt, k, 1), want, "device after the refusal")


def test_one_handle_through_sizes_and_word_counts():
    """the work arrays stay on the handle by capacity: a small call after a large one, two words after one and back, a counted
    session in between.  Every answer is the restatement's, and a fresh handle gives the reused one's bytes: the output is a
    function of (listing, thr) alone"""
    m = KModel(1, 1023, NH, NB)

    def host(name):
        k, thr, km, cnt, _, want = ref(name)
        got = m.unitigs(km, cnt, k, thr)
        same(got, want, name)
        return got

    first = host("k11_sparse")
    host("k5_cycle2")
    host("tangle_k63_thr1")
    host("k7_complete")
    host("tangle_k31_thr2")
    k, thr, km, cnt, _, want = ref("tangle_k31_thr1")
    m.count_begin(k)
    m.count_seqs(U.CASES["tangle_k31_thr1"]()[2])
    assert m.count_finish() == len(cnt)
    counted = m.count_unitigs(thr)
    same(counted, want, "count_unitigs")
    k, thr, km, cnt, _, want = ref("tangle_k33_thr1")
    same(run_dev(m, km, cnt, k, thr), want, "tangle_k33_thr1, device")
    same(m.count_unitigs(1), counted, "count_unitigs again")
    k, thr, km, cnt, _, _ = ref("k11_sparse")
    same(m.unitigs(km, cnt, k, thr), first, "k11_sparse again on the used handle")
    same(KModel(1, 1023, NH, NB).unitigs(km, cnt, k, thr), first, "k11_sparse on a fresh handle")


def test_no_listing_and_even_session_k():
    m = KModel(1, 1023, NH, NB)
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -4
    m.count_begin(31)
    with pytest.raises(KmxError) as e:                              # a session under way has no listing yet
        m.count_unitigs(1)
    assert e.value.code == -4
    m.count_seqs([U.rand_seq(300, 5)])
    m.count_finish()
    assert len(m.count_unitigs(1)[2]) >= 1
    m.count_begin(30)
    m.count_seqs([U.rand_seq(300, 5)])
    m.count_finish()
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -1
    km, cnt = m.count_listing()
    m.build_packed(30, km, cnt)                                     # a build from other data drops the listing
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -4


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first call, for kmx_unitigs and for kmx_count_unitigs: the same call then succeeds,
    and the session's listing and model are as they were"""
    k, thr, km, cnt, _, want = ref("k9_linear2000")
    seq = U.CASES["k9_linear2000"]()[2]
    failed = {"unitigs": 0, "count_unitigs": 0}
    for which in failed:
        for nth in range(1, 16):
            m = KModel(1, 1023, NH, NB)                             # fresh: every buffer of the call is still to be allocated
            if which == "count_unitigs":
                m.count_begin(k)
                m.count_seqs(seq)
                m.count_finish()
                lk, lc = m.count_listing()
                assert np.array_equal(lk, km) and np.array_equal(lc, cnt)
                probe = U.unpack(km[::40], k)
                before = m.kmer_to_occ(probe)
                call = lambda: m.count_unitigs(thr)                 # noqa: E731
            else:
                call = lambda: m.unitigs(km, cnt, k, thr)           # noqa: E731
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                same(call(), want, f"{which}: allocation {nth} did not happen")
            except KmxError as e:
                assert e.code == -6
                failed[which] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(call(), want, f"{which} after a failed allocation ({nth})")
            if which == "count_unitigs":
                lk2, lc2 = m.count_listing()
                assert np.array_equal(lk2, km) and np.array_equal(lc2, cnt), "the listing changed"
                assert m.kmer_to_occ(probe) == before, "the model changed"
    assert failed["unitigs"] >= 8 and failed["count_unitigs"] >= 6, failed   # (11 and 9 buffers are allocated by a first call)


def parse_fasta(text):
    heads, strs = [], []
    for line in text.splitlines():
        (heads if line.startswith(">") else strs).append(line)
    return heads, strs


def fasta_heads(rec):
    return [f">u{u} n_kmers={int(r['n_kmers'])} mean_count={int(r['sum_count']) / int(r['n_kmers']):.2f} circular={int(r['circular'])}" for u, r in enumerate(rec)]


def test_facade_and_driver_fasta(tmp_path):
    """tests/facade_unitigs.cpp (count_unitigs == unitigs on the listing, inside the program) and the driver's -u switch: the
    FASTA they write, parsed back, is the Python result"""
    import os
    import subprocess
    import count_reads as CR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, thr = 21, 3
    reads = [r.encode() for r in U.CASES["reads_thr3"]()[2]]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, reads)
    m = KModel(1, 1023, NH, NB)
    m.init_reads(fa, k)
    km, cnt = m.count_listing()
    buf, off, rec = m.count_unitigs(thr)
    want = [buf[int(off[u]):int(off[u + 1])].tobytes().decode() for u in range(len(rec))]
    same((buf, off, rec), ref("reads_thr3")[5], "init_reads + count_unitigs")
    listing = str(tmp_path / "listing.txt")
    with open(listing, "w") as f:
        f.write("".join(f"{int(x)} {int(c)}\n" for x, c in zip(km, cnt)))

    def build(source, name):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(root, "include"), os.path.join(root, source),
                               "-L" + os.path.join(root, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(root, "kmcex_amd"), "-o", exe])
        return exe

    out = subprocess.check_output([build("tests/facade_unitigs.cpp", "facade_unitigs"), fa, str(k), str(thr), listing], timeout=120).decode()
    assert parse_fasta(out) == (fasta_heads(rec), want)
    work = tmp_path / "work"
    work.mkdir()
    subprocess.check_call([build("examples/kmcex_main.cpp", "kmcEx"), "-g", f"-u{thr}", f"-k{k}", "-nh3", "-nb2", fa, "db", str(work)], timeout=120)
    assert parse_fasta((work / "db" / "unitigs.fa").read_text()) == (fasta_heads(rec), want)
