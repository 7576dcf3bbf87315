"""kmx_unitig_map_* on the MI355X: segments, seg_offsets, records and hits equal, byte for byte, what the plain-Python restatement
of the rule (tests/unitig_map_ref.py) gives, for the host and the device variant of begin and of map_seqs, at one- and two-word
k; a read across three blocks of the hot kernel and read boundaries around a block's edge; the capacities; a counted session
(consequence (b)) and its cleaned graph (consequence (c)); piece sizes in a child process; accumulation; refusals; crafted
offsets; the facade and the driver."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import unitig_map_ref as R
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import SEQ_MAP_DTYPE, SEQ_SEGMENT_DTYPE, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ("segments", "seg_offsets", "records", "hits")


@functools.lru_cache(maxsize=None)
def ref(name):
    """a case of R.MAP_CASES (or one of the two below) and the restatement's flat result, computed once"""
    k, km, cnt, thr, strs, reads = (LOCAL[name] if name in LOCAL else R.MAP_CASES[name])()
    return k, km, cnt, thr, strs, reads, R.flat(*R.map_reads(km, k, strs, reads))


def long_read_case():
    """k = 31 over a random genome of 9 000 bases: one unitig.  The genome and its reverse complement as reads (one segment across
    three blocks of 4 096 windows each), then reads packed so that boundaries fall at windows 4 095 / 4 096 / 4 097 of a block
    and inside a lane's run of 16, with reads of k - 1, k, k + 1 and 0 bases among them"""
    k = 31
    g = U.rand_seq(9000, 95)
    km, cnt = U.listing_of(U.count_kmers([g], k))
    strs, _ = U.unitigs(km, cnt, k, 1)
    pad = (-18000) % 4096                                       # bring the next read to the start of a block
    reads = [g, U.rc(g), g[:pad], g[10:10 + 4095], g[5:6], g[7:8], g[:k - 1], g[:k], g[:k + 1], "", g[100:125], g[40:240].lower(),
             g[:4000] + "N" + g[4001:8200]]
    return k, km, cnt, 1, strs, reads


def piece_case():
    k, km, cnt, thr, strs, reads = R.case("k31_tangle")
    return k, km, cnt, thr, strs, reads[:10]


LOCAL = {"long_read": long_read_case, "piece_small": piece_case}


def same(got, want, what=""):
    for a, b, part in zip(got, want, PARTS):
        if a is None:
            continue
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"


def dev_set(strs):
    import torch
    buf, off = R.join(strs)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()


def begin(m, how, km, k, strs):
    import torch
    packed = U.pack(km, k)
    if how == "host":
        m.unitig_map_begin(packed, k, *R.join(strs))
    else:
        d_km = torch.from_numpy(np.ascontiguousarray(packed).view(np.int64).reshape(-1)).cuda()
        m.unitig_map_begin_dev(d_km, k, *dev_set(strs))


def run_host(m, reads, n_units, capacity=None):
    hits = np.zeros(n_units, dtype=np.uint64)
    segs, so, rec = m.seq_to_unitigs_flat(*R.join(reads), capacity=capacity, hits=hits)
    return segs, so, rec, hits


def run_dev(m, reads, n_units):
    import torch
    buf, off = R.join(reads)
    n_seqs = len(reads)
    d_seq, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    cap = max(len(buf), 1)
    d_segs = torch.zeros((cap, 24), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((n_seqs, 64), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(max(n_units, 1), dtype=torch.int64, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_seq, d_off, d_segs, None, d_rec, d_hits)
    torch.cuda.synchronize()
    return (d_segs.cpu().numpy()[:ns].reshape(-1).view(SEQ_SEGMENT_DTYPE), d_so.cpu().numpy().view(np.uint64), d_rec.cpu().numpy().reshape(-1).view(SEQ_MAP_DTYPE),
            d_hits.cpu().numpy().view(np.uint64)[:n_units])


def all_four(m, name):
    k, km, cnt, thr, strs, reads, want = ref(name)
    for how in ("host", "dev"):                                 # the second begin ends the first session
        begin(m, how, km, k, strs)
        same(run_host(m, reads, len(strs)), want, f"{name}: begin {how}, host")
        same(run_dev(m, reads, len(strs)), want, f"{name}: begin {how}, device")
    m.unitig_map_end()
    return want


@pytest.mark.parametrize("name", sorted(R.MAP_CASES))
def test_equals_the_restatement(name):
    """k = 5, 21, 31 and the two-word 33 and 63; hairpins and self-loops (the tangles); reads twice round a circular unitig;
    N in the first, middle and last window; lowercase; an IUPAC byte; reads of k - 1, k, k + 1 and 0 bases"""
    want = all_four(KModel(1, 1023, NH, NB), name)
    assert len(want[0]) > 0


def test_one_segment_across_three_blocks_and_boundaries_at_a_block_edge():
    k, km, cnt, thr, strs, reads, want = ref("long_read")
    segs, so, rec, hits = want
    assert len(strs) == 1 and rec["n_segments"][0] == 1 == rec["n_segments"][1] and segs["n_windows"][0] == 9000 - k + 1 > 2 * 4096
    assert {int(segs["o"][0]), int(segs["o"][1])} == {0, 1} and segs["off"][0] == 0 == segs["off"][1]
    off = np.cumsum([len(r) for r in reads])
    assert {4095, 0, 1} <= {int(x) % 4096 for x in off} and any(0 < int(x) % 16 < 15 for x in off)      # windows 4 095, 4 096 and 4 097 of a block
    all_four(KModel(1, 1023, NH, NB), "long_read")


def raw_dev(m, reads, n_units, capacity, give_segs=True, give_rec=True, give_hits=True, offsets=None):
    """one kmx_unitig_map_seqs_dev call on buffers longer than it is told, filled with guard bytes
    -> (rc, n_segs, segs bytes, seg_offsets, rec bytes, hits)"""
    import torch
    buf, off = R.join(reads)
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.uint64)
    n_seqs = len(off) - 1
    d_seq, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    segs = torch.full(((capacity + 4) * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    so = torch.full((n_seqs + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    rec = torch.full(((n_seqs + 2) * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    hits = torch.full((n_units + 8,), 0, dtype=torch.int64, device="cuda")
    hits[n_units:] = -7
    ns = C.c_uint64(0)
    rc = m.L.kmx_unitig_map_seqs_dev(m.h, d_seq.data_ptr(), d_off.data_ptr(), n_seqs, len(buf), segs.data_ptr() if give_segs else None, capacity, C.byref(ns), so.data_ptr(),
                                     rec.data_ptr() if give_rec else None, hits.data_ptr() if give_hits else None)
    torch.cuda.synchronize()
    return rc, ns.value, segs.cpu().numpy(), so.cpu().numpy(), rec.cpu().numpy(), hits.cpu().numpy()


def test_capacities_sizing_and_guards():
    """k = 5 on the complete listing: every window is its own unitig, so n_segs is the number of mapped windows.  The sizing call;
    capacity exactly n_segs; one short is KMX_E_RANGE with the number needed, seg_offsets, records and hits complete and nothing
    written at or behind segs[capacity]; the session survives it and succeeds with the capacity reported; rec = NULL and
    hits = NULL are accepted; the host variant reports the same"""
    k, km, cnt, thr, strs, reads, want = ref("k5_complete")
    wseg, wso, wrec, whits = want
    n, nr, nu = len(wseg), len(reads), len(strs)
    assert n == int(wrec["n_mapped"].sum()) and all(len(s) == k for s in strs)
    m = KModel(1, 1023, NH, NB)
    begin(m, "dev", km, k, strs)

    def complete(so, rec, hits):
        return (so[:nr + 1].tobytes() == wso.tobytes() and np.all(so[nr + 1:] == -6) and rec[:nr * 64].tobytes() == wrec.tobytes() and np.all(rec[nr * 64:] == 0xA5) and
                hits[:nu].tobytes() == whits.tobytes() and np.all(hits[nu:] == -7))

    rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, 0, give_segs=False)
    assert (rc, ns) == (0, n) and np.all(segs == 0xA5) and complete(so, rec, hits)
    rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, n - 1)
    assert (rc, ns) == (-5, n) and np.all(segs[(n - 1) * 24:] == 0xA5) and complete(so, rec, hits)
    rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, ns)
    assert (rc, ns) == (0, n) and segs[:n * 24].tobytes() == wseg.tobytes() and np.all(segs[n * 24:] == 0xA5) and complete(so, rec, hits)
    rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, n, give_rec=False, give_hits=False)
    assert (rc, ns) == (0, n) and segs[:n * 24].tobytes() == wseg.tobytes() and np.all(rec == 0xA5) and not hits[:nu].any()
    with pytest.raises(KmxError) as e:
        run_host(m, reads, nu, capacity=n - 1)
    assert e.value.code == -5
    same(run_host(m, reads, nu, capacity=n), want, "host, exact capacity")
    segs, so, rec = m.seq_to_unitigs_flat(*R.join(reads), records=False)
    assert rec is None and segs.tobytes() == wseg.tobytes() and so.tobytes() == wso.tobytes()
    ns, d_so = m.seq_to_unitigs_dev(*dev_set(reads))               # the sizing call through the wrapper
    assert ns == n and d_so.cpu().numpy().view(np.uint64).tobytes() == wso.tobytes()
    m.unitig_map_end()


def test_hits_accumulate_and_empty_batches():
    k, km, cnt, thr, strs, reads, want = ref("k21_cycle_and_tip")
    m = KModel(1, 1023, NH, NB)
    begin(m, "host", km, k, strs)
    hits = np.zeros(len(strs), dtype=np.uint64)
    for _ in range(2):
        m.seq_to_unitigs_flat(*R.join(reads), hits=hits)
    assert np.array_equal(hits, 2 * want[3])
    import torch
    d_hits = torch.zeros(len(strs), dtype=torch.int64, device="cuda")
    for _ in range(2):
        m.seq_to_unitigs_dev(*dev_set(reads), None, None, None, d_hits)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint64), 2 * want[3])
    ns = C.c_uint64(9)                                            # n_seqs == 0: KMX_OK, nothing written
    assert m.L.kmx_unitig_map_seqs(m.h, None, None, 0, None, 0, C.byref(ns), None, None, None) == 0 and ns.value == 0
    segs, so, rec = m.seq_to_unitigs(["", "", ""])              # reads without bases
    assert len(segs) == 0 and so.tolist() == [0, 0, 0, 0] and not rec.view(np.uint64).any()
    same(run_dev(m, ["", "", ""], len(strs)), R.flat(*R.map_reads(km, k, strs, ["", "", ""])), "empty reads, device")
    m.unitig_map_end()


@functools.lru_cache(maxsize=None)
def counted():
    return U.noisy_reads(U.rand_seq(2000, 70), 400, 100, 0.01, 71)


def test_counted_session_maps_every_counted_window():
    """consequence (b) on the device: reads at 20x with 1 % errors counted through kmx_count_*, mapped onto count_unitigs(1) of
    the listing read where it lies: n_mapped is the counted windows of every read and hits[u] == rec[u].sum_count"""
    k, reads = 21, counted()
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    m.count_finish()
    lk_km, lk_cnt = m.count_listing()
    assert int(lk_cnt.max()) < 1023
    ubuf, uoff, urec = m.count_unitigs(1)
    strs = [s.decode() for s in (ubuf[int(uoff[i]):int(uoff[i + 1])].tobytes() for i in range(len(urec)))]
    want = R.flat(*R.map_reads(U.unpack(lk_km, k), k, strs, reads))
    m.count_unitig_map_begin(ubuf, uoff)
    got = run_host(m, reads, len(strs))
    same(got, want, "counted, host")
    same(run_dev(m, reads, len(strs)), want, "counted, device")
    assert np.array_equal(got[2]["n_mapped"], got[2]["n_windows"]) and np.all(got[2]["n_windows"] == 100 - k + 1)
    assert np.array_equal(got[3], urec["sum_count"])
    import torch
    m.count_unitig_map_begin_dev(torch.from_numpy(ubuf.copy()).cuda(), torch.from_numpy(uoff.view(np.int64).copy()).cuda())
    same(run_dev(m, reads, len(strs)), want, "counted, begin_dev")
    lk2, lc2 = m.count_listing()
    assert np.array_equal(lk2, lk_km) and np.array_equal(lc2, lk_cnt), "the listing changed"
    m.count_begin(k)                                              # drops the listing: the session ends with it
    with pytest.raises(KmxError) as e:
        m.seq_to_unitigs(reads[:2])
    assert e.value.code == -4
    with pytest.raises(KmxError) as e:
        m.count_unitig_map_begin(ubuf, uoff)
    assert e.value.code == -4


def test_cleaned_graph_unmaps_what_was_removed():
    """consequence (c) on the device: on count_unitig_graph_clean(thr = 2) a window is unmapped exactly when its entry has
    removed[i] != 0 or a count below thr"""
    k, thr, reads = 21, 2, counted()
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    m.count_finish()
    lk_km, lk_cnt = m.count_listing()
    ubuf, uoff, urec, _, _, removed, _ = m.count_unitig_graph_clean(thr)
    strs = [ubuf[int(uoff[i]):int(uoff[i + 1])].tobytes().decode() for i in range(len(urec))]
    km = U.unpack(lk_km, k)
    want = R.flat(*R.map_reads(km, k, strs, reads))
    m.count_unitig_map_begin(ubuf, uoff)
    got = run_host(m, reads, len(strs))
    same(got, want, "cleaned, host")
    same(run_dev(m, reads, len(strs)), want, "cleaned, device")
    m.unitig_map_end()
    idx = {x: i for i, x in enumerate(km)}
    segs, so, rec, hits = got
    is_mapped = np.zeros(sum(len(r) for r in reads), dtype=bool)
    for s in segs:
        is_mapped[int(s["pos"]):int(s["pos"]) + int(s["n_windows"])] = True
    base, seen = 0, [0, 0]
    for read in reads:
        for w in range(len(read) - k + 1):
            i = idx[U.canon(read[w:w + k])]
            gone = bool(removed[i] != 0 or lk_cnt[i] < thr)
            assert bool(is_mapped[base + w]) != gone
            seen[gone] += 1
        assert not is_mapped[base + len(read) - k + 1:base + len(read)].any()
        base += len(read)
    assert min(seen) > 100 and removed.any()


CHILD = """
import hashlib, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_unitig_map as T
from kmcex_amd import KModel
name = sys.argv[1]
k, km, cnt, thr, strs, reads, want = T.ref(name)
m = KModel(1, 1023, T.NH, T.NB)
T.begin(m, "host", km, k, strs)
for got in (T.run_host(m, reads, len(strs)), T.run_dev(m, reads, len(strs))):
    print(hashlib.sha256(b"|".join(a.tobytes() for a in got)).hexdigest())
"""


@pytest.mark.parametrize("piece,name", [(1, "piece_small"), (1000, "long_read"), (4097, "long_read")])
def test_piece_sizes_change_nothing(piece, name, tmp_path):
    """KMX_MAP_PIECE shrinks the host variant's pieces and the device chunks to 1, 1 000 and 4 097 windows (a fresh process: the
    hooks' switch is read once): host and device results are those of the default size"""
    want = ref(name)[6]
    digest = hashlib.sha256(b"|".join(a.tobytes() for a in want)).hexdigest()
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT))
    env = dict(os.environ, KMX_TEST_HOOKS="1", KMX_MAP_PIECE=str(piece))
    out = subprocess.check_output([sys.executable, str(script), name], env=env, timeout=300).decode().split()
    assert out == [digest, digest]


def test_allocation_failure_leaves_handle_and_session_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first begin and of a first map call in turn: a begin that failed is simply repeated, and
    a map call that failed leaves the session open, so the same call then succeeds with the right bytes"""
    k, km, cnt, thr, strs, reads, want = ref("k21_cycle_and_tip")
    failed = [0, 0]
    for nth in range(1, 13):
        for variant, run in (("host", run_host), ("dev", run_dev)):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                begin(m, variant, km, k, strs)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[0] += 1
                monkeypatch.delenv("KMX_FAIL_ALLOC")
                begin(m, variant, km, k, strs)
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run(m, reads, len(strs))
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[1] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run(m, reads, len(strs)), want, f"after allocation {nth} failed, {variant}")
            m.unitig_map_end()
    assert failed[0] >= 6 and failed[1] >= 6, failed


def test_refusals():
    """even k; a unitig set with a k-mer that is not listed, with one unitig twice, with a lowercase byte, with a unitig shorter
    than k; map_seqs before begin and after end; count_unitig_map_begin without a listing; decreasing offsets in the host form;
    the handle then maps as if nothing had happened"""
    k, km, cnt, thr, strs, reads, want = ref("k21_cycle_and_tip")
    m = KModel(1, 1023, NH, NB)
    with pytest.raises(KmxError) as e:
        m.seq_to_unitigs(reads)
    assert e.value.code == -4
    with pytest.raises(KmxError) as e:
        m.unitig_map_end()
    assert e.value.code == -4
    for call in (m.count_unitig_map_begin, lambda b, o: m.count_unitig_map_begin_dev(*dev_set(strs))):
        with pytest.raises(KmxError) as e:
            call(*R.join(strs))
        assert e.value.code == -4
    for kk in (6, 20, 32, 64):
        with pytest.raises(KmxError) as e:
            m.unitig_map_begin(np.zeros(2 * ((kk + 31) // 32), np.uint64), kk, *R.join(["A" * kk]))
        assert e.value.code == -1
    foreign = U.rand_seq(k + 5, 97)
    for bad in (strs + [foreign], strs + [strs[0]], [strs[0].lower()] + strs[1:], [strs[0][:-1] + "N"] + strs[1:], strs + [strs[0][:k - 1]], strs + [U.rc(strs[0])]):
        for how in ("host", "dev"):
            with pytest.raises(KmxError) as e:
                begin(m, how, km, k, bad)
            assert e.value.code == -1, (how, bad[-1])
            with pytest.raises(KmxError) as e:                       # a begin that fails leaves no session
                m.seq_to_unitigs(reads)
            assert e.value.code == -4
    swapped = list(km)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    with pytest.raises(KmxError) as e:
        begin(m, "host", swapped, k, strs)
    assert e.value.code == -1
    begin(m, "host", km, k, strs)
    buf, off = R.join(reads)
    bad_off = off.copy()
    bad_off[1], bad_off[2] = off[2], off[1]
    ns = C.c_uint64(0)
    so = np.zeros(len(off), dtype=np.uint64)
    assert m.L.kmx_unitig_map_seqs(m.h, buf.ctypes.data, bad_off.ctypes.data, len(off) - 1, None, 0, C.byref(ns), so.ctypes.data, None, None) == -1
    same(run_host(m, reads, len(strs)), want, "after the refusals")
    m.unitig_map_end()
    with pytest.raises(KmxError) as e:
        m.seq_to_unitigs(reads)
    assert e.value.code == -4


def test_crafted_offsets_stay_inside_the_buffers():
    """the _dev form clamps the offsets where it reads them, like kmx_query_seqs_dev: decreasing, far too large and all-ones
    offsets give wrong segments and leave the guard bytes around segs, seg_offsets, rec and hits intact"""
    k, km, cnt, thr, strs, reads, want = ref("k31_tangle")
    m = KModel(1, 1023, NH, NB)
    begin(m, "dev", km, k, strs)
    buf, off = R.join(reads)
    n, nr, nu = len(buf), len(reads), len(strs)
    big = np.uint64(2 ** 64 - 1)
    crafted = [off[::-1].copy(), np.where(np.arange(nr + 1) % 2 == 1, big, off), off + np.uint64(n), np.full(nr + 1, big), np.concatenate([[np.uint64(7)], off[1:]])]
    cap = n
    for bad in crafted:
        rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, cap, offsets=bad)
        assert rc in (0, -5) and ns <= n
        assert np.all(segs[cap * 24:] == 0xA5) and np.all(so[nr + 1:] == -6) and np.all(rec[nr * 64:] == 0xA5) and np.all(hits[nu:] == -7)
    rc, ns, segs, so, rec, hits = raw_dev(m, reads, nu, cap)
    assert rc == 0 and segs[:ns * 24].tobytes() == want[0].tobytes() and so[:nr + 1].tobytes() == want[1].tobytes()
    m.unitig_map_end()


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_map.cpp and the driver's -u1 -M write the restatement's segments and hits for the reads of the input;
    without -M the driver writes neither file"""
    import count_reads as CR
    k, thr = 21, 1
    reads = counted()[:150]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in reads])
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, _ = U.unitigs(km, cnt, k, thr)
    segs, so, recs, hits = R.map_reads(km, k, strs, reads)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    paths = "".join(f"{i}\t{s['pos'] - starts[i]}\t{s['n_windows']}\tu{s['o'] >> 1}\t{'-' if s['o'] & 1 else '+'}\t{s['off']}\n"
                    for i in range(len(reads)) for s in segs[so[i]:so[i + 1]])
    hits_tsv = "".join(f"u{u}\t{h}\n" for u, h in enumerate(hits))

    def build(source, name):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    lines = str(tmp_path / "reads.txt")
    with open(lines, "w") as f:
        f.write("".join(r + "\n" for r in reads))
    out = subprocess.check_output([build("tests/facade_unitig_map.cpp", "facade_unitig_map"), fa, str(k), str(thr), lines], timeout=120).decode()
    assert out == paths + "#\n" + hits_tsv
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    plain, with_map = tmp_path / "plain", tmp_path / "mapped"
    plain.mkdir()
    with_map.mkdir()
    subprocess.check_call([exe, "-g", f"-u{thr}", f"-k{k}", "-nh3", "-nb2", fa, "db", str(plain)], timeout=120)
    log = subprocess.check_output([exe, "-g", f"-u{thr}", "-M", f"-k{k}", "-nh3", "-nb2", fa, "db", str(with_map)], timeout=120).decode()
    assert (with_map / "db" / "reads.paths.tsv").read_text() == paths and (with_map / "db" / "unitigs.hits.tsv").read_text() == hits_tsv
    assert f"{len(reads)} reads, {len(segs)} segments" in log
    assert (plain / "db" / "unitigs.fa").read_text() == (with_map / "db" / "unitigs.fa").read_text()
    assert not (plain / "db" / "reads.paths.tsv").exists() and not (plain / "db" / "unitigs.hits.tsv").exists()
