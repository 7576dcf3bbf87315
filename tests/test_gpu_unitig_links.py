"""kmx_unitig_graph*, kmx_count_unitig_graph* on the MI355X: link_offsets and links equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitig_links_ref.py) gives, and strings, offsets and records are the twin's, for the host and
the device variant, on every case of U.CASES; on a counted session; on listings whose sizes and numbers of unitig ends lie
around the launch geometry of the links kernel; the capacities, one short each; empty outputs; refusals; the rounds; the GFA of
the facade and the driver."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import unitig_links_ref as UL
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def ref(name):
    """(k, thr, packed k-mers, counts, strs, recs, link_offsets, links) of the restatement, computed once"""
    k, thr, km, cnt, strs, recs, off, lk = UL.case_links(name)
    return k, thr, U.pack(km, k), np.asarray(cnt, dtype=np.uint32), strs, recs, off, lk


def listed(km_s, cnt, k, thr=1):
    """(packed k-mers, counts, recs, link_offsets, links) of the restatement for a listing that is no case"""
    strs, recs = U.unitigs(km_s, cnt, k, thr)
    off, lk = UL.flat_links(UL.links(km_s, cnt, k, thr, strs))
    return U.pack(km_s, k), np.asarray(cnt, dtype=np.uint32), recs, off, lk


def same_links(got, off, lk, what=""):
    assert np.asarray(got[3]).dtype == np.uint64 and np.asarray(got[4]).dtype == np.uint32
    assert np.asarray(got[3]).tobytes() == off.tobytes(), f"{what}: link_offsets differ"
    assert np.asarray(got[4]).tobytes() == lk.tobytes(), f"{what}: links differ"


def same_unitigs(got, twin, what=""):
    for a, b, part in zip(got[:3], twin, ("strings", "offsets", "records")):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"{what}: {part} are not the twin's"


def from_torch(got):
    buf, off, rec, loff, lk = got
    return (buf.cpu().numpy(), off.cpu().numpy().view(np.uint64), rec.cpu().numpy().reshape(-1).view(UNITIG_DTYPE),
            loff.cpu().numpy().view(np.uint64), lk.cpu().numpy().view(np.uint32))


def to_dev(km, cnt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(km).view(np.int64).reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(cnt).view(np.int32)).cuda()


def run_dev(m, km, cnt, k, thr):
    d_km, d_cnt = to_dev(km, cnt)
    return from_torch(m.unitig_graph_dev(d_km, d_cnt, k, thr))


def both(m, km, cnt, k, thr, off, lk, what):
    """host and device variant against the restatement's links and against the twin on the same handle -> the host result"""
    twin = m.unitigs(km, cnt, k, thr)
    got = m.unitig_graph(km, cnt, k, thr)
    same_links(got, off, lk, f"{what}, host")
    same_unitigs(got, twin, f"{what}, host")
    dev = run_dev(m, km, cnt, k, thr)
    same_links(dev, off, lk, f"{what}, device")
    same_unitigs(dev, twin, f"{what}, device")
    return got


@pytest.mark.parametrize("name", [n for n in U.CASES if not n.startswith("reads")])
def test_equals_the_restatement(name):
    """degree 4 on both sides (k5_complete, k7_complete: 8 links per node, the tight link_capacity), hairpins and self-loops,
    every cycle length from 2 to 130, two-word k up to 63, counts of 0 and 0xFFFFFFFF, thr of 0 and 0xFFFFFFFF, one bucket of
    the index; the rounds are the twin's; a second call on the same handle gives the same"""
    k, thr, km, cnt, strs, recs, off, lk = ref(name)
    m = KModel(1, 1023, NH, NB)
    m.unitigs(km, cnt, k, thr)
    rounds = m.unitigs_phases()["rounds"]
    got = both(m, km, cnt, k, thr, off, lk, name)
    assert len(got[4]) == int(got[2]["n_pred"].astype(np.int64).sum() + got[2]["n_succ"].astype(np.int64).sum())
    again = m.unitig_graph(km, cnt, k, thr)
    for a, b in zip(got, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), "the second call on the same handle differs"
    ph = m.unitig_graph_phases()
    assert ph["rounds"] == rounds == m.unitigs_phases()["rounds"]
    assert set(ph) == {"adjacency", "links", "ranking", "emit", "unitig_links", "rounds"}


@pytest.mark.parametrize("thr", [1, 3])
def test_thr_on_a_counted_session(thr):
    """reads at 20x with 1 % errors, counted through kmx_count_*: count_unitig_graph and its device variant against the
    restatement on the listing the session returns, and against count_unitigs"""
    reads = U.CASES[f"reads_thr{thr}"]()[2]
    k = 21
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    m.count_finish()
    lk_km, lk_cnt = m.count_listing()
    km_s = U.unpack(lk_km, k)
    _, _, recs, off, lk = listed(km_s, lk_cnt.tolist(), k, thr)
    twin = m.count_unitigs(thr)
    got = m.count_unitig_graph(thr)
    same_links(got, off, lk, "count_unitig_graph")
    same_unitigs(got, twin, "count_unitig_graph")
    dev = from_torch(m.count_unitig_graph_dev(thr))
    same_links(dev, off, lk, "count_unitig_graph_dev")
    same_unitigs(dev, twin, "count_unitig_graph_dev")
    assert (len(lk) > 1000) if thr == 1 else (len(recs) < 10)
    lk2, lc2 = m.count_listing()
    assert np.array_equal(lk2, lk_km) and np.array_equal(lc2, lk_cnt), "the listing changed"


def ends_listing(n_ends, seed, k=31):
    """a listing with exactly n_ends entries that are the head or the tail of their unitig: one Y (a stem that forks into two
    branch stubs: three unitigs, 6 ends), disjoint random paths of 3 nodes (2 ends each), and a single node where n_ends is odd
    (head and tail at once: 1 end)"""
    r = random.Random(seed)

    def rs(n):
        return "".join(r.choice("ACGT") for _ in range(n))

    stem = rs(k + 2)
    seqs = [stem + "A" + rs(k), stem + "C" + rs(k)]
    rest = n_ends - 6
    seqs += [rs(k + 2) for _ in range(rest // 2)]
    if rest % 2:
        seqs.append(rs(k))
    km_s, cnt = U.listing_of(U.count_kmers(seqs, k))
    return km_s, cnt


ENDS = [7, 8, 9, 13, 14, 15, 16, 17, 31, 32, 33, 61, 62, 63, 64, 65, 66, 255, 256, 257, 509, 510, 511, 512, 513, 514]


@pytest.mark.parametrize("n_ends", ENDS)
def test_unitig_ends_around_the_launch_geometry(n_ends):
    """k_uni_links gives every unitig (and one group behind the last, for the last offset) a group of 8 lanes: 4 for its tail
    entry, 4 for its head entry, so a wave of 64 lanes holds 8 groups and a block of 256 threads holds 32.  U + 1 groups: the
    listings have U = 7, 8 and 9 (a wave), 31, 32 and 33 (a block), 255 to 257 (8 blocks), with and without a single-node
    unitig (one entry that is both ends), and their end entries lie around 8, 16, 32, 64, 256 and 512 as well"""
    k = 31
    km_s, cnt = ends_listing(n_ends, 9000 + n_ends, k)
    km, cnt, recs, off, lk = listed(km_s, cnt, k)
    assert sum(1 if r["n_kmers"] == 1 else 2 for r in recs) == n_ends and len(recs) == (n_ends + 1) // 2
    assert len(lk) == 4 and max(r["n_succ"] + r["n_pred"] for r in recs) == 2   # the Y's edges and their mirrors
    both(KModel(1, 1023, NH, NB), km, cnt, k, 1, off, lk, f"{n_ends} ends")


def test_listing_sizes_at_the_launch_edges():
    """n + 1 threads in blocks of 256 (the link counts at the heads and the two lists of end entries), U + 1 groups of 8 lanes
    (the links kernel) for whatever U the prefix has: the first n entries of a dense listing, which are a listing"""
    k, thr, km, cnt, _, _, _, _ = ref("k7_half_thr1")
    km_s = U.unpack(km, k)
    m = KModel(1, 1023, NH, NB)
    for n in (1, 2, 7, 8, 30, 31, 32, 33, 63, 64, 254, 255, 256, 257, 511, 512, 513):
        _, _, _, off, lk = listed(km_s[:n], cnt[:n].tolist(), k, thr)
        both(m, km[:n], cnt[:n], k, thr, off, lk, f"n = {n}")


def raw(m, fn, args, seq_cap, rec_cap, link_cap, give_seq=True, give_loffs=True, give_links=True):
    """one call on device buffers that are longer than the capacities it is told, filled with sentinels
    -> (rc, (n_unitigs, n_bases, n_links), seq, offs, rec, loffs, links)"""
    import torch
    seq = torch.full((seq_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = torch.full((rec_cap + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    rec = torch.full(((rec_cap + 2) * 40,), 0xA5, dtype=torch.uint8, device="cuda")
    loffs = torch.full((2 * rec_cap + 1 + 8,), -7, dtype=torch.int64, device="cuda")
    links = torch.full((link_cap + 16,), -8, dtype=torch.int32, device="cuda")
    nu, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = fn(m.h, *args, seq.data_ptr() if give_seq else None, seq_cap, offs.data_ptr(), rec.data_ptr(), rec_cap,
            loffs.data_ptr() if give_loffs else None, links.data_ptr() if give_links else None, link_cap, C.byref(nu), C.byref(nb), C.byref(nl))
    torch.cuda.synchronize()
    return rc, (nu.value, nb.value, nl.value), seq.cpu().numpy(), offs.cpu().numpy(), rec.cpu().numpy(), loffs.cpu().numpy(), links.cpu().numpy()


def untouched(seq, offs, rec, loffs, links):
    return np.all(seq == 0xA5) and np.all(offs == -6) and np.all(rec == 0xA5) and np.all(loffs == -7) and np.all(links == -8)


@pytest.mark.parametrize("name", ["k7_linear300", "k5_complete"])
def test_capacities_sizing_and_sentinels(name):
    """the sizing call returns the three counts and writes nothing; exact capacities succeed and nothing lies behind them; each
    capacity one short is KMX_E_RANGE with the three counts and every buffer as it was.  k5_complete needs link_capacity =
    8 * nodes in full; the host variant reports the same; a missing link buffer is KMX_E_ARG"""
    k, thr, km, cnt, strs, recs, off, lk = ref(name)
    wbuf, woff, wrec = U.flat(strs, recs)
    m = KModel(1, 1023, NH, NB)
    d_km, d_cnt = to_dev(km, cnt)
    args = (k, d_km.data_ptr(), d_cnt.data_ptr(), len(cnt), thr)
    nu, nb, nl = len(wrec), len(wbuf), len(lk)
    assert nl >= 2 and (name != "k5_complete" or nl == 8 * len(cnt))
    fn = m.L.kmx_unitig_graph_dev
    rc, counts, *bufs = raw(m, fn, args, nb, nu, nl, give_seq=False)
    assert (rc, counts) == (0, (nu, nb, nl)) and untouched(*bufs)
    rc, counts, seq, offs, rec, loffs, links = raw(m, fn, args, nb, nu, nl)
    assert (rc, counts) == (0, (nu, nb, nl))
    assert seq[:nb].tobytes() == wbuf.tobytes() and np.all(seq[nb:] == 0xA5)
    assert np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(offs[nu + 1:] == -6)
    assert rec[:nu * 40].tobytes() == wrec.tobytes() and np.all(rec[nu * 40:] == 0xA5)
    assert loffs[:2 * nu + 1].tobytes() == off.tobytes() and np.all(loffs[2 * nu + 1:] == -7)
    assert links[:nl].tobytes() == lk.tobytes() and np.all(links[nl:] == -8)
    for sc, rcap, lcap in ((nb - 1, nu, nl), (nb, nu - 1, nl), (nb, nu, nl - 1)):
        rc, counts, *bufs = raw(m, fn, args, sc, rcap, lcap)
        assert (rc, counts) == (-5, (nu, nb, nl)), (sc, rcap, lcap)
        assert untouched(*bufs), (sc, rcap, lcap)
    for miss in ("give_loffs", "give_links"):
        rc, counts, *bufs = raw(m, fn, args, nb, nu, nl, **{miss: False})
        assert rc == -1 and untouched(*bufs), miss
    # the host variant reports the same
    obuf = np.full(nb + 8, 0xA5, dtype=np.uint8)
    ooff = np.full(nu + 1, 6, dtype=np.uint64)
    oloff = np.full(2 * nu + 1, 7, dtype=np.uint64)
    olk = np.full(nl + 8, 8, dtype=np.uint32)
    cu, cb, cl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    host = (m.h, k, km.ctypes.data, cnt.ctypes.data, len(cnt), thr, obuf.ctypes.data)
    tail = (C.byref(cu), C.byref(cb), C.byref(cl))
    for sc, rcap, lcap in ((nb - 1, nu, nl), (nb, nu - 1, nl), (nb, nu, nl - 1)):
        rc = m.L.kmx_unitig_graph(*host, sc, ooff.ctypes.data, None, rcap, oloff.ctypes.data, olk.ctypes.data, lcap, *tail)
        assert (rc, cu.value, cb.value, cl.value) == (-5, nu, nb, nl)
        assert np.all(obuf == 0xA5) and np.all(ooff == 6) and np.all(oloff == 7) and np.all(olk == 8)
    rc = m.L.kmx_unitig_graph(*host, nb, ooff.ctypes.data, None, nu, oloff.ctypes.data, olk.ctypes.data, nl, *tail)
    assert rc == 0 and oloff.tobytes() == off.tobytes() and olk[:nl].tobytes() == lk.tobytes() and np.all(olk[nl:] == 8) and np.all(obuf[nb:] == 0xA5)
    assert m.L.kmx_unitig_graph(*host, nb, ooff.ctypes.data, None, nu, None, olk.ctypes.data, nl, *tail) == -1
    assert m.L.kmx_unitig_graph(*host, nb, ooff.ctypes.data, None, nu, oloff.ctypes.data, None, nl, *tail) == -1


def test_empty_and_thr_above_every_count():
    k, _, km, cnt, _, _, _, _ = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    for kk, cc, thr in ((km[:0], cnt[:0], 1), (km, cnt, int(cnt.max()) + 1)):
        buf, off, rec, loff, lk = m.unitig_graph(kk, cc, k, thr)
        assert len(buf) == 0 and len(rec) == 0 and off.tolist() == [0] and loff.tolist() == [0] and len(lk) == 0
        d_km, d_cnt = to_dev(kk, cc)
        rc, counts, seq, offs, rec, loffs, links = raw(m, m.L.kmx_unitig_graph_dev, (k, d_km.data_ptr() or None, d_cnt.data_ptr() or None, len(cc), thr), 4, 4, 4)
        assert (rc, counts) == (0, (0, 0, 0)) and offs[0] == 0 and loffs[0] == 0
        assert np.all(offs[1:] == -6) and np.all(loffs[1:] == -7) and np.all(seq == 0xA5) and np.all(links == -8)


def test_bad_listings_and_arguments():
    """unsorted, duplicated and non-canonical listings and an even k are KMX_E_ARG like the twin's; the handle answers the next
    call"""
    k, thr, km, cnt, _, _, off, lk = ref("k7_linear300")
    km_s = U.unpack(km, k)
    m = KModel(1, 1023, NH, NB)
    swapped = km.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    dup = km.copy()
    dup[20] = dup[19]
    noncanon = km.copy()
    i = next(j for j, s in enumerate(km_s) if (j == 0 or U.rc(s) > km_s[j - 1]) and (j + 1 == len(km_s) or U.rc(s) < km_s[j + 1]))
    noncanon[i] = U.pack([U.rc(km_s[i])], k)[0]                    # still ascending, no longer canonical
    assert np.all(np.diff(noncanon.astype(np.int64)) > 0)
    for bad in (swapped, dup, noncanon):
        for call in (m.unitig_graph, lambda *a: run_dev(m, *a)):
            with pytest.raises(KmxError) as e:
                call(bad, cnt, k, 1)
            assert e.value.code == -1
    for kk in (4, 6, 30, 32, 64):                                   # even
        with pytest.raises(KmxError) as e:
            m.unitig_graph(np.zeros(2 * ((kk + 31) // 32), np.uint64), np.ones(2, np.uint32), kk, 1)
        assert e.value.code == -1
    with pytest.raises(KmxError) as e:                              # no listing
        m.count_unitig_graph(1)
    assert e.value.code == -4
    both(m, km, cnt, k, thr, off, lk, "after the refusals")


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first kmx_unitig_graph call with exact room (no sizing call in front, so the
    countdown reaches the staged output): the uploaded listing (2), the work arrays and the scan's scratch (9), the staged
    strings, offsets, link_offsets and links (4).  The three counts are as documented, and the same call then succeeds on the
    same handle"""
    k, thr, km, cnt, strs, recs, off, lk = ref("k9_linear2000")
    wbuf, woff, _ = U.flat(strs, recs)
    nu, nb, nl = len(strs), len(wbuf), len(lk)
    failed = 0
    for nth in range(1, 20):
        m = KModel(1, 1023, NH, NB)                             # fresh: every buffer of the call is still to be allocated
        obuf, ooff = np.zeros(nb, np.uint8), np.zeros(nu + 1, np.uint64)
        oloff, olk = np.zeros(2 * nu + 1, np.uint64), np.zeros(nl, np.uint32)
        cu, cb, cl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

        def call():
            return m.L.kmx_unitig_graph(m.h, k, km.ctypes.data, cnt.ctypes.data, len(cnt), thr, obuf.ctypes.data, nb, ooff.ctypes.data, None, nu,
                                        oloff.ctypes.data, olk.ctypes.data, nl, C.byref(cu), C.byref(cb), C.byref(cl))

        monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
        rc = call()
        monkeypatch.delenv("KMX_FAIL_ALLOC")
        assert rc in (0, -6), (nth, rc)
        failed += rc == -6
        assert call() == 0 and (cu.value, cb.value, cl.value) == (nu, nb, nl), nth
        assert obuf.tobytes() == wbuf.tobytes() and ooff.tobytes() == woff.tobytes(), nth
        assert oloff.tobytes() == off.tobytes() and olk.tobytes() == lk.tobytes(), nth
    assert failed >= 15, failed


def test_facade_and_driver_gfa(tmp_path):
    """tests/facade_unitig_graph.cpp (count_unitig_graph == count_unitigs and == unitig_graph on the listing, inside the
    program) and the driver's -u2 -G: the GFA they write is the restatement's text, and -G leaves unitigs.fa what -u2 alone
    writes"""
    import count_reads as CR
    k, thr = 21, 2
    reads = [r.encode() for r in U.CASES["reads_thr3"]()[2]]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, reads)
    m = KModel(1, 1023, NH, NB)
    m.init_reads(fa, k)
    km, cnt = m.count_listing()
    strs, recs = U.unitigs(U.unpack(km, k), cnt.tolist(), k, thr)
    off, lk = UL.flat_links(UL.links(U.unpack(km, k), cnt.tolist(), k, thr, strs))
    got = m.count_unitig_graph(thr)
    same_links(got, off, lk, "init_reads + count_unitig_graph")
    want = UL.gfa(strs, recs, off, lk, k)
    assert want.count("\nL\t") >= 1
    listing = str(tmp_path / "listing.txt")
    with open(listing, "w") as f:
        f.write("".join(f"{int(x)} {int(c)}\n" for x, c in zip(km, cnt)))

    def build(source, name):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    out = subprocess.check_output([build("tests/facade_unitig_graph.cpp", "facade_unitig_graph"), fa, str(k), str(thr), listing], timeout=120).decode()
    assert out == want
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    plain, graph = tmp_path / "plain", tmp_path / "graph"
    plain.mkdir()
    graph.mkdir()
    subprocess.check_call([exe, "-g", f"-u{thr}", f"-k{k}", "-nh3", "-nb2", fa, "db", str(plain)], timeout=120)
    subprocess.check_call([exe, "-g", f"-u{thr}", "-G", f"-k{k}", "-nh3", "-nb2", fa, "db", str(graph)], timeout=120)
    assert (graph / "db" / "unitigs.gfa").read_text() == want
    assert (graph / "db" / "unitigs.fa").read_bytes() == (plain / "db" / "unitigs.fa").read_bytes()
    assert not (plain / "db" / "unitigs.gfa").exists()
