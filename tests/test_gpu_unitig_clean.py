"""kmx_*unitig_graph_clean* on the MI355X: strings, offsets, records, link_offsets, links, removed and every stats field
equal, byte for byte, what the plain-Python restatement of the rule (tests/unitig_clean_ref.py) gives, for the host and the
device variant, on every case of U.CASES and on the hand-built shapes of CLEAN_CASES; each subset of ops; prefixes of the
rounds; listings around the launch geometry of the two new kernels; a counted session; the capacities, one short each;
refusals; empty outputs; allocation failures; the facade and the driver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import unitig_clean_ref as CL
import unitig_links_ref as UL
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE, CleanParams, CleanStats, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ("strings", "offsets", "records", "link_offsets", "links", "removed")


@functools.lru_cache(maxsize=None)
def listing(name):
    """(k, thr, k-mers as strings, counts, packed k-mers, counts uint32) of a case of U.CASES, thr as the case has it"""
    c = U.CASES[name]()
    if len(c) == 3:
        k, thr, seqs = c
        km, cnt = U.listing_of(U.count_kmers(seqs, k))
    else:
        k, thr, km, cnt = c
    return k, thr, km, cnt, U.pack(km, k), np.asarray(cnt, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def ref(name, thr=None, ops=7, max_tip=None, max_bubble=None, max_rounds=16):
    """the restatement's result for a case of U.CASES, computed once per parameter set"""
    k, thr0, km, cnt, _, _ = listing(name)
    return CL.clean(km, cnt, k, thr0 if thr is None else thr, ops, max_tip, max_bubble, max_rounds)


def same(got, res, what=""):
    """a library result (numpy) against a result of the restatement"""
    want = CL.flat(res)
    assert np.asarray(got[1]).dtype == np.uint64 and np.asarray(got[3]).dtype == np.uint64 and np.asarray(got[4]).dtype == np.uint32
    for a, b, part in zip(got[:6], want, PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"
    assert got[6] == res["stats"], f"{what}: stats differ"


def from_torch(got):
    buf, off, rec, loff, lk, removed, st = got
    return (buf.cpu().numpy(), off.cpu().numpy().view(np.uint64), rec.cpu().numpy().reshape(-1).view(UNITIG_DTYPE),
            loff.cpu().numpy().view(np.uint64), lk.cpu().numpy().view(np.uint32), removed.cpu().numpy(), st)


def to_dev(km, cnt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(km).view(np.int64).reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(cnt).view(np.int32)).cuda()


def both(m, km, cnt, k, thr, res, what, **par):
    """host and device variant against the restatement -> the host result"""
    got = m.unitig_graph_clean(km, cnt, k, thr, **par)
    same(got, res, f"{what}, host")
    d_km, d_cnt = to_dev(km, cnt)
    keep = d_cnt.clone()
    same(from_torch(m.unitig_graph_clean_dev(d_km, d_cnt, k, thr, **par)), res, f"{what}, device")
    assert bool((d_cnt == keep).all()), f"{what}: the caller's counts were written"
    return got


@pytest.mark.parametrize("name", [n for n in U.CASES if not n.startswith("reads")])
def test_equals_the_restatement(name):
    """ops = 7, caps 2 k, max_rounds = 16 on every case; a second call on the same handle gives the same bytes; the twin
    afterwards is what it was; k7_tenth, whose thr is 0, is KMX_E_ARG"""
    k, thr, _, _, km, cnt = listing(name)
    m = KModel(1, 1023, NH, NB)
    if thr == 0:
        with pytest.raises(KmxError) as e:
            m.unitig_graph_clean(km, cnt, k, thr)
        assert e.value.code == -1
        return
    res = ref(name)
    before = m.unitig_graph(km, cnt, k, thr)
    got = both(m, km, cnt, k, thr, res, name)
    assert (res["stats"]["n_unitigs_before"], res["stats"]["n_links_before"]) == (len(before[2]), len(before[4]))
    again = m.unitig_graph_clean(km, cnt, k, thr)
    for a, b in zip(got[:6], again[:6]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), "the second call on the same handle differs"
    assert got[6] == again[6]
    ph = m.unitig_clean_phases()
    assert set(ph) == {"adjacency", "links", "ranking", "emit", "unitig_links", "clean", "rounds"} and ph["rounds"] >= 1
    after = m.unitig_graph(km, cnt, k, thr)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), "the twin changed after a cleaning call"
    if not any(res["removed"]):                                # a no-op is exact
        for a, b in zip(got[:5], before):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert (got[6]["rounds_run"], got[6]["converged"]) == (1, 1)


@pytest.mark.parametrize("name", list(CL.CLEAN_CASES))
def test_crafted_shapes(name):
    k, thr, km_s, cnt, p, res = CL.clean_case(name)
    ops, max_tip, max_bubble, max_rounds = p
    km, cnt = U.pack(km_s, k), np.asarray(cnt, dtype=np.uint32)
    got = both(KModel(1, 1023, NH, NB), km, cnt, k, thr, res, name, ops=ops, max_tip=max_tip, max_bubble=max_bubble, max_rounds=max_rounds)
    st, rec = got[6], got[2]
    if name == "y_short_branch_goes":
        assert (st["n_tips"], st["n_kmers_removed"], len(rec)) == (1, 10, 1) and int(rec["n_kmers"][0]) == 111
    if name in ("y_two_equal_short_lower_index_survives", "y_equal_length_sum_decides"):
        assert (st["n_tips"], st["n_kmers_removed"], len(rec)) == (1, 10, 1)
    if name == "tip_into_two_junctions_stays":
        assert (st["n_tips"], st["n_kmers_removed"], len(rec)) == (1, 5, 3) and 12 in rec["n_kmers"].tolist()
    if name == "tip_on_a_cycle_closes_it":
        assert len(rec) == 1 and int(rec["circular"][0]) == 1 and int(rec["n_kmers"][0]) == 40
    if name.startswith("snp_bubble"):
        assert (st["n_bubbles"], st["n_kmers_removed"], len(rec)) == (1, 31, 1)
    if name == "hairpin_and_self_loop_arms_stay":
        assert st["n_bubbles"] == 0 and sorted((int(r["n_pred"]), int(r["n_succ"])) for r in rec).count((1, 1)) == 2
    if name == "tip_of_exactly_max_tip":
        assert (st["n_tips"], st["n_kmers_removed"]) == (1, 12)
    if name == "tip_of_max_tip_plus_one":
        assert (st["n_tips"], st["rounds_run"], st["converged"]) == (0, 1, 1)
    if name == "k63_y_and_bubble":
        assert (st["n_tips"], st["n_bubbles"], len(rec)) == (1, 1, 2)
    if name == "stem_merges_three":
        assert len(rec) == 1 and (int(rec["n_kmers"][0]), int(rec["sum_count"][0]), int(rec["min_count"][0]), int(rec["max_count"][0])) == (169, 507, 3, 3)


@pytest.mark.parametrize("ops", [1, 2, 4, 3, 5, 6])
def test_ops_subsets(ops):
    """each single bit and each pair, on a dense listing and on the reads at thr = 2"""
    m = KModel(1, 1023, NH, NB)
    for name, thr in (("k7_half_thr3", 3), ("reads_thr1", 2)):
        k, _, _, _, km, cnt = listing(name)
        res = ref(name, thr, ops)
        st = res["stats"]
        assert not (st["n_tips"] and not ops & 1) and not (st["n_islands"] and not ops & 2) and not (st["n_bubbles"] and not ops & 4)
        both(m, km, cnt, k, thr, res, f"{name}, ops = {ops}", ops=ops)


def test_max_rounds_prefixes():
    """k7_half_thr3 needs four rounds: max_rounds = 1, 2, 3 stop early with converged = 0, and each prefix is the restatement's"""
    k, thr, _, _, km, cnt = listing("k7_half_thr3")
    m = KModel(1, 1023, NH, NB)
    conv = []
    for mr in (1, 2, 3, 4):
        res = ref("k7_half_thr3", thr, 7, None, None, mr)
        got = both(m, km, cnt, k, thr, res, f"max_rounds = {mr}", max_rounds=mr)
        conv.append(got[6]["converged"])
        assert got[6]["rounds_run"] == mr
    assert conv == [0, 0, 0, 1]
    full = ref("k7_half_thr3")
    assert [e["unitigs"] for e in full["log"]] == [2082, 1039, 908, 891]


@pytest.mark.parametrize("n_uni", [7, 8, 9, 31, 32, 33, 255, 256, 257])
def test_unitigs_around_the_launch_geometry(n_uni):
    """k_uni_clean gives every unitig a group of 8 lanes: a wave holds 8 unitigs, a block 32.  Listings of exactly n_uni
    unitigs with one clippable tip and one bubble among disjoint paths"""
    k = 31
    km_s, cnt = CL.geometry_listing(n_uni, 7000 + n_uni, k)
    res = CL.clean(km_s, cnt, k, 1)
    assert res["stats"]["n_unitigs_before"] == n_uni and (res["stats"]["n_tips"], res["stats"]["n_bubbles"]) == (1, 1)
    both(KModel(1, 1023, NH, NB), U.pack(km_s, k), np.asarray(cnt, dtype=np.uint32), k, 1, res, f"{n_uni} unitigs")


def test_listing_sizes_at_the_launch_edges():
    """k_uni_drop runs one thread per entry in blocks of 256: the first n entries of a dense listing, which are a listing"""
    k, _, km_s, cnt_l, km, cnt = listing("k7_half_thr1")
    m = KModel(1, 1023, NH, NB)
    for n in (1, 2, 255, 256, 257, 511, 512, 513):
        res = CL.clean(km_s[:n], cnt_l[:n], k, 1)
        both(m, km[:n], cnt[:n], k, 1, res, f"n = {n}")


def test_counted_session():
    """reads at 20x with 1 % errors counted through kmx_count_*: thr = 2 cleans the graph down to one unitig; the listing and
    the uncleaned graph are afterwards what they were"""
    reads = U.CASES["reads_thr1"]()[2]
    k, thr = 21, 2
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    m.count_finish()
    lk_km, lk_cnt = m.count_listing()
    before = m.count_unitig_graph(thr)
    res = CL.clean(U.unpack(lk_km, k), lk_cnt.tolist(), k, thr)
    got = m.count_unitig_graph_clean(thr)
    same(got, res, "count_unitig_graph_clean")
    same(from_torch(m.count_unitig_graph_clean_dev(thr)), res, "count_unitig_graph_clean_dev")
    assert len(got[2]) == 1 and len(before[2]) == 53 and (got[6]["n_tips"], got[6]["n_islands"], got[6]["n_bubbles"], got[6]["rounds_run"]) == (15, 7, 5, 2)
    lk2, lc2 = m.count_listing()
    assert np.array_equal(lk2, lk_km) and np.array_equal(lc2, lk_cnt), "the listing changed"
    after = m.count_unitig_graph(thr)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), "count_unitig_graph changed after a cleaning call"


def params(ops=7, max_tip=42, max_bubble=42, max_rounds=16):
    return CleanParams(ops, max_tip, max_bubble, max_rounds)


def raw(m, fn, head, P, seq_cap, rec_cap, link_cap, n, give_seq=True, give_removed=True, give_stats=True):
    """one call on device buffers that are longer than the capacities it is told, filled with sentinels
    -> (rc, (n_unitigs, n_bases, n_links), stats dict, removed, seq, offs, rec, loffs, links)"""
    import torch
    seq = torch.full((seq_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    offs = torch.full((rec_cap + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    rec = torch.full(((rec_cap + 2) * 40,), 0xA5, dtype=torch.uint8, device="cuda")
    loffs = torch.full((2 * rec_cap + 1 + 8,), -7, dtype=torch.int64, device="cuda")
    links = torch.full((link_cap + 16,), -8, dtype=torch.int32, device="cuda")
    removed = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    nu, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    st = CleanStats()
    rc = fn(m.h, *head, C.addressof(P) if P is not None else None, seq.data_ptr() if give_seq else None, seq_cap, offs.data_ptr(), rec.data_ptr(), rec_cap,
            loffs.data_ptr(), links.data_ptr(), link_cap, C.byref(nu), C.byref(nb), C.byref(nl), removed.data_ptr() if give_removed else None,
            C.addressof(st) if give_stats else None)
    torch.cuda.synchronize()
    return (rc, (nu.value, nb.value, nl.value), {f: int(getattr(st, f)) for f, _ in CleanStats._fields_}, removed.cpu().numpy(),
            seq.cpu().numpy(), offs.cpu().numpy(), rec.cpu().numpy(), loffs.cpu().numpy(), links.cpu().numpy())


def untouched(seq, offs, rec, loffs, links):
    return np.all(seq == 0xA5) and np.all(offs == -6) and np.all(rec == 0xA5) and np.all(loffs == -7) and np.all(links == -8)


def test_capacities_sizing_and_sentinels():
    """the sizing call returns the cleaned counts, stats and removed and writes no output buffer; exact capacities succeed with
    the sentinels intact behind them; each capacity one short is KMX_E_RANGE with the three counts, stats and removed complete
    and the output buffers untouched; the uncleaned call's counts as capacities succeed; removed = NULL and stats = NULL are
    accepted"""
    name = "k7_half_thr3"                                       # four rounds; 891 unitigs and their links are left
    k, thr, _, _, km, cnt = listing(name)
    n = len(cnt)
    res = ref(name)
    wbuf, woff, wrec, wloff, wlk, wrem = CL.flat(res)
    nu, nb, nl = len(wrec), len(wbuf), len(wlk)
    assert nu == 891 and nl >= 2 and res["stats"]["rounds_run"] == 4
    m = KModel(1, 1023, NH, NB)
    d_km, d_cnt = to_dev(km, cnt)
    head = (k, d_km.data_ptr(), d_cnt.data_ptr(), n, thr)
    P = params(7, 2 * k, 2 * k, 16)
    fn = m.L.kmx_unitig_graph_clean_dev

    def complete(st, rem):
        return st == res["stats"] and rem[:n].tobytes() == wrem.tobytes() and np.all(rem[n:] == 0x5A)

    rc, counts, st, rem, *bufs = raw(m, fn, head, P, nb, nu, nl, n, give_seq=False)
    assert (rc, counts) == (0, (nu, nb, nl)) and complete(st, rem) and untouched(*bufs)

    def exact(out):
        rc, counts, st, rem, seq, offs, rec, loffs, links = out
        assert (rc, counts) == (0, (nu, nb, nl))
        assert seq[:nb].tobytes() == wbuf.tobytes() and np.array_equal(offs[:nu + 1].view(np.uint64), woff)
        assert rec[:nu * 40].tobytes() == wrec.tobytes() and loffs[:2 * nu + 1].tobytes() == wloff.tobytes() and links[:nl].tobytes() == wlk.tobytes()
        return st, rem, seq, offs, rec, loffs, links

    st, rem, seq, offs, rec, loffs, links = exact(raw(m, fn, head, P, nb, nu, nl, n))
    assert complete(st, rem)
    assert np.all(seq[nb:] == 0xA5) and np.all(offs[nu + 1:] == -6) and np.all(rec[nu * 40:] == 0xA5) and np.all(loffs[2 * nu + 1:] == -7) and np.all(links[nl:] == -8)
    for sc, rcap, lcap in ((nb - 1, nu, nl), (nb, nu - 1, nl), (nb, nu, nl - 1)):
        rc, counts, st, rem, *bufs = raw(m, fn, head, P, sc, rcap, lcap, n)
        assert (rc, counts) == (-5, (nu, nb, nl)), (sc, rcap, lcap)
        assert complete(st, rem) and untouched(*bufs), (sc, rcap, lcap)
    s0 = res["stats"]
    b0 = len(m.unitig_graph(km, cnt, k, thr)[0])
    exact(raw(m, fn, head, P, b0, s0["n_unitigs_before"], s0["n_links_before"], n))
    st, rem, *_ = exact(raw(m, fn, head, P, nb, nu, nl, n, give_removed=False))
    assert st == res["stats"] and np.all(rem == 0x5A)
    exact(raw(m, fn, head, P, nb, nu, nl, n, give_stats=False))
    # the host variant reports the same
    obuf, ooff = np.full(nb + 8, 0xA5, dtype=np.uint8), np.full(nu + 1, 6, dtype=np.uint64)
    oloff, olk = np.full(2 * nu + 1, 7, dtype=np.uint64), np.full(nl + 8, 8, dtype=np.uint32)
    orem = np.full(n + 8, 0x5A, dtype=np.uint8)
    cu, cb, cl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    hst = CleanStats()
    host = (m.h, k, km.ctypes.data, cnt.ctypes.data, n, thr, C.addressof(P), obuf.ctypes.data)
    tail = (C.byref(cu), C.byref(cb), C.byref(cl), orem.ctypes.data, C.addressof(hst))
    for sc, rcap, lcap in ((nb - 1, nu, nl), (nb, nu - 1, nl), (nb, nu, nl - 1)):
        rc = m.L.kmx_unitig_graph_clean(*host, sc, ooff.ctypes.data, None, rcap, oloff.ctypes.data, olk.ctypes.data, lcap, *tail)
        assert (rc, cu.value, cb.value, cl.value) == (-5, nu, nb, nl)
        assert np.all(obuf == 0xA5) and np.all(ooff == 6) and np.all(oloff == 7) and np.all(olk == 8)
        assert {f: int(getattr(hst, f)) for f, _ in CleanStats._fields_} == res["stats"] and orem[:n].tobytes() == wrem.tobytes() and np.all(orem[n:] == 0x5A)
    rc = m.L.kmx_unitig_graph_clean(*host, nb, ooff.ctypes.data, None, nu, oloff.ctypes.data, olk.ctypes.data, nl, *tail)
    assert rc == 0 and obuf[:nb].tobytes() == wbuf.tobytes() and np.all(obuf[nb:] == 0xA5) and ooff.tobytes() == woff.tobytes()
    assert oloff.tobytes() == wloff.tobytes() and olk[:nl].tobytes() == wlk.tobytes() and np.all(olk[nl:] == 8)
    rc = m.L.kmx_unitig_graph_clean(*host, nb, ooff.ctypes.data, None, nu, oloff.ctypes.data, olk.ctypes.data, nl, C.byref(cu), C.byref(cb), C.byref(cl), None, None)
    assert rc == 0 and obuf[:nb].tobytes() == wbuf.tobytes()


def test_refusals():
    """ops 0 or 8, max_tip = 0, max_bubble = 0, max_rounds 0 or 65, NULL params, thr = 0, even k, bad listings and no session
    listing; nothing is written, and the handle answers the next call"""
    name = "k7_linear300"
    k, thr, _, _, km, cnt = listing(name)
    n = len(cnt)
    m = KModel(1, 1023, NH, NB)
    d_km, d_cnt = to_dev(km, cnt)
    head = (k, d_km.data_ptr(), d_cnt.data_ptr(), n, thr)
    fn = m.L.kmx_unitig_graph_clean_dev
    for P in (params(ops=0), params(ops=8), params(max_tip=0), params(max_bubble=0), params(max_rounds=0), params(max_rounds=65), None):
        rc, counts, st, rem, *bufs = raw(m, fn, head, P, 4096, 64, 64, n)
        assert rc == -1 and counts == (0, 0, 0) and untouched(*bufs) and np.all(rem == 0x5A) and not any(st.values())
    rc, counts, st, rem, *bufs = raw(m, fn, (k, d_km.data_ptr(), d_cnt.data_ptr(), n, 0), params(), 4096, 64, 64, n)
    assert rc == -1 and untouched(*bufs)
    assert raw(m, fn, head, params(max_rounds=64), 4096, 256, 2048, n)[0] == 0     # (8 links per node always suffice)
    swapped = km.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    dup = km.copy()
    dup[20] = dup[19]
    for bad in (swapped, dup):
        for call in (m.unitig_graph_clean, lambda kk, cc, *a: m.unitig_graph_clean_dev(*to_dev(kk, cc), *a)):
            with pytest.raises(KmxError) as e:
                call(bad, cnt, k, 1)
            assert e.value.code == -1
    for kk in (4, 6, 30, 32, 64):                                   # even
        with pytest.raises(KmxError) as e:
            m.unitig_graph_clean(np.zeros(2 * ((kk + 31) // 32), np.uint64), np.ones(2, np.uint32), kk, 1)
        assert e.value.code == -1
    for call in (m.count_unitig_graph_clean, m.count_unitig_graph_clean_dev):
        with pytest.raises(KmxError) as e:                          # no listing
            call(1)
        assert e.value.code == -4
    both(m, km, cnt, k, thr, ref(name), "after the refusals")


def test_empty_and_thr_above_every_count():
    k, _, _, _, km, cnt = listing("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    for kk, cc, thr in ((km[:0], cnt[:0], 1), (km, cnt, int(cnt.max()) + 1)):
        buf, off, rec, loff, lk, removed, st = m.unitig_graph_clean(kk, cc, k, thr)
        assert len(buf) == 0 and len(rec) == 0 and off.tolist() == [0] and loff.tolist() == [0] and len(lk) == 0 and not removed.any()
        assert st == dict.fromkeys(CL.STATS, 0) | {"rounds_run": 1, "converged": 1}
        d_km, d_cnt = to_dev(kk, cc)
        rc, counts, st, rem, seq, offs, rec, loffs, links = raw(m, m.L.kmx_unitig_graph_clean_dev, (k, d_km.data_ptr() or None, d_cnt.data_ptr() or None, len(cc), thr), params(), 4, 4, 4, len(cc))
        assert (rc, counts) == (0, (0, 0, 0)) and offs[0] == 0 and loffs[0] == 0 and (st["rounds_run"], st["converged"]) == (1, 1)
        assert np.all(offs[1:] == -6) and np.all(loffs[1:] == -7) and np.all(seq == 0xA5) and np.all(links == -8) and not rem[:len(cc)].any()


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first kmx_unitig_graph_clean call with exact room; the same call then succeeds on
    the same handle with the right bytes"""
    name = "y_short_branch_goes"
    k, thr, km_s, cnt, p, res = CL.clean_case(name)
    km, cnt = U.pack(km_s, k), np.asarray(cnt, dtype=np.uint32)
    wbuf, woff, wrec, wloff, wlk, wrem = CL.flat(res)
    nu, nb, nl, n = len(wrec), len(wbuf), len(wlk), len(cnt)
    P = params(*p)
    failed = 0
    for nth in range(1, 26):
        m = KModel(1, 1023, NH, NB)                             # fresh: every buffer of the call is still to be allocated
        obuf, ooff, orec = np.zeros(nb, np.uint8), np.zeros(nu + 1, np.uint64), np.zeros(nu, UNITIG_DTYPE)
        oloff, olk, orem = np.zeros(2 * nu + 1, np.uint64), np.zeros(max(nl, 1), np.uint32), np.zeros(n, np.uint8)
        cu, cb, cl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        st = CleanStats()

        def call():
            return m.L.kmx_unitig_graph_clean(m.h, k, km.ctypes.data, cnt.ctypes.data, n, thr, C.addressof(P), obuf.ctypes.data, nb, ooff.ctypes.data, orec.ctypes.data, nu,
                                              oloff.ctypes.data, olk.ctypes.data, nl, C.byref(cu), C.byref(cb), C.byref(cl), orem.ctypes.data, C.addressof(st))

        monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
        rc = call()
        monkeypatch.delenv("KMX_FAIL_ALLOC")
        assert rc in (0, -6), (nth, rc)
        failed += rc == -6
        assert call() == 0 and (cu.value, cb.value, cl.value) == (nu, nb, nl), nth
        assert obuf.tobytes() == wbuf.tobytes() and ooff.tobytes() == woff.tobytes() and orec.tobytes() == wrec.tobytes(), nth
        assert oloff.tobytes() == wloff.tobytes() and olk[:nl].tobytes() == wlk.tobytes() and orem.tobytes() == wrem.tobytes(), nth
        assert {f: int(getattr(st, f)) for f, _ in CleanStats._fields_} == res["stats"], nth
    assert failed >= 18, failed


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_clean.cpp and the driver's -u2 -C -G write the GFA and the FASTA of the restatement's cleaned graph;
    without -C the files are those of the uncleaned graph"""
    import count_reads as CR
    k, thr = 21, 2
    reads = [r.encode() for r in U.CASES["reads_thr1"]()[2]]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, reads)
    m = KModel(1, 1023, NH, NB)
    m.init_reads(fa, k)
    km, cnt = m.count_listing()
    km_s = U.unpack(km, k)
    res = CL.clean(km_s, cnt.tolist(), k, thr)
    off, lk = UL.flat_links(res["rows"])
    want_gfa = UL.gfa(res["strs"], res["recs"], off, lk, k)
    strs0, recs0 = U.unitigs(km_s, cnt.tolist(), k, thr)
    off0, lk0 = UL.flat_links(UL.links(km_s, cnt.tolist(), k, thr, strs0))
    assert len(res["strs"]) == 1 and len(strs0) == 53

    def build(source, name):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    listing_txt = str(tmp_path / "listing.txt")
    with open(listing_txt, "w") as f:
        f.write("".join(f"{int(x)} {int(c)}\n" for x, c in zip(km, cnt)))
    out = subprocess.check_output([build("tests/facade_unitig_clean.cpp", "facade_unitig_clean"), fa, str(k), str(thr), listing_txt], timeout=120).decode()
    assert out == want_gfa
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    plain, cleaned = tmp_path / "plain", tmp_path / "cleaned"
    plain.mkdir()
    cleaned.mkdir()
    subprocess.check_call([exe, "-g", f"-u{thr}", "-G", f"-k{k}", "-nh3", "-nb2", fa, "db", str(plain)], timeout=120)
    log = subprocess.check_output([exe, "-g", f"-u{thr}", "-C", "-G", f"-k{k}", "-nh3", "-nb2", fa, "db", str(cleaned)], timeout=120).decode()
    assert (cleaned / "db" / "unitigs.gfa").read_text() == want_gfa
    fasta = (cleaned / "db" / "unitigs.fa").read_text()
    assert [ln for ln in fasta.splitlines() if not ln.startswith(">")] == res["strs"] and fasta.count(">") == 1
    assert "15 tips" in log and "7 islands" in log and "5 bubbles" in log and "2 rounds" in log
    assert (plain / "db" / "unitigs.gfa").read_text() == UL.gfa(strs0, recs0, off0, lk0, k)
    assert (plain / "db" / "unitigs.fa").read_text().count(">") == 53
