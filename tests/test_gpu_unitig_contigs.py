"""kmx_unitig_contigs* on the MI355X: every output array, the stats and the three counts equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitig_contigs_ref.py) gives, for the host and the device form, on every case at five parameter
pairs, with link hits from the library's own walks on a live session and from the restatement; the cut cases (lines and rings of
1 to 1000 unitigs, half of them reverse-complemented, across several emit tiles); consequence (b) live; U == 0, urec == NULL,
hits near 2^63; refusals; crafted device input inside guard bands; allocation failures; the facade and the driver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import unitig_contigs_ref as G
import unitig_links_ref as L
import unitig_map_ref as R
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import CONTIG_DTYPE, CONTIG_PLACE_DTYPE, ContigParams, ContigStats, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the contigs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat_input(k, strs, recs, rows):
    """-> (ubuf, uoffsets, urec or None, link_offsets, links) as the graph calls return them"""
    ubuf, uoff = R.join(strs)
    urec = U.flat(strs, recs)[2] if recs is not None else None
    loff, lk = L.flat_links(rows)
    return ubuf, uoff, urec, loff, lk


@functools.lru_cache(maxsize=None)
def listed_input(name):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    return (k,) + flat_input(k, strs, recs, rows)


def same(got, exp, what=""):
    for a, b, part in zip(got, exp, G.PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"


def stats_array(st):
    return np.array([st[f] for f in G.STAT_FIELDS], dtype=np.uint64)


def run_host(m, k, ubuf, uoff, urec, loff, lk, hits, min_reads, ratio):
    out = m.unitig_contigs_flat(k, ubuf, uoff, loff, lk, hits, min_reads, ratio, urec)
    st = out[8]
    return out[:8] + (stats_array(st), np.array([len(out[2]), len(out[0]), len(out[6])], dtype=np.uint64))


def to_dev(a, view):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda()


def dev_input(ubuf, uoff, urec, loff, lk):
    import torch
    return (to_dev(ubuf, np.uint8) if len(ubuf) else torch.zeros(1, dtype=torch.uint8, device="cuda"), to_dev(uoff, np.int64), to_dev(loff, np.int64),
            to_dev(lk, np.int32) if len(lk) else torch.zeros(0, dtype=torch.int32, device="cuda"),
            to_dev(urec.view(np.uint8).reshape(-1, 40), np.uint8) if urec is not None and len(urec) else None)


def run_dev(m, k, dev, n_ubases, hits, min_reads, ratio):
    import torch
    d_ubuf, d_uoff, d_loff, d_lk, d_urec = dev
    d_hits = to_dev(hits, np.int64) if len(hits) else torch.zeros(0, dtype=torch.int64, device="cuda")
    out, (nc, nb, nl), st = m.unitig_contigs_dev(k, d_ubuf[:n_ubases], d_uoff, d_loff, d_lk, d_hits, min_reads, ratio, d_urec)
    torch.cuda.synchronize()
    nu = d_uoff.numel() - 1
    h = [t.cpu().numpy() for t in out]
    return (h[0][:nb], h[1].view(np.uint64)[:nc + 1], h[2][:nc].reshape(-1).view(CONTIG_DTYPE), h[3].view(np.uint32)[:nu], h[4][:nu].reshape(-1).view(CONTIG_PLACE_DTYPE),
            h[5].view(np.uint64)[:2 * nc + 1], h[6].view(np.uint32)[:nl], h[7].view(np.uint64)[:nl], stats_array(st), np.array([nc, nb, nl], dtype=np.uint64))


def library_hits(name):
    """link_hits of the case's reads from the library's own walks on a live session, at (0, 0) and (k, 1): they are the restatement's"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    loff, lk = L.flat_links(rows)
    m = KModel(1, 1023, NH, NB)
    m.unitig_map_begin(U.pack(km, k), k, *R.join(strs))
    got = {}
    for which, (gap, indel) in (("exact", (0, 0)), ("bridged", (k, 1))):
        hits = np.zeros(len(lk), dtype=np.uint64)
        m.seq_to_walks(list(reads), loff, lk, gap, indel, link_hits=hits)
        assert hits.tolist() == list(G.hits_of(name, which)), f"{name}: the library's link hits ({which}) are not the restatement's"
        got[which] = hits
    m.unitig_map_end()
    return got


@pytest.mark.parametrize("name", G.LISTED_CASES)
def test_equals_the_restatement(name):
    """host form and device form, every output array, the stats and the three counts, on every case x hits x parameter pair"""
    k, ubuf, uoff, urec, loff, lk = listed_input(name)
    hits = library_hits(name)
    m = KModel(1, 1023, NH, NB)
    dev = dev_input(ubuf, uoff, urec, loff, lk)
    for which in ("exact", "bridged"):
        for pair in G.PARAMS:
            exp = G.flat(G.want(name, which, *pair))
            same(run_host(m, k, ubuf, uoff, urec, loff, lk, hits[which], *pair), exp, f"{name} {which} {pair}: host")
            same(run_dev(m, k, dev, len(ubuf), hits[which], *pair), exp, f"{name} {which} {pair}: device")


def test_the_cases_are_not_trivial():
    st = G.want("k31_tangle", "exact", 2, 0)
    assert st["stats"]["n_contigs"] == 64 and st["stats"]["n_multi"] == 7 and max(r["n_steps"] for r in st["crecs"]) == 14 and sum(o & 1 for o in st["steps"]) == 24
    assert G.want("k21_every_kind", "exact", 2, 4)["stats"]["n_below_ratio"] == 24 and G.want("k21_every_kind", "exact", 2, 0)["stats"]["n_below_ratio"] == 0
    ring = G.want(G.RING, "exact", 1, 0)
    assert ring["stats"]["n_contigs"] == 3 and [r["n_steps"] for r in ring["crecs"] if r["circular"]] == [2]


@pytest.mark.parametrize("ring", (False, True), ids=("line", "ring"))
@pytest.mark.parametrize("k", G.CUT_K)
def test_cut_cases(k, ring):
    """a sequence cut into N unitigs, a random half reverse-complemented: one contig, the sequence or its reverse complement, and
    every array the restatement's; doubling depth, power-of-two cycles, reverse steps, pieces across several emit tiles"""
    m = KModel(1, 1023, NH, NB)
    for n in G.CUT_N:
        kk, strs, rows, hits, text = G.cut_case(n, k, ring)
        res = G.want_cut(n, k, ring)
        exp = G.flat(res)
        assert len(res["cstrs"]) == 1 and res["cstrs"][0] == G.cut_expected(n, k, ring) and res["crecs"][0]["circular"] == int(ring)
        ubuf, uoff, urec, loff, lk = flat_input(k, strs, None, rows)
        h = np.array(hits, dtype=np.uint64)
        got = run_host(m, k, ubuf, uoff, None, loff, lk, h, 1, 0)
        same(got, exp, f"cut n={n} k={k} ring={ring}: host")
        assert got[0].tobytes().decode() == G.cut_expected(n, k, ring)
        same(run_dev(m, k, dev_input(ubuf, uoff, None, loff, lk), len(ubuf), h, 1, 0), exp, f"cut n={n} k={k} ring={ring}: device")


def test_contigs_are_a_valid_set_for_the_map():
    """consequence (b), live: unitig_map_begin on the contigs of k21_every_kind succeeds and the case's reads map with at least as
    many windows as onto the unitigs"""
    name = "k21_every_kind"
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    _, ubuf, uoff, urec, loff, lk = listed_input(name)
    m = KModel(1, 1023, NH, NB)
    packed = U.pack(km, k)
    m.unitig_map_begin(packed, k, ubuf, uoff)
    out = m.contigs_from_walks(k, ubuf, uoff, loff, lk, list(reads), 0, 0, 2, 4, urec)
    on_unitigs = int(m.seq_to_unitigs(list(reads))[2]["n_mapped"].sum())
    assert out[9].tolist() == list(G.hits_of(name, "exact"))
    same(out[:8], G.flat(G.want(name, "exact", 2, 4))[:8], "contigs_from_walks")
    assert len(out[2]) == 13 < len(strs)
    m.unitig_map_begin(packed, k, out[0], out[1])                # the second begin ends the first session
    on_contigs = int(m.seq_to_unitigs(list(reads))[2]["n_mapped"].sum())
    m.unitig_map_end()
    assert on_contigs >= on_unitigs > 0


def raw_host(m, k, ubuf, uoff, urec, loff, lk, hits, par, swap=()):
    """one kmx_unitig_contigs call on freshly allocated outputs -> rc; swap replaces an argument by name (a pointer or None)"""
    nu = len(uoff) - 1
    a = {"useq": ubuf.ctypes.data, "uoffsets": uoff.ctypes.data, "urec": urec.ctypes.data if urec is not None else None, "link_offsets": loff.ctypes.data, "links": lk.ctypes.data,
         "link_hits": hits.ctypes.data, "params": C.byref(par)}
    keep = [np.zeros(max(len(ubuf), 1), np.uint8), np.zeros(nu + 1, np.uint64), np.zeros(max(nu, 1), CONTIG_DTYPE), np.zeros(max(nu, 1), np.uint32), np.zeros(max(nu, 1), CONTIG_PLACE_DTYPE),
            np.zeros(2 * nu + 1, np.uint64), np.zeros(max(len(lk), 1), np.uint32), np.zeros(max(len(lk), 1), np.uint64)]
    for name_, arr in zip(("cseq", "coffsets", "crec", "steps", "place", "clink_offsets", "clinks", "csupport"), keep):
        a[name_] = arr.ctypes.data
    st, nc, nb, nl = ContigStats(), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    a.update(n_contigs=C.byref(nc), n_cbases=C.byref(nb), n_clinks=C.byref(nl), stats=C.byref(st), k=k, n_unitigs=nu, n_links=len(lk))
    a.update(dict(swap))
    return m.L.kmx_unitig_contigs(m.h, a["k"], a["useq"], a["uoffsets"], a["n_unitigs"], a["urec"], a["link_offsets"], a["links"], a["n_links"], a["link_hits"], a["params"], a["cseq"],
                                  a["coffsets"], a["crec"], a["steps"], a["place"], a["clink_offsets"], a["clinks"], a["csupport"], a["n_contigs"], a["n_cbases"], a["n_clinks"], a["stats"])


def test_refusals():
    """every KMX_E_ARG of the header, host form and (where it applies) device form, each leaving the handle usable"""
    import torch
    name, pair = "k31_tangle", (2, 0)
    k, ubuf, uoff, urec, loff, lk = listed_input(name)
    hits = np.array(G.hits_of(name, "exact"), dtype=np.uint64)
    exp = G.flat(G.want(name, "exact", *pair))
    m = KModel(1, 1023, NH, NB)
    nu = len(uoff) - 1
    args = (m, k, ubuf, uoff, urec, loff, lk, hits)
    good = ContigParams(*pair, 0)
    assert raw_host(*args, good) == 0
    for bad_k in (4, 22, 3, 65, 64):
        assert raw_host(*args, good, {"k": bad_k}) == -1
    assert raw_host(*args, good, {"n_unitigs": 2 ** 31}) == -1
    assert raw_host(*args, ContigParams(2, 65537, 0)) == -1 and raw_host(*args, ContigParams(2, 65536, 0)) == 0
    assert raw_host(*args, ContigParams(2, 0, 1)) == -1
    for gone in ("useq", "uoffsets", "link_offsets", "links", "link_hits", "params", "cseq", "coffsets", "crec", "steps", "place", "clink_offsets", "clinks", "csupport", "n_contigs", "n_cbases",
                 "n_clinks", "stats"):
        assert raw_host(*args, good, {gone: None}) == -1, gone
    assert raw_host(*args, good, {"urec": None}) == 0
    assert raw_host(*args, good, {"cseq": ubuf.ctypes.data}) == -1 and raw_host(*args, good, {"csupport": hits.ctypes.data}) == -1 and raw_host(*args, good, {"coffsets": uoff.ctypes.data + 8}) == -1
    first = uoff.copy()
    first[0] = 1
    dec = uoff.copy()
    dec[2], dec[3] = uoff[3], uoff[2]
    short = np.array([0, k - 1] + [int(x) for x in uoff[2:]], dtype=np.uint64)
    for bad in (first, dec, short):
        assert raw_host(m, k, ubuf, bad, urec, loff, lk, hits, good) == -1
    lo_first = loff.copy()
    lo_first[0] = 1
    lo_dec = loff.copy()
    lo_dec[3], lo_dec[4] = loff[4] + 1, loff[3]
    lo_short = loff.copy()
    lo_short[-1] -= 1
    lo_row5 = loff.copy()                                        # one row takes everything in front of the next rows that still have room: 5 or more entries
    o = 0
    while int(loff[o + 3]) - int(loff[o]) < 5:
        o += 1
    lo_row5[o + 1] = lo_row5[o + 2] = loff[o + 3]
    for bad in (lo_first, lo_dec, lo_short, lo_row5):
        assert raw_host(m, k, ubuf, uoff, urec, bad, lk, hits, good) == -1
    bad_lk = lk.copy()
    bad_lk[len(lk) // 2] = 2 * nu
    no_mirror = lk.copy()
    rows = L.rows_of(loff, lk)
    a = next(x for x, row in enumerate(rows) if row and row[0] != x and row[0] != x ^ 1 and (x ^ 1) not in row)
    no_mirror[int(loff[a])] = a ^ 1                              # a -> a ^ 1 in place of a -> b: b ^ 1 -> a ^ 1 has lost its mirror
    for bad in (bad_lk, no_mirror):
        assert raw_host(m, k, ubuf, uoff, urec, loff, bad, hits, good) == -1
    # the device form: what it can check without reading a buffer
    dev = dev_input(ubuf, uoff, urec, loff, lk)
    d_hits = to_dev(hits, np.int64)
    for kw in ({"k": 22}, {"min_reads": 2, "ratio": 65537}):
        with pytest.raises(KmxError) as e:
            m.unitig_contigs_dev(kw.get("k", k), dev[0], dev[1], dev[2], dev[3], d_hits, kw.get("min_reads", 2), kw.get("ratio", 0), dev[4])
        assert e.value.code == -1
    out, _, _ = m.unitig_contigs_dev(k, dev[0], dev[1], dev[2], dev[3], d_hits, 2, 0, dev[4])
    for i, t in ((0, dev[0]), (7, d_hits), (1, dev[1])):         # an output that is an input
        swapped = list(out)
        swapped[i] = t
        with pytest.raises(KmxError) as e:
            m.unitig_contigs_dev(k, dev[0], dev[1], dev[2], dev[3], d_hits, 2, 0, dev[4], out=tuple(swapped))
        assert e.value.code == -1
    torch.cuda.synchronize()
    same(run_host(*args, *pair), exp, "host, after the refusals")
    same(run_dev(m, k, dev, len(ubuf), hits, *pair), exp, "device, after the refusals")


def test_no_unitigs_no_records_and_hits_near_2_63():
    import torch
    m = KModel(1, 1023, NH, NB)
    # U == 0: KMX_OK, coffsets[0] = clink_offsets[0] = 0, zero counts
    z64 = np.full(1, 7, dtype=np.uint64)
    co, clo = z64.copy(), z64.copy()
    st, nc, nb, nl = ContigStats(), C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    st.n_links = 5
    par = ContigParams(1, 0, 0)
    zero = np.zeros(1, dtype=np.uint64)
    rc = m.L.kmx_unitig_contigs(m.h, 21, None, zero.ctypes.data, 0, None, zero.ctypes.data, None, 0, None, C.byref(par), None, co.ctypes.data, None, None, None, clo.ctypes.data, None, None,
                                C.byref(nc), C.byref(nb), C.byref(nl), C.byref(st))
    assert rc == 0 and co[0] == clo[0] == 0 and (nc.value, nb.value, nl.value) == (0, 0, 0) and not any(st.as_dict().values())
    d_zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_co, d_clo = torch.full((1,), 7, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda")
    nc.value = 9
    rc = m.L.kmx_unitig_contigs_dev(m.h, 21, None, d_zero.data_ptr(), 0, 0, None, d_zero.data_ptr() + 0, None, 0, None, C.byref(par), None, d_co.data_ptr(), None, None, None, d_clo.data_ptr(), None, None,
                                    C.byref(nc), C.byref(nb), C.byref(nl), C.byref(st))
    torch.cuda.synchronize()
    assert rc == 0 and d_co.item() == d_clo.item() == 0 and nc.value == 0
    # urec == NULL: the three count fields are 0, everything else as with the records
    name, pair = "k31_tangle", (2, 0)
    k, ubuf, uoff, urec, loff, lk = listed_input(name)
    kk, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    hits = list(G.hits_of(name, "exact"))
    exp = G.flat(G.contigs(k, strs, None, rows, hits, *pair))
    assert not exp[2]["sum_count"].any() and not exp[2]["min_count"].any() and G.flat(G.want(name, "exact", *pair))[2]["sum_count"].all()
    h = np.array(hits, dtype=np.uint64)
    same(run_host(m, k, ubuf, uoff, None, loff, lk, h, *pair), exp, "urec = NULL, host")
    same(run_dev(m, k, dev_input(ubuf, uoff, None, loff, lk), len(ubuf), h, *pair), exp, "urec = NULL, device")
    # hits near 2^63 with ratio = 65536: the product needs 128 bits
    big = [(1 << 63) - 1 - 3 * (e % 5) if x else 0 for e, x in enumerate(hits)]
    big[hits.index(max(hits))] = (1 << 63) - 1
    small = list(big)
    for e, x in enumerate(hits):
        if x == 1:
            small[e] = 1 << 46                                     # 2 * 2^46 * 65536 = 2^63 < best: below_ratio only in 128 bits (2^63 * 65536 mod 2^64 = 0 would be, too, for the wrong reason)
    for hh in (big, small):
        res = G.contigs(k, strs, recs, rows, hh, 1, 65536)
        exp = G.flat(res)
        ha = np.array(hh, dtype=np.uint64)
        same(run_host(m, k, ubuf, uoff, urec, loff, lk, ha, 1, 65536), exp, "hits near 2^63, host")
        same(run_dev(m, k, dev_input(ubuf, uoff, urec, loff, lk), len(ubuf), ha, 1, 65536), exp, "hits near 2^63, device")
    assert G.contigs(k, strs, recs, rows, big, 1, 65536)["stats"]["n_below_ratio"] == 0 < G.contigs(k, strs, recs, rows, small, 1, 65536)["stats"]["n_below_ratio"]


GUARD = 64


def raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, pair, n_unitigs=None):
    """one kmx_unitig_contigs_dev call on output buffers longer than it is told, filled with guard bytes -> (rc, counts, stats, outputs as
    numpy, a function that says whether every guard band is intact)"""
    import torch
    nu = len(uoff) - 1 if n_unitigs is None else n_unitigs
    nb, nl = len(ubuf), len(lk)
    sizes = (nb, (nu + 1) * 8, nu * 64, nu * 4, nu * 8, (2 * nu + 1) * 8, nl * 4, nl * 8)
    outs = [torch.full((s + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for s in sizes]
    ins = [to_dev(ubuf, np.uint8), to_dev(uoff, np.int64), to_dev(urec.view(np.uint8), np.uint8) if urec is not None else None, to_dev(loff, np.int64), to_dev(lk, np.int32), to_dev(hits, np.int64)]
    before = [t.clone() for t in ins if t is not None]
    st, nc, ncb, ncl = ContigStats(), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    par = ContigParams(*pair, 0)
    rc = m.L.kmx_unitig_contigs_dev(m.h, k, ins[0].data_ptr(), ins[1].data_ptr(), nu, nb, ins[2].data_ptr() if ins[2] is not None else None, ins[3].data_ptr(), ins[4].data_ptr(), nl, ins[5].data_ptr(),
                                    C.byref(par), *[t.data_ptr() for t in outs], C.byref(nc), C.byref(ncb), C.byref(ncl), C.byref(st))
    torch.cuda.synchronize()
    host = [t.cpu().numpy() for t in outs]
    intact = all(np.all(h[s:] == 0xA5) for h, s in zip(host, sizes)) and all(torch.equal(a, b) for a, b in zip([t for t in ins if t is not None], before))
    return rc, (nc.value, ncb.value, ncl.value), st.as_dict(), [h[:s] for h, s in zip(host, sizes)], intact


def test_crafted_device_input_stays_inside_the_buffers():
    """the _dev form clamps: an asymmetric CSR, targets >= 2 U, a row of 6, row bounds beyond n_links and decreasing, decreasing and
    huge uoffsets, and a CSR that links o to the chain of o ^ 1: KMX_OK, wrong contigs, every guard band and every input intact,
    the call ends; the good input then gives the right bytes"""
    name, pair = "k31_tangle", (1, 4)
    k, ubuf, uoff, urec, loff, lk = listed_input(name)
    hits = np.array(G.hits_of(name, "exact"), dtype=np.uint64)
    m = KModel(1, 1023, NH, NB)
    nu, nl, big = len(uoff) - 1, len(lk), np.uint64(2 ** 64 - 1)
    r = np.random.RandomState(7)
    asym = lk.copy()
    asym[::3] = r.randint(0, 2 * nu, len(asym[::3]))             # every third edge points somewhere else: most mirrors are gone
    beyond = lk.copy()
    beyond[1::4] = 2 * nu + r.randint(0, 5, len(beyond[1::4]))
    beyond[2::4] = 0xFFFFFFFF
    row6 = loff.copy()
    row6[1:2 * nu] = np.minimum(np.arange(1, 2 * nu, dtype=np.uint64) * np.uint64(6), np.uint64(nl))   # rows of 6 from the front, the rest empty
    twist = lk.copy()                                            # o -> t becomes o -> t ^ 1 wherever a row has one entry: links into the chains of the other orientation
    for o in range(2 * nu):
        if int(loff[o + 1]) - int(loff[o]) == 1:
            twist[int(loff[o])] ^= np.uint32(o & 1)
    selfmir = np.array([(o ^ 1) if i % 2 else o for o in range(2 * nu) for i in range(int(loff[o + 1]) - int(loff[o]))], dtype=np.uint32)   # only hairpins and self-loops
    assert len(selfmir) == nl
    bad_links = [asym, beyond, twist, selfmir, np.full(nl, 0, np.uint32), np.full(nl, 1, np.uint32)]
    bad_loff = [row6, loff + np.uint64(nl), loff[::-1].copy(), np.full(len(loff), big), np.where(np.arange(len(loff)) % 2 == 1, big, loff)]
    bad_uoff = [uoff[::-1].copy(), np.full(nu + 1, big), np.zeros(nu + 1, np.uint64), np.where(np.arange(nu + 1) % 2 == 1, big, uoff), uoff + np.uint64(len(ubuf) // 2),
                np.arange(nu + 1, dtype=np.uint64) * np.uint64(3)]
    huge_hits = np.full(nl, big)
    crafted = ([(uoff, loff, x, hits) for x in bad_links] + [(uoff, x, lk, hits) for x in bad_loff] + [(x, loff, lk, hits) for x in bad_uoff] +
               [(uoff, loff, lk, huge_hits), (bad_uoff[0], bad_loff[2], asym, huge_hits), (bad_uoff[3], row6, beyond, hits)])
    for uo, lo, links, hh in crafted:
        rc, counts, st, outs, intact = raw_dev(m, k, ubuf, uo, urec, lo, links, hh, pair)
        assert rc == 0 and intact
        assert counts[0] <= nu and st["n_kept"] + st["n_below_min"] + st["n_below_ratio"] == st["n_links"]
    rc, counts, st, outs, intact = raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, pair)
    exp = G.flat(G.want(name, "exact", *pair))
    nc, nb, ncl = counts
    assert rc == 0 and intact and counts == tuple(int(x) for x in exp[9]) and stats_array(st).tobytes() == exp[8].tobytes()
    assert outs[0][:nb].tobytes() == exp[0].tobytes() and outs[1][:(nc + 1) * 8].tobytes() == exp[1].tobytes() and outs[2][:nc * 64].tobytes() == exp[2].tobytes()
    assert outs[3].tobytes() == exp[3].tobytes() and outs[4].tobytes() == exp[4].tobytes() and outs[5][:(2 * nc + 1) * 8].tobytes() == exp[5].tobytes()
    assert outs[6][:ncl * 4].tobytes() == exp[6].tobytes() and outs[7][:ncl * 8].tobytes() == exp[7].tobytes()


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first contig call in turn, host and device form: the same call then succeeds with the
    right bytes"""
    name, pair = G.RING, (1, 0)
    k, ubuf, uoff, urec, loff, lk = listed_input(name)
    hits = np.array(G.hits_of(name, "exact"), dtype=np.uint64)
    exp = G.flat(G.want(name, "exact", *pair))
    failed = {"host": 0, "dev": 0}
    for nth in range(1, 34):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            dev = dev_input(ubuf, uoff, urec, loff, lk)
            run = (lambda: run_host(m, k, ubuf, uoff, urec, loff, lk, hits, *pair)) if variant == "host" else (lambda: run_dev(m, k, dev, len(ubuf), hits, *pair))
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run()
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run(), exp, f"after allocation {nth} failed, {variant}")
    assert failed["host"] >= 30 and failed["dev"] >= 16, failed


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_contigs.cpp prints what unitig_contigs returns for the case that reaches every join kind, with the texts of
    the three writers, and the driver's -u2 -M -W -X2,4 -G writes contigs.fa, contigs.paths.tsv and contigs.gfa: all equal the
    restatement's text; -X without -M -W is refused with a message"""
    import count_reads as CR
    import unitig_walk_ref as W
    name = "k21_every_kind"
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    noisy = list(reads[:400])
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in noisy])
    lines = str(tmp_path / "reads.txt")
    with open(lines, "w") as f:
        f.write("".join(r + "\n" for r in reads))

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    segs, so = W.mapped(name)
    hits = W.walk_segs(k, strs, segs, so, rows, 42, 2)[3]
    res = G.contigs(k, strs, recs, rows, hits, 2, 4)
    assert res["stats"]["n_multi"] > 0 and res["stats"]["n_below_ratio"] > 0
    out = subprocess.check_output([build("tests/facade_unitig_contigs.cpp", "facade_unitig_contigs"), fa, str(k), str(thr), lines, "42", "2", "2", "4"], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 9
    assert blocks[0] == "".join(" ".join(str(r[f]) for f, _ in G.CONTIG_FIELDS) + "\n" for r in res["crecs"])
    assert blocks[1] == "".join(f"{o}\n" for o in res["steps"]) and blocks[2] == "".join(f"{oc} {off}\n" for oc, off in res["place"])
    assert blocks[3] == "".join(f"{x}\n" for x in G.offsets_of(res["crows"])) + "".join(f"{t} {s}\n" for row in res["crows"] for t, s in row)
    assert blocks[4] == " ".join(str(res["stats"][f]) for f in G.STAT_FIELDS) + "\n"
    assert blocks[5] == G.fasta(res) and blocks[6] == G.paths_tsv(res) and blocks[7] == G.gfa(res, k) and blocks[8] == G.gfa(res, k, strs, recs)
    # the driver maps the reads of its input, the 400 noisy reads, at the defaults max_gap = k, max_indel = 1
    nsegs, nso, _, _ = R.map_reads(km, k, strs, noisy)
    hits = W.walk_segs(k, strs, nsegs, nso, rows, k, 1)[3]
    res = G.contigs(k, strs, recs, rows, hits, 2, 4)
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    plain, graph = tmp_path / "plain", tmp_path / "graph"
    plain.mkdir()
    graph.mkdir()
    log = subprocess.check_output([exe, "-g", f"-u{thr}", "-M", "-W", "-X2,4", f"-k{k}", "-nh3", "-nb2", fa, "db", str(plain)], timeout=120).decode()
    assert (plain / "db" / "contigs.fa").read_text() == G.fasta(res) and (plain / "db" / "contigs.paths.tsv").read_text() == G.paths_tsv(res)
    assert not (plain / "db" / "contigs.gfa").exists() and f"{res['stats']['n_contigs']} contigs ({res['stats']['n_multi']} of several unitigs" in log
    subprocess.check_call([exe, "-g", f"-u{thr}", "-M", "-W", "-X2,4", "-G", f"-k{k}", "-nh3", "-nb2", fa, "db", str(graph)], stdout=subprocess.DEVNULL, timeout=120)
    assert (graph / "db" / "contigs.gfa").read_text() == G.gfa(res, k, strs, recs) and (graph / "db" / "contigs.fa").read_text() == G.fasta(res)
    refused = subprocess.run([exe, "-g", f"-u{thr}", "-M", "-X2", f"-k{k}", fa, "db", str(plain)], stdout=subprocess.PIPE)     # -X without -W
    assert refused.returncode == 2 and b"-X needs -M -W" in refused.stdout
    assert subprocess.call([exe, "-g", f"-u{thr}", "-M", "-W", "-X2,70000", f"-k{k}", fa, "db", str(plain)], stdout=subprocess.DEVNULL) == 2
