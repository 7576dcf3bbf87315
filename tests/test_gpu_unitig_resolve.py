"""kmx_unitig_walk_through* and kmx_unitig_resolve* on the MI355X: the through hits, every output array of the resolution, both counts
and both stats equal, byte for byte, what the plain-Python restatement (tests/unitig_resolve_ref.py) gives, for the host and the
device form, on the listed cases with their real walks, planted repeats, synthetic through matrices and the emit geometry; through
hits over two batches and from the library's own live-session walks; the planted repeats end to end; the sizing call and
KMX_E_RANGE; refusals; crafted device input inside guard bands; allocation failures."""
import ctypes as C

import numpy as np
import pytest

import unitig_contigs_ref as G
import unitig_links_ref as L
import unitig_map_ref as R
import unitig_resolve_ref as X
import unitig_walk_ref as W
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import RESOLVE_PLACE_DTYPE, UNITIG_DTYPE, KmxError, ResolveParams, ResolveStats, ThroughStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the resolution
GUARD = 64
EMPTY8, EMPTY64 = np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64)


def flat_input(strs, recs, rows):
    """-> (ubuf, uoffsets, urec or None, link_offsets, links) as the graph calls return them"""
    ubuf, uoff = R.join(strs)
    urec = U.flat(strs, recs)[2] if recs is not None else None
    loff, lk = L.flat_links(rows)
    return ubuf, uoff, urec, loff, lk


def to_dev(a, view):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.from_numpy(np.zeros(1, view)).dtype, device="cuda")[:0]
    return torch.from_numpy(a.view(view)).cuda()


def same(got, exp, what=""):
    assert len(got) == len(exp) == len(X.PARTS)
    for a, b, part in zip(got, exp, X.PARTS):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), f"{what}: {part} differ"


def stats_array(st):
    return np.array([st[f] for f in X.RESOLVE_STAT_FIELDS], dtype=np.uint64)


def run_host(m, k, inp, hits, t, pair, capacity=None):
    ubuf, uoff, urec, loff, lk = inp
    out = m.unitig_resolve_flat(k, ubuf, uoff, loff, lk, np.array(t, dtype=np.uint64), pair[0], pair[1], urec, np.array(hits, dtype=np.uint64) if hits is not None else None, capacity)
    return (out[0], out[1], out[2] if out[2] is not None else EMPTY8, out[3], out[4], out[5], out[6], out[7], out[8] if out[8] is not None else EMPTY64, stats_array(out[9]),
            np.array([len(out[3]), len(out[0])], dtype=np.uint64))


def run_dev(m, k, inp, hits, t, pair):
    import torch
    ubuf, uoff, urec, loff, lk = inp
    d_urec = to_dev(urec.view(np.uint8).reshape(-1, 40), np.uint8) if urec is not None else None
    d_hits = to_dev(np.array(hits, dtype=np.uint64), np.int64) if hits is not None else None
    out, (n, b), st = m.unitig_resolve_dev(k, to_dev(ubuf, np.uint8), to_dev(uoff, np.int64), to_dev(loff, np.int64), to_dev(lk, np.int32), to_dev(np.array(t, dtype=np.uint64), np.int64),
                                           pair[0], pair[1], d_urec, d_hits)
    torch.cuda.synchronize()
    h = [x.cpu().numpy() if x is not None else None for x in out]
    nu, nl = len(uoff) - 1, len(lk)
    return (h[0][:b], h[1].view(np.uint64)[:n + 1], h[2][:n].reshape(-1).view(UNITIG_DTYPE) if h[2] is not None else EMPTY8, h[3].view(np.uint32)[:n],
            h[4][:nu].reshape(-1).view(RESOLVE_PLACE_DTYPE), h[5].view(np.uint64)[:2 * n + 1], h[6].view(np.uint32)[:nl], h[7].view(np.uint64)[:nl],
            h[8].view(np.uint64)[:nl] if h[8] is not None else EMPTY64, stats_array(st), np.array([n, b], dtype=np.uint64))


def compare(m, label, k, strs, recs, rows, hits, t, pairs=X.PARAMS):
    """host and device form against the restatement at every parameter pair, with urec / link_hits present (where the case has them)
    and NULL"""
    inp = flat_input(strs, recs, rows)
    bare = (inp[0], inp[1], None, inp[3], inp[4])
    for pair in pairs:
        exp = X.flat(X.resolve(k, strs, recs, rows, hits, list(t), *pair))
        same(run_host(m, k, inp, hits, t, pair), exp, f"{label} {pair}: host")
        same(run_dev(m, k, inp, hits, t, pair), exp, f"{label} {pair}: device")
    if recs is not None or hits is not None:
        exp = X.flat(X.resolve(k, strs, None, rows, None, list(t), *pairs[-1]))
        same(run_host(m, k, bare, None, t, pairs[-1]), exp, f"{label}: host, urec and link_hits NULL")
        same(run_dev(m, k, bare, None, t, pairs[-1]), exp, f"{label}: device, urec and link_hits NULL")


def through_host(m, walks, steps, rows, into=None):
    w, _, s, _, _ = W.flat(walks, [0], steps, [], dict.fromkeys(W.STAT_FIELDS, 0))
    loff, lk = L.flat_links(rows)
    return m.unitig_through_flat(w, s, loff, lk, into)


def through_dev(m, walks, steps, rows, d_into=None):
    import torch
    w, _, s, _, _ = W.flat(walks, [0], steps, [], dict.fromkeys(W.STAT_FIELDS, 0))
    loff, lk = L.flat_links(rows)
    d_t, st = m.unitig_through_dev(to_dev(w.view(np.uint8).reshape(-1, 80), np.uint8), len(w), to_dev(s, np.int32), len(s), to_dev(loff, np.int64), to_dev(lk, np.int32), d_into)
    torch.cuda.synchronize()
    return d_t, st


@pytest.mark.parametrize("name", G.LISTED_CASES)
def test_through_equals_the_restatement(name):
    """host and device form on the restatement's walks at (0, 0) and (k, 1); two batches accumulate to one; the reverse complements
    of all reads give the same bytes; the library's own live-session walks give the restatement's through hits and link hits"""
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    n_u = len(strs)
    m = KModel(1, 1023, NH, NB)
    for which in X.WALK_PARAMS:
        walks, _, steps, _, _ = X.listed_walks(name, which)
        exp, est = X.listed_through(name, which)
        got, st = through_host(m, walks, steps, rows)
        assert got.tolist() == list(exp) and st == est, f"{name} {which}: host"
        d_t, st = through_dev(m, walks, steps, rows)
        assert d_t.cpu().numpy().view(np.uint64).tolist() == list(exp) and st == est, f"{name} {which}: device"
        half = len(walks) // 2                                   # two batches: the walks cut in two, the second half's steps renumbered
        cut = walks[half]["first_step"] if half < len(walks) else len(steps)
        first, second = walks[:half], [dict(w, first_step=w["first_step"] - cut) for w in walks[half:]]
        acc, st1 = through_host(m, first, steps[:cut], rows)
        acc, st2 = through_host(m, second, steps[cut:], rows, acc)
        assert acc.tolist() == list(exp) and st1["n_added"] + st2["n_added"] == est["n_added"] and st1["n_missing"] == st2["n_missing"] == 0
        d_acc, _ = through_dev(m, first, steps[:cut], rows)
        d_acc, _ = through_dev(m, second, steps[cut:], rows, d_acc)
        assert d_acc.cpu().numpy().view(np.uint64).tolist() == list(exp)
        wm = X.listed_walks(name, which, True)
        assert through_host(m, wm[0], wm[2], rows)[0].tolist() == list(exp), "consequence (b)"
    loff, lk = L.flat_links(rows)
    m.unitig_map_begin(U.pack(km, k), k, *R.join(strs))
    for which, (gap, indel) in (("exact", (0, 0)), ("bridged", (k, 1))):
        hits = np.zeros(len(lk), dtype=np.uint64)
        got, st = m.through_from_walks(list(reads), loff, lk, gap, indel, link_hits=hits)
        assert got.tolist() == list(X.listed_through(name, which)[0]) and hits.tolist() == list(G.hits_of(name, which)) and st["n_missing"] == 0 and got.size == 16 * n_u
    m.unitig_map_end()


@pytest.mark.parametrize("name", G.LISTED_CASES)
def test_resolve_on_the_listed_cases(name):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    m = KModel(1, 1023, NH, NB)
    for which in X.WALK_PARAMS:
        compare(m, f"{name} {which}", k, strs, recs, rows, list(G.hits_of(name, which)), X.listed_through(name, which)[0])
    compare(m, f"{name} zero", k, strs, recs, rows, None, [0] * (16 * len(strs)), ((1, 0),))


@pytest.mark.parametrize("name", X.SYNTH_CASES)
def test_resolve_on_synthetic_through(name):
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    compare(KModel(1, 1023, NH, NB), name, k, strs, recs, rows, list(G.hits_of(name, "exact")), X.synthetic_case(name))


@pytest.mark.parametrize("name", sorted(X.PLANTED))
def test_planted_repeats_end_to_end(name):
    """every array equals the restatement's; resolved_contigs_from_walks inside a live session returns the one contig; the resolved set
    is refused by unitig_map_begin, which leaves the handle usable"""
    k, genome, km, cnt, strs, recs, reads, rows, hits, t = X.planted_case(name)
    m = KModel(1, 1023, NH, NB)
    compare(m, name, k, strs, recs, rows, hits, t)
    ubuf, uoff, urec, loff, lk = flat_input(strs, recs, rows)
    packed = U.pack(km, k)
    m.unitig_map_begin(packed, k, ubuf, uoff)
    ct, res, through = m.resolved_contigs_from_walks(k, ubuf, uoff, loff, lk, list(reads), 0, 0, 2, 0, 1, 0, urec)
    assert through.tolist() == list(t)
    want = X.resolve(k, strs, recs, rows, hits, t, 2, 0)
    exp = G.contigs(k, want["rstrs"], want["rrecs"], want["rrows"], want["rlink_hits"], 1, 0)
    for a, b in zip(ct[:8], G.flat(exp)[:8]):
        assert np.asarray(a).tobytes() == b.tobytes()
    if want["stats"]["n_resolved"] and k > 5:
        assert len(ct[2]) == 1 and len(ct[0]) in (len(genome) - 1, len(genome) - 2)
        s = ct[0].tobytes().decode()
        assert s in genome or U.rc(s) in genome
        with pytest.raises(KmxError) as e:                       # consequence (c): a k-mer of the resolved unitig appears p times
            m.unitig_map_begin(packed, k, res[0], res[1])
        assert e.value.code == -1
        m.unitig_map_begin(packed, k, ubuf, uoff)                # the handle is usable
        assert m.through_from_walks(list(reads), loff, lk, 0, 0)[0].tolist() == list(t)
    m.unitig_map_end()


@pytest.mark.parametrize("length", X.GEOMETRY_LENGTHS)
def test_emit_geometry(length):
    """one resolved unitig with four copies behind a neighbour whose length shifts every alignment class: copies straddle emit tiles
    and 16-byte words"""
    m = KModel(1, 1023, NH, NB)
    for shift in range(16):
        k, strs, rows, t = X.geometry_case(length, shift)
        compare(m, f"geometry {length} +{shift}", k, strs, None, rows, None, t, ((2, 0),))


def raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, t, pair, rec_cap, seq_cap, sizing=False):
    """one kmx_unitig_resolve_dev call on output buffers longer than it is told, filled with guard bytes -> (rc, counts, stats, outputs as
    numpy, whether every guard band and every input is intact)"""
    import torch
    nu, nl = len(uoff) - 1, len(lk)
    sizes = (seq_cap, (rec_cap + 1) * 8, rec_cap * 40, rec_cap * 4, nu * 8, (2 * rec_cap + 1) * 8, nl * 4, nl * 8, nl * 8)
    outs = [torch.full((s + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for s in sizes]
    ins = [to_dev(ubuf, np.uint8), to_dev(uoff, np.int64), to_dev(urec.view(np.uint8), np.uint8), to_dev(loff, np.int64), to_dev(lk, np.int32), to_dev(hits, np.int64), to_dev(t, np.int64)]
    before = [x.clone() for x in ins]
    st, n, b = ResolveStats(), C.c_uint64(0), C.c_uint64(0)
    par = ResolveParams(*pair)
    ptrs = [None] * 9 if sizing else [x.data_ptr() for x in outs]
    rc = m.L.kmx_unitig_resolve_dev(m.h, k, ins[0].data_ptr(), ins[1].data_ptr(), nu, len(ubuf), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), nl, ins[5].data_ptr(), ins[6].data_ptr(),
                                    C.byref(par), ptrs[0], seq_cap, ptrs[1], rec_cap, ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], ptrs[8], C.byref(n), C.byref(b), C.byref(st))
    torch.cuda.synchronize()
    host = [x.cpu().numpy() for x in outs]
    intact = all(np.all(h[s:] == 0xA5) for h, s in zip(host, sizes)) and all(torch.equal(x, y) for x, y in zip(ins, before))
    return rc, (n.value, b.value), st.as_dict(), host, sizes, intact


def good_case():
    name = "k31_tangle"
    k, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    ubuf, uoff, urec, loff, lk = flat_input(strs, recs, rows)
    hits = np.array(G.hits_of(name, "exact"), dtype=np.uint64)
    t = np.array(X.synthetic_case(name), dtype=np.uint64)
    exp = X.flat(X.resolve(k, strs, recs, rows, hits.tolist(), t.tolist(), 2, 1))
    return k, ubuf, uoff, urec, loff, lk, hits, t, exp


def check_raw(host, sizes, counts, st, exp):
    n, b = counts
    assert counts == tuple(int(x) for x in exp[10]) and stats_array(st).tobytes() == exp[9].tobytes()
    cut = (b, (n + 1) * 8, n * 40, n * 4, sizes[4], (2 * n + 1) * 8, sizes[6], sizes[7], sizes[8])
    for h, c, e, part in zip(host, cut, exp, X.PARTS):
        assert h[:c].tobytes() == e.tobytes(), part


def test_sizing_call_and_short_capacities():
    """the sizing call writes the two counts and the stats and nothing else; a capacity too small is KMX_E_RANGE with both counts set and
    nothing written, whichever of the two is short; the exact capacities then give the right bytes"""
    k, ubuf, uoff, urec, loff, lk, hits, t, exp = good_case()
    m = KModel(1, 1023, NH, NB)
    n, b = (int(x) for x in exp[10])
    assert n > len(uoff) - 1
    rc, counts, st, host, sizes, intact = raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, t, (2, 1), n, b, sizing=True)
    assert rc == 0 and counts == (n, b) and intact and all(np.all(h == 0xA5) for h in host) and stats_array(st).tobytes() == exp[9].tobytes()
    for rec_cap, seq_cap in ((n - 1, b), (n, b - 1), (0, 0), (len(uoff) - 1, len(ubuf))):
        rc, counts, st, host, sizes, intact = raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, t, (2, 1), rec_cap, seq_cap)
        assert rc == -5 and counts == (n, b) and intact and all(np.all(h == 0xA5) for h in host), (rec_cap, seq_cap)
    for rec_cap, seq_cap in ((n, b), (4 * (len(uoff) - 1), 4 * len(ubuf))):
        rc, counts, st, host, sizes, intact = raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, t, (2, 1), rec_cap, seq_cap)
        assert rc == 0 and intact
        check_raw(host, sizes, counts, st, exp)
    inp = (ubuf, uoff, urec, loff, lk)
    with pytest.raises(KmxError) as e:
        run_host(m, k, inp, hits, t, (2, 1), (n - 1, b))
    assert e.value.code == -5
    with pytest.raises(KmxError) as e:
        run_host(m, k, inp, hits, t, (2, 1), (n, b - 1))
    assert e.value.code == -5
    same(run_host(m, k, inp, hits, t, (2, 1), (n + 3, b + 5)), exp, "host, roomy capacities")


def raw_host(m, k, ubuf, uoff, urec, loff, lk, hits, t, par, swap=()):
    """one kmx_unitig_resolve call on freshly allocated outputs of 4 U and 4 n_ubases -> rc; swap replaces an argument by name"""
    nu, nl = len(uoff) - 1, len(lk)
    a = {"k": k, "useq": ubuf.ctypes.data, "uoffsets": uoff.ctypes.data, "n_unitigs": nu, "urec": urec.ctypes.data, "link_offsets": loff.ctypes.data, "links": lk.ctypes.data, "n_links": nl,
         "link_hits": hits.ctypes.data, "through": t.ctypes.data, "params": C.byref(par), "seq_capacity": 4 * len(ubuf), "rec_capacity": 4 * nu}
    keep = [np.zeros(4 * len(ubuf), np.uint8), np.zeros(4 * nu + 1, np.uint64), np.zeros(4 * nu, UNITIG_DTYPE), np.zeros(4 * nu, np.uint32), np.zeros(nu, RESOLVE_PLACE_DTYPE),
            np.zeros(8 * nu + 1, np.uint64), np.zeros(nl, np.uint32), np.zeros(nl, np.uint64), np.zeros(nl, np.uint64)]
    names = ("rseq", "roffsets", "rrec", "origin", "rplace", "rlink_offsets", "rlinks", "link_origin", "rlink_hits")
    for name_, arr in zip(names, keep):
        a[name_] = arr.ctypes.data
    st, n, b = ResolveStats(), C.c_uint64(0), C.c_uint64(0)
    a.update(n_unitigs_out=C.byref(n), n_bases_out=C.byref(b), stats=C.byref(st))
    a.update(dict(swap))
    return m.L.kmx_unitig_resolve(m.h, a["k"], a["useq"], a["uoffsets"], a["n_unitigs"], a["urec"], a["link_offsets"], a["links"], a["n_links"], a["link_hits"], a["through"], a["params"], a["rseq"],
                                  a["seq_capacity"], a["roffsets"], a["rec_capacity"], a["rrec"], a["origin"], a["rplace"], a["rlink_offsets"], a["rlinks"], a["link_origin"], a["rlink_hits"],
                                  a["n_unitigs_out"], a["n_bases_out"], a["stats"])


def test_refusals_and_no_unitigs():
    """every KMX_E_ARG of the header, each leaving the handle usable; U == 0"""
    import torch
    k, ubuf, uoff, urec, loff, lk, hits, t, exp = good_case()
    m = KModel(1, 1023, NH, NB)
    nu = len(uoff) - 1
    args = (m, k, ubuf, uoff, urec, loff, lk, hits, t)
    good = ResolveParams(2, 1)
    assert raw_host(*args, good) == 0
    for bad_k in (4, 22, 3, 65, 64):
        assert raw_host(*args, good, {"k": bad_k}) == -1
    assert raw_host(*args, good, {"n_unitigs": 2 ** 31}) == -1
    for gone in ("useq", "uoffsets", "link_offsets", "links", "through", "params", "roffsets", "origin", "rplace", "rlink_offsets", "rlinks", "link_origin", "n_unitigs_out", "n_bases_out", "stats",
                 "urec", "rrec", "link_hits", "rlink_hits"):                 # the last four: one of a pair that goes together
        assert raw_host(*args, good, {gone: None}) == -1, gone
    assert raw_host(*args, good, {"urec": None, "rrec": None}) == 0 and raw_host(*args, good, {"link_hits": None, "rlink_hits": None}) == 0
    assert raw_host(*args, good, {"rseq": ubuf.ctypes.data}) == -1 and raw_host(*args, good, {"link_origin": hits.ctypes.data}) == -1 and raw_host(*args, good, {"roffsets": uoff.ctypes.data + 8}) == -1
    first = uoff.copy()
    first[0] = 1
    dec = uoff.copy()
    dec[2], dec[3] = uoff[3], uoff[2]
    short = np.array([0, k - 1] + [int(x) for x in uoff[2:]], dtype=np.uint64)
    for bad in (first, dec, short):
        assert raw_host(m, k, ubuf, bad, urec, loff, lk, hits, t, good) == -1
    lo_first = loff.copy()
    lo_first[0] = 1
    lo_dec = loff.copy()
    lo_dec[3], lo_dec[4] = loff[4] + 1, loff[3]
    lo_short = loff.copy()
    lo_short[-1] -= 1
    lo_row5 = loff.copy()
    o = 0
    while int(loff[o + 3]) - int(loff[o]) < 5:
        o += 1
    lo_row5[o + 1] = lo_row5[o + 2] = loff[o + 3]
    for bad in (lo_first, lo_dec, lo_short, lo_row5):
        assert raw_host(m, k, ubuf, uoff, urec, bad, lk, hits, t, good) == -1
    bad_lk = lk.copy()
    bad_lk[len(lk) // 2] = 2 * nu
    no_mirror = lk.copy()
    rows = L.rows_of(loff, lk)
    a = next(x for x, row in enumerate(rows) if row and row[0] != x and row[0] != x ^ 1 and (x ^ 1) not in row)
    no_mirror[int(loff[a])] = a ^ 1
    for bad in (bad_lk, no_mirror):
        assert raw_host(m, k, ubuf, uoff, urec, loff, bad, hits, t, good) == -1
    # the through call: walks that do not tile the steps, a CSR the walks would refuse, NULL
    name = "k31_tangle"
    walks, _, steps, _, _ = X.listed_walks(name, "exact")
    w, _, s, _, _ = W.flat(walks, [0], steps, [], dict.fromkeys(W.STAT_FIELDS, 0))
    st = ThroughStats()
    out = np.zeros(16 * nu, dtype=np.uint64)
    call = lambda ww, ss, ns, lo, ll, th=out, stp=C.byref(st), U_=nu: m.L.kmx_unitig_walk_through(m.h, ww.ctypes.data if ww is not None else None, len(w), ss.ctypes.data if ss is not None else None,
                                                                                                  ns, lo.ctypes.data if lo is not None else None, ll.ctypes.data if ll is not None else None, len(lk), U_,
                                                                                                  th.ctypes.data if th is not None else None, stp)
    assert call(w, s, len(s), loff, lk) == 0 and out.tolist() == list(X.listed_through(name, "exact")[0])
    w1 = w.copy()
    w1["first_step"][0] = 1
    w2 = w.copy()
    w2["n_steps"][len(w) // 2] += 1
    for bad_w in (w1, w2):
        assert call(bad_w, s, len(s), loff, lk) == -1
    assert call(w, s, len(s) - 1, loff, lk) == -1 and call(w, s, len(s) + 1, loff, lk) == -1
    for bad in (lo_first, lo_dec, lo_short):
        assert call(w, s, len(s), bad, lk) == -1
    assert call(w, s, len(s), loff, bad_lk) == -1
    assert call(None, s, len(s), loff, lk) == -1 and call(w, None, len(s), loff, lk) == -1 and call(w, s, len(s), None, lk) == -1 and call(w, s, len(s), loff, None) == -1
    assert call(w, s, len(s), loff, lk, th=None) == -1 and call(w, s, len(s), loff, lk, stp=None) == -1 and call(w, s, len(s), loff, lk, U_=2 ** 31) == -1
    assert out.tolist() == list(X.listed_through(name, "exact")[0]), "a refused call adds nothing"
    # U == 0
    z64, ro, rlo = np.zeros(1, dtype=np.uint64), np.full(1, 7, dtype=np.uint64), np.full(1, 7, dtype=np.uint64)
    rs, n, b = ResolveStats(), C.c_uint64(9), C.c_uint64(9)
    rs.n_candidates = 5
    one = np.zeros(1, dtype=np.uint8)
    rc = m.L.kmx_unitig_resolve(m.h, 21, None, z64.ctypes.data, 0, None, z64.ctypes.data, None, 0, None, None, C.byref(good), one.ctypes.data, 0, ro.ctypes.data, 0, None, None, None, rlo.ctypes.data, None,
                                None, None, C.byref(n), C.byref(b), C.byref(rs))
    assert rc == 0 and ro[0] == rlo[0] == 0 and (n.value, b.value) == (0, 0) and not any(rs.as_dict().values())
    d_z, d_ro, d_rlo, d_one = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    n.value = 9
    rc = m.L.kmx_unitig_resolve_dev(m.h, 21, None, d_z.data_ptr(), 0, 0, None, d_z.data_ptr(), None, 0, None, None, C.byref(good), d_one.data_ptr(), 0, d_ro.data_ptr(), 0, None, None, None, d_rlo.data_ptr(),
                                    None, None, None, C.byref(n), C.byref(b), C.byref(rs))
    torch.cuda.synchronize()
    assert rc == 0 and d_ro.item() == d_rlo.item() == 0 and n.value == 0
    st.n_added = 3
    assert m.L.kmx_unitig_walk_through(m.h, None, 0, None, 0, z64.ctypes.data, None, 0, 0, None, C.byref(st)) == 0 and st.n_added == 0
    same(run_host(m, k, (ubuf, uoff, urec, loff, lk), hits, t, (2, 1)), exp, "host, after the refusals")
    same(run_dev(m, k, (ubuf, uoff, urec, loff, lk), hits, t, (2, 1)), exp, "device, after the refusals")


def test_crafted_device_input_stays_inside_the_buffers():
    """the _dev forms clamp: an asymmetric CSR, targets >= 2 U, rows of 6, bad row bounds and uoffsets, through cells of 2^64 - 1;
    first_step beyond n_steps and steps >= 2 U for the through hits: KMX_OK, wrong output, every guard band and every input intact,
    the call ends; the good input then gives the right bytes"""
    import torch
    k, ubuf, uoff, urec, loff, lk, hits, t, exp = good_case()
    m = KModel(1, 1023, NH, NB)
    nu, nl, big = len(uoff) - 1, len(lk), np.uint64(2 ** 64 - 1)
    r = np.random.RandomState(7)
    asym = lk.copy()
    asym[::3] = r.randint(0, 2 * nu, len(asym[::3]))
    beyond = lk.copy()
    beyond[1::4] = 2 * nu + r.randint(0, 5, len(beyond[1::4]))
    beyond[2::4] = 0xFFFFFFFF
    row6 = loff.copy()
    row6[1:2 * nu] = np.minimum(np.arange(1, 2 * nu, dtype=np.uint64) * np.uint64(6), np.uint64(nl))
    bad_links = [asym, beyond, np.full(nl, 0, np.uint32), np.full(nl, 1, np.uint32)]
    bad_loff = [row6, loff + np.uint64(nl), loff[::-1].copy(), np.full(len(loff), big), np.where(np.arange(len(loff)) % 2 == 1, big, loff)]
    bad_uoff = [uoff[::-1].copy(), np.full(nu + 1, big), np.zeros(nu + 1, np.uint64), np.where(np.arange(nu + 1) % 2 == 1, big, uoff), uoff + np.uint64(len(ubuf) // 2),
                np.arange(nu + 1, dtype=np.uint64) * np.uint64(3)]
    huge = np.full(16 * nu, big)
    perm = np.tile(np.array([big, 0, 0, 0, 0, big, 0, 0, 0, 0, big, 0, 0, 0, 0, big], dtype=np.uint64), nu)     # every candidate resolved
    crafted = ([(uoff, loff, x, t) for x in bad_links] + [(uoff, x, lk, t) for x in bad_loff] + [(x, loff, lk, t) for x in bad_uoff] +
               [(uoff, loff, lk, huge), (uoff, loff, lk, perm), (uoff, loff, asym, perm), (uoff, row6, beyond, perm), (bad_uoff[0], bad_loff[2], asym, perm), (bad_uoff[3], row6, lk, perm)])
    for uo, lo, links, th in crafted:
        # crafted uoffsets let unitigs overlap, so the bytes can exceed 4 n_ubases: room for 4 copies of U unitigs of n_ubases bytes
        rc, counts, st, host, sizes, intact = raw_dev(m, k, ubuf, uo, urec, lo, links, hits, th, (2, 1), 4 * nu, 4 * nu * len(ubuf))
        assert rc == 0 and intact and counts[0] <= 4 * nu and counts[1] <= 4 * nu * len(ubuf)
        assert st["n_candidates"] == st["n_resolved"] + st["n_crossed"] + st["n_unsupported"] + st["n_ambiguous"]
    rc, counts, st, host, sizes, intact = raw_dev(m, k, ubuf, uoff, urec, loff, lk, hits, t, (2, 1), 4 * nu, 4 * len(ubuf))
    assert rc == 0 and intact
    check_raw(host, sizes, counts, st, exp)
    # the through hits
    name = "k31_tangle"
    kk, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    walks, _, steps, _, _ = X.listed_walks(name, "exact")
    w, _, s, _, _ = W.flat(walks, [0], steps, [], dict.fromkeys(W.STAT_FIELDS, 0))
    far = w.copy()
    far["first_step"][::2] = np.uint64(len(s)) + np.arange(len(far["first_step"][::2]), dtype=np.uint64) * np.uint64(2 ** 40)
    none = w.copy()
    none["first_step"][:] = big
    wild = s.copy()
    wild[::5] = 2 * nu + r.randint(0, 3, len(wild[::5]))
    wild[1::7] = 0xFFFFFFFF

    def through_raw(ww, ss, lo, links):
        d_out = torch.full((16 * nu * 8 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        d_out[GUARD:GUARD + 16 * nu * 8] = 0
        ins = [to_dev(ww.view(np.uint8), np.uint8), to_dev(ss, np.int32), to_dev(lo, np.int64), to_dev(links, np.int32)]
        before = [x.clone() for x in ins]
        st = ThroughStats()
        rc = m.L.kmx_unitig_walk_through_dev(m.h, ins[0].data_ptr(), len(ww), ins[1].data_ptr(), len(ss), ins[2].data_ptr(), ins[3].data_ptr(), len(links), nu, d_out.data_ptr() + GUARD, C.byref(st))
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        ok = np.all(h[:GUARD] == 0xA5) and np.all(h[GUARD + 16 * nu * 8:] == 0xA5) and all(torch.equal(x, y) for x, y in zip(ins, before))
        return rc, st.as_dict(), h[GUARD:GUARD + 16 * nu * 8].view(np.uint64), ok

    for ww, ss, lo, links in [(far, s, loff, lk), (none, s, loff, lk), (w, wild, loff, lk), (w, s, loff, asym), (w, s, loff, beyond), (w, s, row6, lk), (far, wild, bad_loff[2], asym)] + \
                             [(w, s, x, lk) for x in bad_loff]:
        rc, st, got, ok = through_raw(ww, ss, lo, links)
        assert rc == 0 and ok and st["n_interior"] == st["n_added"] + st["n_missing"] == int(got.sum()) + st["n_missing"]
    rc, st, got, ok = through_raw(w, wild, loff, lk)
    assert st["n_missing"] > 0
    rc, st, got, ok = through_raw(w, s, loff, lk)
    assert rc == 0 and ok and got.tolist() == list(X.listed_through(name, "exact")[0]) and st == X.listed_through(name, "exact")[1]


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first call in turn, both calls, host and device form: the same call then succeeds with the
    right bytes"""
    k, ubuf, uoff, urec, loff, lk, hits, t, exp = good_case()
    inp = (ubuf, uoff, urec, loff, lk)
    name = "k31_tangle"
    kk, km, cnt, thr, strs, recs, reads, rows = G.listed_case(name)
    walks, _, steps, _, _ = X.listed_walks(name, "exact")
    want_t = list(X.listed_through(name, "exact")[0])
    failed = {"host": 0, "dev": 0, "through host": 0, "through dev": 0}
    for nth in range(1, 26):
        for variant in failed:
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            if variant == "host":
                run = lambda: same(run_host(m, k, inp, hits, t, (2, 1), (int(exp[10][0]), int(exp[10][1]))), exp, f"after allocation {nth} failed, host")
            elif variant == "dev":
                run = lambda: same(run_dev(m, k, inp, hits, t, (2, 1)), exp, f"after allocation {nth} failed, device")
            elif variant == "through host":
                run = lambda: through_host(m, walks, steps, rows)[0].tolist() == want_t or pytest.fail("through, host")
            else:
                run = lambda: through_dev(m, walks, steps, rows)[0].cpu().numpy().view(np.uint64).tolist() == want_t or pytest.fail("through, device")
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run()
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            run()
    assert failed["host"] >= 12 and failed["dev"] >= 6 and failed["through host"] >= 7 and failed["through dev"] >= 2, failed


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_resolve.cpp prints what unitig_through and unitig_resolve return on the 3 x 40 planted case, with the resolved
    table and the contigs of the resolved graph; the driver's -u1 -M -W0 -X1 -R2 on the 2 x 40 case writes a contigs.fa with the one
    contig and unitigs.resolved.tsv: all equal the restatement's text; -R without -X is refused with a message"""
    import os
    import subprocess
    import count_reads as CR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(root, "include"), os.path.join(root, source),
                               "-L" + os.path.join(root, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(root, "kmcex_amd"), "-o", exe])
        return exe

    def files(name):
        k, genome, km, cnt, strs, recs, reads, rows, hits, t = X.planted_case(name)
        fa, lines = str(tmp_path / f"{name}.fa"), str(tmp_path / f"{name}.txt")
        CR.write_fasta(fa, [r.encode() for r in reads])
        with open(lines, "w") as f:
            f.write("".join(r + "\n" for r in reads))
        res = X.resolve(k, strs, recs, rows, hits, t, 2, 0)
        return k, genome, strs, recs, rows, hits, t, fa, lines, res, G.contigs(k, res["rstrs"], res["rrecs"], res["rrows"], res["rlink_hits"], 1, 0)

    k, genome, strs, recs, rows, hits, t, fa, lines, res, ct = files("k21_3x40")
    out = subprocess.check_output([build("tests/facade_unitig_resolve.cpp", "facade_unitig_resolve"), fa, str(k), "1", lines, "0", "0", "2", "0"], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 7
    assert blocks[0] == "".join(f"{x}\n" for x in t)
    assert blocks[1] == "".join(f"{s} {u} {r['n_pred']} {r['n_succ']} {r['sum_count']}\n" for s, u, r in zip(res["rstrs"], res["origin"], res["rrecs"]))
    assert blocks[2] == "".join(f"{f} {n}\n" for f, n in res["rplace"])
    assert blocks[3] == "".join(f"{x}\n" for x in G.offsets_of(res["rrows"])) + "".join(f"{b} {e} {h}\n" for b, e, h in zip([b for row in res["rrows"] for b in row], res["link_origin"], res["rlink_hits"]))
    walks, _, steps, _, _ = W.walk_segs(k, strs, *R.map_reads(X.planted_case("k21_3x40")[2], k, strs, X.planted_case("k21_3x40")[6])[:2], rows, 0, 0)
    tst = X.through(walks, steps, rows, len(strs))[1]
    assert blocks[4] == " ".join(str(tst[f]) for f in X.THROUGH_STAT_FIELDS) + "\n" + " ".join(str(res["stats"][f]) for f in X.RESOLVE_STAT_FIELDS) + "\n"
    assert blocks[5] == X.resolved_tsv(res) and blocks[6] == G.fasta(ct) and res["stats"]["n_resolved"] == 1 and len(ct["cstrs"]) == 1
    k, genome, strs, recs, rows, hits, t, fa, lines, res, ct = files("k21_2x40")
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    work = tmp_path / "work"
    work.mkdir()
    log = subprocess.check_output([exe, "-g", "-u1", "-M", "-W0", "-X1", "-R2", f"-k{k}", "-nh3", "-nb2", fa, "db", str(work)], timeout=120).decode()
    got = (work / "db" / "contigs.fa").read_text()
    assert got == G.fasta(ct) and len(ct["cstrs"]) == 1 and (ct["cstrs"][0] in genome or U.rc(ct["cstrs"][0]) in genome) and len(ct["cstrs"][0]) == 529
    assert (work / "db" / "unitigs.resolved.tsv").read_text() == X.resolved_tsv(res) and "1 of 1 candidates" in log
    assert (work / "db" / "unitigs.fa").read_text().count(">") == len(strs)       # the unresolved graph
    refused = subprocess.run([exe, "-g", "-u1", "-M", "-W0", "-R2", f"-k{k}", fa, "db", str(work)], stdout=subprocess.PIPE)     # -R without -X
    assert refused.returncode == 2 and b"-R needs -M -W -X" in refused.stdout
