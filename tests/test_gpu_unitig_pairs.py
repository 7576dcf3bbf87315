"""kmx_unitig_pair_walks* on the MI355X: the records, the list of pair links, hist, pair_hits and the stats equal, byte for byte, what
the plain-Python restatement of the rule (tests/unitig_pairs_ref.py) gives, for the host and the device form: on the two cases from
reads through the live session (map, walks and pairs from the library), on the second one mapped onto its contigs, with the mates
swapped and a batch cut, and on crafted walk arrays that reach what real reads do not; KMX_E_RANGE, the refusals, the call outside a
session, allocation failures, crafted device input between guard bands, the facade."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pairs_ref as P
import unitig_walk_ref as W
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import PAIR_DTYPE, PAIR_LINK_DTYPE, WALK_DTYPE, KmxError, PairParams, PairStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the pairs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def begin(m, how, km, k, strs):
    import torch
    packed = U.pack(km, k)
    if how == "host":
        m.unitig_map_begin(packed, k, *R.join(strs))
    else:
        buf, off = R.join(strs)
        d_km = torch.from_numpy(np.ascontiguousarray(packed).view(np.int64).reshape(-1)).cuda()
        m.unitig_map_begin_dev(d_km, k, torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda())


def same(got, exp, what=""):
    for a, b, part in zip(got, exp, P.PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"


def stats_array(st):
    return np.array([st[f] for f in P.STAT_FIELDS], dtype=np.uint64)


def flat_walks(walks, wo, steps):
    w = np.zeros(len(walks), dtype=WALK_DTYPE)
    for i, g in enumerate(walks):
        for f, v in g.items():
            w[f][i] = v
    return w, np.array(wo, dtype=np.uint64), np.array(steps, dtype=np.uint32)


def run_host(m, fw, loff, lk, params, plinks=None):
    """-> the five parts, from kmx_unitig_pair_walks on flat walks; plinks: the flat list earlier batches left"""
    hist, hits = np.zeros(params[3], dtype=np.uint64), np.zeros(len(lk), dtype=np.uint64)
    rec, lst, st = m.unitig_pairs_flat(*fw, loff, lk, params[1], params[0], params[2], params[3], plinks=plinks, hist=hist, pair_hits=hits)
    return rec, lst, hist, hits, stats_array(st)


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def dev_walks(fw):
    """flat walks as the tensors unitig_walks_dev leaves: (d_walks uint8 [n, 80], n_walks, d_walk_offsets, d_steps, n_steps)"""
    w, wo, steps = fw
    return to_dev(w.view(np.uint8).reshape(-1, 80)) if len(w) else None, len(w), to_dev(wo, np.int64), to_dev(steps, np.int32) if len(steps) else None, len(steps)


def run_dev(m, dw, d_lo, d_lk, params, plinks=None, capacity=None):
    """-> the five parts, from kmx_unitig_pair_walks_dev on device walks"""
    import torch
    d_walks, nw, d_wo, d_steps, ns = dw
    n_pairs, n_in = (d_wo.numel() - 1) // 2, 0 if plinks is None else len(plinks)
    cap = n_in + n_pairs if capacity is None else capacity
    d_pairs = torch.zeros((max(n_pairs, 1), 64), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(params[3], dtype=torch.int64, device="cuda")
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    d_pl = torch.zeros((max(cap, 1), 32), dtype=torch.uint8, device="cuda")
    if n_in:
        d_pl[:n_in] = to_dev(plinks.view(np.uint8).reshape(-1, 32))
    st, n = m.unitig_pairs_dev(d_walks, nw, d_wo, d_steps, ns, d_lo, d_lk, params[1], params[0], params[2], params[3], d_pairs, d_hist, d_hits, d_pl, n_in)
    torch.cuda.synchronize()
    return (d_pairs.cpu().numpy()[:n_pairs].reshape(-1).view(PAIR_DTYPE), d_pl.cpu().numpy()[:n].reshape(-1).view(PAIR_LINK_DTYPE), d_hist.cpu().numpy().view(np.uint64),
            d_hits.cpu().numpy().view(np.uint64)[:d_lk.numel()], stats_array(st))


def dev_csr(loff, lk):
    return to_dev(loff, np.int64), to_dev(lk if len(lk) else np.zeros(0, np.uint32), np.int32)


# ---- the two cases from reads, through the live session
@functools.lru_cache(maxsize=None)
def read_ref(name):
    k, km, cnt, strs, reads, rows, genome = P.case(name)
    walks, wo, steps = P.walked(name)
    mu = [len(s) - k + 1 for s in strs]
    return P.flat(*P.pair_walks(k, mu, walks, wo, steps, rows, *P.READ_PARAMS))


@pytest.mark.parametrize("name", P.READ_CASES)
def test_reads_through_the_live_session(name):
    """map, walks and pairs from the library, host form after a host begin and device form after a device begin"""
    import torch
    k, km, cnt, strs, reads, rows, genome = P.case(name)
    loff, lk = L.flat_links(rows)
    exp = read_ref(name)
    mm, md, bw, nb = P.READ_PARAMS
    m = KModel(1, 1023, NH, NB)
    begin(m, "host", km, k, strs)
    hist, hits = np.zeros(nb, dtype=np.uint64), np.zeros(len(lk), dtype=np.uint64)
    rec, lst, st, walks, wo, steps = m.seq_to_pairs(reads, loff, lk, md, k, 0, mm, bw, nb, hist=hist, pair_hits=hits)
    same((rec, lst, hist, hits, stats_array(st)), exp, f"{name}: host")
    if name == "one_unitig":
        assert np.all(rec["cls"] == P.SAME) and np.all(rec["frag"] == 400) and np.all(rec["d"] == 221) and len(rec) == 2601
    else:
        link = rec[rec["cls"] == P.LINK]
        assert len(link) == 101 and np.all(link["edge"] == P.NO_EDGE) and np.all(221 - link["d"] == P.island_gap()) and len(lst) == 1 and lst["n_pairs"][0] == 101
        assert np.all(rec["cls"][rec["cls"] != P.LINK] == P.SAME)
    begin(m, "dev", km, k, strs)                                 # ends the first session
    buf, off = R.join(reads)
    d_seq, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    d_segs = torch.zeros((d_seq.numel(), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_seq, d_off, d_segs)
    d_lo, d_lk = dev_csr(loff, lk)
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    wst, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, k, 0, d_walks, d_steps)
    same(run_dev(m, (d_walks, wst["n_walks"], d_wo, d_steps, wst["n_steps"]), d_lo, d_lk, P.READ_PARAMS), exp, f"{name}: device")
    m.unitig_map_end()


def test_two_islands_mapped_onto_the_contigs():
    """the contigs kmx_unitig_contigs returns are a unitig set for the session and clink_offsets / clinks its CSR: the pairs across
    the gap link the two contigs at the same distance"""
    name = "two_islands"
    k, km, cnt, strs, reads, rows, genome = P.case(name)
    loff, lk = L.flat_links(rows)
    m = KModel(1, 1023, NH, NB)
    cseq, coffs, crec, csteps, place, cloffs, clinks, csup, cst = m.unitig_contigs_flat(k, *R.join(strs), loff, lk, np.zeros(len(lk), dtype=np.uint64), 1, 0)
    cstrs = [cseq[int(coffs[i]):int(coffs[i + 1])].tobytes().decode() for i in range(len(coffs) - 1)]
    crows = L.rows_of(cloffs, clinks)
    assert len(cstrs) == 2 and not any(crows)
    segs, so, _, _ = R.map_reads(km, k, cstrs, reads)
    walks, wo, steps, _, _ = W.walk_segs(k, cstrs, segs, so, crows, k, 0)
    exp = P.flat(*P.pair_walks(k, [len(s) - k + 1 for s in cstrs], walks, wo, steps, crows, *P.READ_PARAMS))
    assert len(exp[1]) == 1 and exp[1]["n_pairs"][0] == 101 and exp[1]["min_dist"][0] == exp[1]["max_dist"][0] == 221 - P.island_gap()
    mm, md, bw, nb = P.READ_PARAMS
    m.unitig_map_begin(U.pack(km, k), k, cseq, coffs)
    hist, hits = np.zeros(nb, dtype=np.uint64), np.zeros(len(clinks), dtype=np.uint64)
    rec, lst, st, _, _, _ = m.seq_to_pairs(reads, cloffs, clinks, md, k, 0, mm, bw, nb, hist=hist, pair_hits=hits)
    same((rec, lst, hist, hits, stats_array(st)), exp, "on the contigs")
    m.unitig_map_end()


# ---- crafted walk arrays on a session that holds the m_u they were made for
@functools.lru_cache(maxsize=None)
def craft_csr():
    return L.flat_links(P.craft_rows())


@functools.lru_cache(maxsize=None)
def craft_ref(n_pairs, params):
    k, km, strs, mu = P.craft_set()
    return P.flat(*P.pair_walks(k, mu, *P.crafted(n_pairs, 100 + n_pairs), P.craft_rows(), *params))


@pytest.fixture(scope="module")
def craft_model():
    """one session on the crafted unitig set for every test that only reads it"""
    k, km, strs, mu = P.craft_set()
    m = KModel(1, 1023, NH, NB)
    begin(m, "dev", km, k, strs)
    yield m
    m.unitig_map_end()


@pytest.mark.parametrize("n_pairs", P.CRAFT_SIZES)
def test_crafted_walks_equal_the_restatement(craft_model, n_pairs):
    """1, 255, 256, 257 and 513 pairs: reads with no walk, several walks and a tie, every walk below min_mapped; frag negative, in the
    last bin and beyond it, bin_width = 1 with n_bins = 1; keys of both orders, unitigs 0 and U - 1; a target in the fourth entry of
    a row; INVERTED; FAR"""
    m = craft_model
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    fw = flat_walks(*P.crafted(n_pairs, 100 + n_pairs))
    dw = dev_walks(fw)
    for params in P.CRAFT_PARAMS:
        exp = craft_ref(n_pairs, params)
        same(run_host(m, fw, loff, lk, params), exp, f"{n_pairs} pairs {params}: host")
        same(run_dev(m, dw, d_lo, d_lk, params), exp, f"{n_pairs} pairs {params}: device")
    if n_pairs >= 255:
        exp = craft_ref(n_pairs, P.CRAFT_PARAMS[0])
        assert set(exp[0]["cls"].tolist()) == set(range(6)) and exp[2][-1] > 0 and exp[4][4] > 0 and 0 < exp[4][7] < exp[4][6]


def test_far_at_max_dist_and_one_beyond(craft_model):
    m = craft_model
    loff, lk = craft_csr()
    k, km, strs, mu = P.craft_set()
    fw = flat_walks(*P.key_pairs([(6, 8)], [50]))
    for max_dist, cls in ((50, P.LINK), (49, P.FAR)):
        params = (1, max_dist, 1, 1)
        exp = P.flat(*P.pair_walks(k, mu, *P.key_pairs([(6, 8)], [50]), P.craft_rows(), *params))
        assert exp[0]["cls"][0] == cls and exp[0]["d"][0] == 50
        same(run_host(m, fw, loff, lk, params), exp, f"max_dist {max_dist}: host")
        same(run_dev(m, dev_walks(fw), *dev_csr(loff, lk), params), exp, f"max_dist {max_dist}: device")


def test_mates_swapped_and_batches_cut(craft_model):
    """consequences (a) and (c) on the library: the mates swapped give the same list, hist and stats and the mirrored pair_hits; a
    batch cut into two and into single pairs, merged into the same list, gives the bytes of one call"""
    m = craft_model
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    n_pairs, params = 257, P.CRAFT_PARAMS[0]
    walks, wo, steps = P.crafted(n_pairs, 100 + n_pairs)
    exp = craft_ref(n_pairs, params)
    sw, swo, order = P.swapped(walks, wo)
    want = P.flat(*P.pair_walks(k, mu, sw, swo, steps, rows, *params))
    for got in (run_host(m, flat_walks(sw, swo, steps), loff, lk, params), run_dev(m, dev_walks(flat_walks(sw, swo, steps)), d_lo, d_lk, params)):
        same(got, want, "mates swapped")
        assert got[1].tobytes() == exp[1].tobytes() and got[2].tobytes() == exp[2].tobytes() and got[4].tobytes() == exp[4].tobytes()
        assert got[3].tolist() == P.mirror_hits(rows, exp[3].tolist())
    for form, pieces in (("host", (100, n_pairs)), ("dev", (100, n_pairs)), ("dev", tuple(range(1, n_pairs + 1)))):
        lst, at = None, 0
        hist, hits, tot, recs = np.zeros(params[3], dtype=np.uint64), np.zeros(len(lk), dtype=np.uint64), np.zeros(10, dtype=np.uint64), []
        for end in pieces:
            cw, cwo = P.cut(walks, wo, at, end)
            fw = flat_walks(cw, cwo, steps)
            rec, lst, h, t, s = run_host(m, fw, loff, lk, params, lst) if form == "host" else run_dev(m, dev_walks(fw), d_lo, d_lk, params, lst)
            base = np.uint64(wo[2 * at])
            rec = rec.copy()
            for f in ("walk_a", "walk_b"):
                rec[f] = np.where(rec[f] == np.uint64(P.NO_WALK), rec[f], rec[f] + base)
            recs.append(rec)
            hist, hits, tot, at = hist + h, hits + t, tot + s, end
        same((np.concatenate(recs), lst, hist, hits, tot), exp, f"cut at {pieces[:3]}, {form}")


def test_merges_of_many_keys(craft_model):
    """5000 distinct keys plus 3000 repeats of them in one batch; then a merge where every new key is already in the list, and one
    where none is"""
    m = craft_model
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    params = (1, 2 ** 32 - 1, 10, 4)
    first, second = P.merge_case()
    r1 = P.pair_walks(k, mu, *first, rows, *params)
    e1 = P.flat(*r1)
    assert len(e1[1]) == 5000 and e1[4][6] == 8000
    f1, f2 = flat_walks(*first), flat_walks(*second)
    d1, d2 = dev_walks(f1), dev_walks(f2)
    same(run_host(m, f1, loff, lk, params), e1, "first batch: host")
    same(run_dev(m, d1, d_lo, d_lk, params), e1, "first batch: device")
    e11 = P.flat(*P.pair_walks(k, mu, *first, rows, *params, plinks=r1[1]))
    e12 = P.flat(*P.pair_walks(k, mu, *second, rows, *params, plinks=r1[1]))
    assert len(e11[1]) == 5000 and len(e12[1]) == 5700
    same(run_host(m, f1, loff, lk, params, e1[1]), e11, "every key is in the list: host")
    same(run_dev(m, d1, d_lo, d_lk, params, e1[1]), e11, "every key is in the list: device")
    same(run_host(m, f2, loff, lk, params, e1[1]), e12, "no key is in the list: host")
    same(run_dev(m, d2, d_lo, d_lk, params, e1[1]), e12, "no key is in the list: device")


def raw_dev(m, dw, d_lo, d_lk, n_links, params, plinks, capacity, n_seqs=None, give=(True, True, True, True)):
    """one kmx_unitig_pair_walks_dev call whose four outputs lie between guard bands of GUARD elements
    -> (rc, n_plinks, stats, pairs, list, hist, pair_hits: each the whole buffer with its bands, as uint8 rows or int64)"""
    import torch
    d_walks, nw, d_wo, d_steps, ns = dw
    n_seqs = d_wo.numel() - 1 if n_seqs is None else n_seqs
    n_pairs, n_in = n_seqs // 2, len(plinks)
    pairs = torch.full((n_pairs + 2 * GUARD, 64), 0xA5, dtype=torch.uint8, device="cuda")
    lst = torch.full((capacity + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    hist = torch.full((params[3] + 2 * GUARD,), -7, dtype=torch.int64, device="cuda")
    hits = torch.full((n_links + 2 * GUARD,), -7, dtype=torch.int64, device="cuda")
    hist[GUARD:GUARD + params[3]] = 0
    hits[GUARD:GUARD + n_links] = 0
    if n_in:
        lst[GUARD:GUARD + n_in] = to_dev(plinks.view(np.uint8).reshape(-1, 32))
    par, st, n = PairParams(*params), PairStats(), C.c_uint64(n_in)
    at = lambda t, rows: t[GUARD:].data_ptr() if rows is not None else None
    rc = m.L.kmx_unitig_pair_walks_dev(m.h, d_walks.data_ptr() if d_walks is not None else None, nw, d_wo.data_ptr(), n_seqs, d_steps.data_ptr() if d_steps is not None else None, ns,
                                       d_lo.data_ptr(), d_lk.data_ptr() if n_links else None, n_links, C.byref(par), at(pairs, give[0] or None), at(hist, give[1] or None),
                                       at(hits, give[2] or None), at(lst, give[3] or None), capacity, C.byref(n), C.byref(st))
    torch.cuda.synchronize()
    return rc, n.value, st.as_dict(), pairs.cpu().numpy(), lst.cpu().numpy(), hist.cpu().numpy(), hits.cpu().numpy()


def bands_intact(n_pairs, capacity, n_bins, n_links, pairs, lst, hist, hits):
    return (np.all(pairs[:GUARD] == 0xA5) and np.all(pairs[GUARD + n_pairs:] == 0xA5) and np.all(lst[:GUARD] == 0xA5) and np.all(lst[GUARD + capacity:] == 0xA5) and
            np.all(hist[:GUARD] == -7) and np.all(hist[GUARD + n_bins:] == -7) and np.all(hits[:GUARD] == -7) and np.all(hits[GUARD + n_links:] == -7))


def test_range_leaves_the_list_as_it_was(craft_model):
    """capacity = needed - 1: KMX_E_RANGE, the list's bytes as they were, *n_plinks the number needed, nothing written at or behind
    plinks[capacity]; records, stats, hist and pair_hits complete; then the repeat with hist = pair_hits = NULL succeeds"""
    m = craft_model
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    n_pairs, params = 513, P.CRAFT_PARAMS[0]
    walks, wo, steps = P.crafted(n_pairs, 100 + n_pairs)
    old_walks = P.crafted(257, 357)
    old = P.pair_walks(k, mu, *old_walks, rows, *params)[1]
    exp = P.flat(*P.pair_walks(k, mu, walks, wo, steps, rows, *params, plinks=old))
    fold, need = P.flat_list(old), len(exp[1])
    assert need > len(old) > 20
    fw = flat_walks(walks, wo, steps)
    dw = dev_walks(fw)
    rc, n, st, pairs, lst, hist, hits = raw_dev(m, dw, d_lo, d_lk, len(lk), params, fold, need - 1)
    assert rc == -5 and n == need and bands_intact(n_pairs, need - 1, params[3], len(lk), pairs, lst, hist, hits)
    assert lst[GUARD:GUARD + len(old)].tobytes() == fold.tobytes() and np.all(lst[GUARD + len(old):] == 0xA5)
    assert pairs[GUARD:GUARD + n_pairs].tobytes() == exp[0].tobytes() and stats_array(st).tobytes() == exp[4].tobytes()
    assert hist[GUARD:GUARD + params[3]].view(np.uint64).tobytes() == exp[2].tobytes() and hits[GUARD:GUARD + len(lk)].view(np.uint64).tobytes() == exp[3].tobytes()
    rc, n, st, pairs, lst, hist, hits = raw_dev(m, dw, d_lo, d_lk, len(lk), params, fold, need, give=(True, False, False, True))
    assert rc == 0 and n == need and lst[GUARD:GUARD + need].tobytes() == exp[1].tobytes() and bands_intact(n_pairs, need, params[3], len(lk), pairs, lst, hist, hits)
    assert not hist[GUARD:GUARD + params[3]].any() and not hits[GUARD:GUARD + len(lk)].any()
    # the host form
    h, t = np.zeros(params[3], dtype=np.uint64), np.zeros(len(lk), dtype=np.uint64)
    with pytest.raises(KmxError) as e:
        m.unitig_pairs_flat(*fw, loff, lk, params[1], params[0], params[2], params[3], plinks=fold, capacity=need - 1, hist=h, pair_hits=t)
    assert e.value.code == -5 and e.value.needed == need and h.tobytes() == exp[2].tobytes() and t.tobytes() == exp[3].tobytes()
    lst_h = np.zeros(need - 1, dtype=PAIR_LINK_DTYPE)
    lst_h[:len(old)] = fold
    lst_h[len(old):] = np.frombuffer(b"\xa5" * 32, dtype=PAIR_LINK_DTYPE)[0]
    before = lst_h.tobytes()
    par, pst, cnt = PairParams(*params), PairStats(), C.c_uint64(len(old))
    rc = m.L.kmx_unitig_pair_walks(m.h, fw[0].ctypes.data, len(fw[0]), fw[1].ctypes.data, 2 * n_pairs, fw[2].ctypes.data, len(fw[2]), loff.ctypes.data, lk.ctypes.data, len(lk), C.byref(par),
                                   None, None, None, lst_h.ctypes.data, need - 1, C.byref(cnt), C.byref(pst))
    assert rc == -5 and cnt.value == need and lst_h.tobytes() == before and stats_array(pst.as_dict()).tobytes() == exp[4].tobytes()
    rec, lst2, st2 = m.unitig_pairs_flat(*fw, loff, lk, params[1], params[0], params[2], params[3], plinks=fold, capacity=need)
    assert lst2.tobytes() == exp[1].tobytes() and rec.tobytes() == exp[0].tobytes()


def test_refusals_and_the_call_outside_a_session():
    """KMX_E_ARG before anything runs: an odd n_seqs, bin_width = 0, n_bins = 0 and 65537, a NULL required buffer, *n_plinks above
    the capacity, an output that overlaps an input; in the host form also bad walk_offsets, a bad CSR and a list that is not
    strictly ascending; KMX_E_STATE outside a session; n_seqs = 0 is KMX_OK with all-zero stats and the list untouched; the
    session then answers as if nothing had happened"""
    k, km, strs, mu = P.craft_set()
    rows = P.craft_rows()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    params = P.CRAFT_PARAMS[0]
    walks, wo, steps = P.crafted(255, 355)
    fw = flat_walks(walks, wo, steps)
    dw = dev_walks(fw)
    exp = craft_ref(255, params)
    m = KModel(1, 1023, NH, NB)
    with pytest.raises(KmxError) as e:
        m.unitig_pairs_flat(*fw, loff, lk, params[1], params[0], params[2], params[3])
    assert e.value.code == -4
    assert raw_dev(m, dw, d_lo, d_lk, len(lk), params, P.flat_list([]), 255)[0] == -4
    begin(m, "host", km, k, strs)
    lst = np.zeros(600, dtype=PAIR_LINK_DTYPE)

    def host_rc(par=params, w=fw[0], o=fw[1], s=fw[2], lo=loff, links=lk, n_seqs=None, n_in=0, cap=600, pl=lst, pairs=None, st=True):
        p, stt, n = PairParams(*par), PairStats(), C.c_uint64(n_in)
        ptr = lambda a: a.ctypes.data if a is not None else None
        return m.L.kmx_unitig_pair_walks(m.h, ptr(w), len(fw[0]), ptr(o), len(fw[1]) - 1 if n_seqs is None else n_seqs, ptr(s), len(fw[2]), ptr(lo), ptr(links),
                                         len(lk), C.byref(p), ptr(pairs), None, None, ptr(pl), cap, C.byref(n), C.byref(stt) if st else None)

    assert host_rc() == 0
    for bad in ((5, 120, 0, 12), (5, 120, 16, 0), (5, 120, 16, 65537)):
        assert host_rc(par=bad) == -1 and raw_dev(m, dw, d_lo, d_lk, len(lk), bad, P.flat_list([]), 255)[0] == -1
    assert host_rc(n_seqs=len(fw[1]) - 2) == -1 and raw_dev(m, dw, d_lo, d_lk, len(lk), params, P.flat_list([]), 255, n_seqs=509)[0] == -1
    assert host_rc(w=None) == -1 and host_rc(o=None) == -1 and host_rc(s=None) == -1 and host_rc(lo=None) == -1 and host_rc(links=None) == -1 and host_rc(st=False) == -1
    assert host_rc(n_in=601) == -1
    assert host_rc(pairs=fw[0].view(np.uint8)) == -1             # the records would overwrite the walks
    assert host_rc(pl=fw[2].view(np.uint8), cap=len(fw[2]) // 8) == -1
    swapped = fw[1].copy()
    swapped[3], swapped[4] = fw[1][4] + 1, fw[1][3]
    short = fw[1].copy()
    short[-1] -= 1
    above = fw[1].copy()
    above[0] = 1
    for bad in (swapped, short, above):
        assert host_rc(o=bad) == -1
    bad_lk = lk.copy()
    bad_lk[len(lk) // 2] = 2 * len(strs)
    bad_lo = loff.copy()
    bad_lo[3], bad_lo[4] = loff[4] + 1, loff[3]
    assert host_rc(links=bad_lk) == -1 and host_rc(lo=bad_lo) == -1
    for bad in ([(4, 9, 1, 1, 1, 1), (4, 9, 1, 1, 1, 1)], [(4, 9, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)], [(5, 0, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)]):
        pl = np.zeros(600, dtype=PAIR_LINK_DTYPE)
        pl[:2] = P.flat_list(bad)
        assert host_rc(pl=pl, n_in=2) == -1
    # n_seqs == 0: KMX_OK, all-zero stats, the list untouched
    pl = np.zeros(4, dtype=PAIR_LINK_DTYPE)
    pl[:2] = P.flat_list([(4, 8, 1, 1, 1, 1), (4, 9, 1, 1, 1, 1)])
    before = pl.tobytes()
    p, stt, n = PairParams(*params), PairStats(), C.c_uint64(2)
    stt.n_pairs = 9
    assert m.L.kmx_unitig_pair_walks(m.h, None, 0, None, 0, None, 0, None, None, 0, C.byref(p), None, None, None, pl.ctypes.data, 4, C.byref(n), C.byref(stt)) == 0
    assert n.value == 2 and pl.tobytes() == before and not any(stt.as_dict().values())
    same(run_host(m, fw, loff, lk, params), exp, "after the refusals: host")
    same(run_dev(m, dw, d_lo, d_lk, params), exp, "after the refusals: device")
    m.unitig_map_end()
    with pytest.raises(KmxError) as e:
        m.unitig_pairs_flat(*fw, loff, lk, params[1], params[0], params[2], params[3])
    assert e.value.code == -4


def test_allocation_failure_leaves_handle_and_session_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first pair call in turn, host and device form: the session stays open and the same call
    then succeeds with the right bytes"""
    k, km, strs, mu = P.craft_set()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    params = P.CRAFT_PARAMS[0]
    fw = flat_walks(*P.crafted(257, 357))
    dw = dev_walks(fw)
    exp = craft_ref(257, params)
    failed = {"host": 0, "dev": 0}
    for nth in range(1, 18):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            begin(m, variant, km, k, strs)
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run_host(m, fw, loff, lk, params) if variant == "host" else run_dev(m, dw, d_lo, d_lk, params)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run_host(m, fw, loff, lk, params) if variant == "host" else run_dev(m, dw, d_lo, d_lk, params), exp, f"after allocation {nth} failed, {variant}")
            m.unitig_map_end()
    assert failed["host"] >= 12 and failed["dev"] >= 6, failed


def test_crafted_device_input_stays_inside_the_buffers(craft_model):
    """the _dev form clamps: walk_offsets beyond n_walks, decreasing and all ones; first_step and n_steps that point beyond steps or
    wrap; steps >= 2 U; off_last >= m_u; rows longer than 4, row bounds beyond n_links and decreasing; an input list out of order:
    KMX_OK, wrong pairs, and the guard bands around pairs, the list, hist and pair_hits are intact"""
    m = craft_model
    k, km, strs, mu = P.craft_set()
    loff, lk = craft_csr()
    d_lo, d_lk = dev_csr(loff, lk)
    n_pairs, params = 513, (0, 2 ** 32 - 1, 3, 17)
    w, wo, steps = flat_walks(*P.crafted(n_pairs, 100 + n_pairs))
    nw, ns, nl, U2 = len(w), len(steps), len(lk), 2 * len(strs)
    big = np.uint64(2 ** 64 - 1)
    r = np.random.RandomState(9)

    def walks_with(**f):
        v = w.copy()
        for name, val in f.items():
            v[name] = val
        return v

    bad_walks = [walks_with(first_step=np.full(nw, big)), walks_with(first_step=w["first_step"] + np.uint64(ns)), walks_with(n_steps=np.full(nw, 0xFFFFFFFF, np.uint32)),
                 walks_with(first_step=np.full(nw, big - np.uint64(1)), n_steps=np.full(nw, 3, np.uint32)), walks_with(off_last=np.full(nw, 0xFFFFFFFF, np.uint32)),
                 walks_with(off_last=r.randint(0, 400, nw).astype(np.uint32), n_mapped=np.full(nw, big), n_span=np.full(nw, big))]
    bad_steps = [np.where(np.arange(ns) % 3 == 1, U2 + r.randint(0, 5, ns), steps).astype(np.uint32), np.full(ns, 0xFFFFFFFF, np.uint32)]
    bad_wo = [wo[::-1].copy(), wo + np.uint64(nw), np.full(len(wo), big), np.zeros(len(wo), np.uint64), np.where(np.arange(len(wo)) % 2 == 1, big, wo)]
    long_rows = np.zeros(len(loff), dtype=np.uint64)
    long_rows[1:] = np.minimum(np.arange(1, len(loff)) * 9, nl)                       # rows of 9 entries
    bad_lo = [loff + np.uint64(nl), loff[::-1].copy(), np.full(len(loff), big), np.where(np.arange(len(loff)) % 2 == 1, big, loff), long_rows]
    old = P.flat_list([(7, 9, 1, 5, 5, 5), (4, 8, 2, 9, 1, 8), (4, 8, 1, 1, 1, 1), (0xFFFFFFFF, 0xFFFFFFFF, 3, 3, 3, 3)])
    none = P.flat_list([])
    crafted = ([((v, wo, steps), d_lo, none) for v in bad_walks] + [((w, wo, s), d_lo, none) for s in bad_steps] + [((w, o, steps), d_lo, none) for o in bad_wo] +
               [((w, wo, steps), to_dev(x, np.int64), none) for x in bad_lo] + [((w, wo, steps), d_lo, old), ((bad_walks[5], bad_wo[0], bad_steps[0]), to_dev(bad_lo[3], np.int64), old)])
    cap = n_pairs + len(old)
    for fw, lo, lst_in in crafted:
        rc, n, st, pairs, lst, hist, hits = raw_dev(m, dev_walks(fw), lo, d_lk, nl, params, lst_in, cap)
        assert rc == 0 and n <= cap and st["n_pairs"] == n_pairs
        assert st["n_none"] + st["n_single"] + st["n_same"] + st["n_inverted"] + st["n_link"] + st["n_far"] == n_pairs
        assert bands_intact(n_pairs, cap, params[3], nl, pairs, lst, hist, hits)
        assert np.all(lst[GUARD + max(n, len(lst_in)):] == 0xA5)    # a list that folds to fewer entries leaves its old tail behind them
    exp = craft_ref(n_pairs, params)
    rc, n, st, pairs, lst, hist, hits = raw_dev(m, dev_walks((w, wo, steps)), d_lo, d_lk, nl, params, none, cap)
    assert rc == 0 and pairs[GUARD:GUARD + n_pairs].tobytes() == exp[0].tobytes() and lst[GUARD:GUARD + n].tobytes() == exp[1].tobytes()


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_pairs.cpp prints what seq_pairs returns for the two islands in two batches merged into one list, and the
    two tables; the driver's -u1 -M -W -P400 writes pairs.links.tsv and pairs.insert.tsv: all equal the restatement's text"""
    import count_reads as CR
    name = "two_islands"
    k, km, cnt, strs, reads, rows, genome = P.case(name)
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in reads])
    lines = str(tmp_path / "reads.txt")
    with open(lines, "w") as f:
        f.write("".join(r + "\n" for r in reads))

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    exe = build("tests/facade_unitig_pairs.cpp", "facade_unitig_pairs")
    mm, md, bw, nb = P.READ_PARAMS
    out = subprocess.check_output([exe, fa, str(k), "1", lines, str(mm), str(md), str(bw), str(nb)], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 5
    walks, wo, steps = P.walked(name)
    pairs, plinks, hist, hits, st = P.pair_walks(k, [len(s) - k + 1 for s in strs], walks, wo, steps, rows, *P.READ_PARAMS)
    fp = P.flat(pairs, plinks, hist, hits, st)[0]
    assert blocks[0] == "".join(" ".join(str(int(r[f])) for f in P.PAIR_DTYPE.names) + "\n" for r in fp)
    assert blocks[1] == " ".join(str(st[f]) for f in P.STAT_FIELDS) + "\n"
    assert blocks[2] == P.links_tsv(plinks, rows) and blocks[3] == P.insert_tsv(hist, bw) and blocks[4] == "".join(f"{x}\n" for x in hits)
    # the driver places the pairs of its input at min_mapped = 1, bins of 10 bases up to 2000
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    pairs, plinks, hist, hits, st = P.pair_walks(k, [len(s) - k + 1 for s in strs], walks, wo, steps, rows, 1, md, 10, 200)
    log = subprocess.check_output([exe, "-g", "-u1", "-M", "-W", f"-P{md}", f"-k{k}", "-nh3", "-nb2", fa, "db", str(tmp_path)], timeout=120).decode()
    assert (tmp_path / "db" / "pairs.links.tsv").read_text() == P.links_tsv(plinks, rows) and (tmp_path / "db" / "pairs.insert.tsv").read_text() == P.insert_tsv(hist, 10)
    assert f"{st['n_pairs']} pairs: {st['n_same']} on one unitig (0 negative, median fragment 400), {st['n_link']} links (0 adjacent, 1 distinct)" in log
    assert subprocess.call([exe, "-g", "-u1", "-M", f"-P{md}", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2     # -P without -W
    odd = str(tmp_path / "odd.fa")
    CR.write_fasta(odd, [r.encode() for r in reads[:-1]])
    assert subprocess.call([exe, "-g", "-u1", "-M", "-W", "-P", f"-k{k}", "-nh3", "-nb2", odd, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 1   # an odd number of reads
