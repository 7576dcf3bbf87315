"""kmx_unitig_pair_lift* on the MI355X: the records, the lifted list, n_out and stats equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitig_pair_lift_ref.py) gives, for the host and the device form (the device form always between
guard bands) and for both fold kernels: lists at the block and wavefront edges of the per-entry kernels with every entry its own
key, one run of 513, runs that start and end around the wavefront and block edges, a run of mirrored entries, every class with the
wrapping sums, max_dist at both ends, lists only the device form takes, KMX_E_RANGE and the sizing call, the empty inputs, the
refusals, a handle used twice, the acceptance case (consequence (d) through the real calls, into kmx_unitig_scaffold_dev), the
facade and the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import unitig_contigs_ref as Cn
import unitig_map_ref as R
import unitig_pair_lift_ref as F
import unitig_pair_reduce_ref as X
import unitig_pairs_ref as P
import unitig_scaffold_ref as S
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import KmxError, PairLiftParams, PairLiftStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the list
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
K = 21
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
FOLDS = ("wave", "plain")


@pytest.fixture(scope="module")
def model():
    return KModel(1, 1023, NH, NB)


def offsets_of(mu, k=K):
    return np.cumsum([0] + [m + k - 1 for m in mu], dtype=np.uint64).astype(np.uint64)


def place_array(place):
    return np.array([tuple(p) for p in place], dtype=Cn.CONTIG_PLACE_DTYPE) if len(place) else np.zeros(0, dtype=Cn.CONTIG_PLACE_DTYPE)


def crec_array(cm):
    c = np.zeros(len(cm), dtype=Cn.CONTIG_DTYPE)
    c["n_kmers"] = np.array(cm, dtype=np.uint64)
    c["n_steps"] = 1
    return c


def same(got, exp, what):
    assert np.asarray(got[0]).tobytes() == exp[0].tobytes(), f"{what}: lrec differ"
    assert np.asarray(got[1]).tobytes() == exp[1].tobytes(), f"{what}: lout differ"
    assert got[2] == exp[2], f"{what}: n_out {got[2]} != {exp[2]}"
    st = [got[3][f] for f in F.STAT_FIELDS]
    assert st == exp[3], f"{what}: stats differ: {st} != {exp[3]}"


def run_host(m, case, max_dist, capacity=None, k=K):
    mu, place, cm, pl = case
    rec, lout, st = m.unitig_pair_lift_flat(k, offsets_of(mu, k), place_array(place), crec_array(cm), F.plinks_array(pl), max_dist, capacity=capacity)
    return rec, lout, len(lout), st


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def raw_dev(m, case, max_dist, cap, k=K, lists=True, n_ubases=None, n_contigs=None):
    """one kmx_unitig_pair_lift_dev call whose two outputs lie between guard bands of GUARD elements -> (rc, n_out, stats, the two
    outputs with their bands as NumPy arrays)"""
    import torch
    mu, place, cm, plinks = case
    off, pl = offsets_of(mu, k), F.plinks_array(plinks)
    n = len(pl)
    d_pl = to_dev(pl.view(np.uint8).reshape(-1, 32)) if n else None
    d_off = to_dev(off, np.int64)
    d_place = to_dev(place_array(place).view(np.uint8).reshape(-1, 8)) if len(mu) else None
    d_crec = to_dev(crec_array(cm).view(np.uint8).reshape(-1, 64)) if len(cm) else None
    lrec = torch.full((n + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    lout = torch.full((cap + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    p, st, no = PairLiftParams(max_dist, 0), PairLiftStats(), C.c_uint64(0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = m.L.kmx_unitig_pair_lift_dev(m.h, k, d_off.data_ptr(), len(mu), int(off[-1]) if n_ubases is None else n_ubases, ptr(d_place), ptr(d_crec), len(cm) if n_contigs is None else n_contigs,
                                      ptr(d_pl), n, C.byref(p), lrec[GUARD:].data_ptr(), lout[GUARD:].data_ptr() if lists else None, cap if lists else 0, C.byref(no), C.byref(st))
    torch.cuda.synchronize()
    return rc, no.value, st.as_dict(), (lrec.cpu().numpy(), lout.cpu().numpy())


def bands_intact(out, n, cap):
    lrec, lout = out
    return np.all(lrec[:GUARD] == 0xA5) and np.all(lrec[GUARD + n:] == 0xA5) and np.all(lout[:GUARD] == 0xA5) and np.all(lout[GUARD + cap:] == 0xA5)


def run_dev(m, case, max_dist, capacity=None, k=K, **kw):
    """-> the four parts as run_host gives them, from kmx_unitig_pair_lift_dev between guard bands"""
    n = len(case[3])
    cap = n if capacity is None else capacity
    rc, no, st, out = raw_dev(m, case, max_dist, cap, k, **kw)
    if rc:
        raise KmxError(rc, m.L.kmx_last_error().decode(errors="replace"))
    assert bands_intact(out, n, cap) and no <= cap
    lrec, lout = out
    assert np.all(lout[GUARD + no:GUARD + cap] == 0xA5)            # nothing behind what is promised
    return lrec[GUARD:GUARD + n].reshape(-1).view(F.PAIR_LIFT_DTYPE), lout[GUARD:GUARD + no].reshape(-1).view(P.PAIR_LINK_DTYPE), no, st


def expected(case, max_dist, checked=True, canonical=True):
    return F.flat(F.check(*case, max_dist, canonical=canonical) if checked else F.lift(*case, max_dist))


def both(m, case, max_dist, what, checked=True, canonical=True, host=True):
    """host and device form under both fold kernels against the restatement -> what the restatement gives"""
    exp = expected(case, max_dist, checked, canonical)
    for fold in FOLDS:
        m.unitig_pair_lift_fold(fold)
        if host:
            same(run_host(m, case, max_dist), exp, f"{what}: host, {fold} fold")
        same(run_dev(m, case, max_dist), exp, f"{what}: device, {fold} fold")
    m.unitig_pair_lift_fold("wave")
    return exp


# ---- the rule against the restatement
def test_every_entry_its_own_key_at_the_block_and_wave_edges(model):
    for n in SIZES:
        mu = F.random_places(P.CRAFT_U, 5, 9)[0]
        ip, icm = F.identity_place(mu)
        pl = S.random_list(n, 5)
        exp = both(model, (mu, ip, icm, pl), F.ALL, f"identity {n}")
        assert exp[2] == n and exp[1].tobytes() == F.plinks_array(pl).tobytes()      # consequence (a)
        for seed, n_contigs, max_dist in ((2, 12, 300), (3, 40, 0), (4, P.CRAFT_U, F.ALL)):
            both(model, F.random_case(n, seed, n_contigs), max_dist, f"random {n} on {n_contigs} contigs")


def test_one_run_and_runs_around_the_edges(model):
    for n in SIZES:
        exp = both(model, F.runs_case((n,)), F.ALL, f"one run of {n}")
        assert exp[2] == 1 and exp[3][F.STAT_FIELDS.index("n_link")] == n
    exp = both(model, F.runs_case(F.RUN_EDGES), F.ALL, "runs around the edges")
    assert exp[2] == len(F.RUN_EDGES) and np.bincount(exp[0]["out"]).tolist() == list(F.RUN_EDGES)
    ends = set(np.cumsum(F.RUN_EDGES).tolist())
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257} <= ends and {1, 2, 63, 64, 65} <= set(F.RUN_EDGES)
    for run in (0, 6, 10, 12):                                     # a run made only of mirrored entries: the same list
        got = both(model, F.runs_case(F.RUN_EDGES, mirror_run=run), F.ALL, f"run {run} mirrored", canonical=False)
        assert got[1].tobytes() == exp[1].tobytes() and got[0]["flipped"].sum() == F.RUN_EDGES[run]
    both(model, F.runs_case((513,), mirror_run=0), F.ALL, "513 mirrored entries in one run", canonical=False)


def test_every_class_and_the_wrapping_sums(model):
    for unplaced in (False, True):
        mu, place, cm, pl, want = F.classes_case(unplaced)
        for max_dist in (F.CLASSES_MAX_DIST, 0, 1, 55, 140, F.ALL):
            exp = both(model, (mu, place, cm, pl), max_dist, f"classes at {max_dist}", canonical=False, host=not unplaced)
        assert exp[3][F.STAT_FIELDS.index("n_link")] == 6 and exp[3][F.STAT_FIELDS.index("n_far")] == 1
        exp = expected((mu, place, cm, pl), F.CLASSES_MAX_DIST, canonical=False)
        assert exp[0]["cls"].tolist() == want and exp[1]["n_pairs"].tolist() == [9, 2, 5] and exp[1]["sum_dist"].tolist() == [740, 90, 6]
    mu, place, cm = [5, 5], [(0, 0), (2, 4)], [9, 9]               # shift = 4 + 4: sum_dist + n_pairs * shift wraps past 2^64
    pl = [(0, 2, 2 ** 62 + 1, 2 ** 64 - 7, 3, 4), (1, 3, 7, 2 ** 64 - 1, 0, 2 ** 32 - 1)]
    both(model, (mu, place, cm, pl), F.ALL, "wrapping sums", canonical=False)


# ---- what only the device form takes
def test_device_lists_the_host_form_refuses(model):
    mu, place, cm, pl = F.random_case(257, 2, 12)
    r = np.random.default_rng(5)
    dup = pl + [pl[i] for i in r.integers(0, len(pl), 40)] + [(e[0], e[1], e[2] + 1, e[3] + 3, e[4], e[5]) for e in pl[::9]]
    shuffled = [pl[i] for i in r.permutation(len(pl))]
    with_mirrors = sorted(pl + [F.mirrored(e) for e in pl[::3]])
    for what, lst in (("duplicate keys", sorted(dup)), ("not ascending", shuffled), ("an entry beside its mirror", with_mirrors), ("all three", [dup[i] for i in r.permutation(len(dup))] + with_mirrors)):
        exp = both(model, (mu, place, cm, lst), 300, what, checked=False, host=False)
        assert exp[2] > 0
    assert expected((mu, place, cm, shuffled), 300, False)[1].tobytes() == expected((mu, place, cm, pl), 300, False)[1].tobytes()     # consequence (b)
    # unplaced ends: oc beyond C, a contig too long, a unitig that sticks out of its contig
    bad_place, bad_cm = list(place), list(cm)
    bad_place[3] = (2 * len(cm) + 1, 0)
    bad_place[7] = (2 ** 32 - 1, 5)
    bad_place[11] = (place[11][0], cm[place[11][0] >> 1] - mu[11] + 1)
    bad_cm[place[20][0] >> 1] = 2 ** 32
    exp = both(model, (mu, bad_place, bad_cm, pl), 300, "unplaced ends", checked=False, host=False)
    assert exp[3][1] > 4
    rc, no, st, out = raw_dev(model, (mu, place, cm, pl), 300, len(pl), n_contigs=5)      # fewer contigs than place names
    exp = expected((mu, place, cm[:5], pl), 300, False)
    assert rc == 0 and bands_intact(out, len(pl), len(pl)) and out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and no == exp[2]


def test_device_offsets_are_clamped(model):
    """offsets beyond n_ubases: m_u comes from the clamped values, and nothing is read or written outside a buffer"""
    mu, place, cm, pl = F.random_case(129, 2, 12)
    off = offsets_of(mu)
    cut = int(off[len(mu) // 2])
    clamped = [max(int(min(off[u + 1], cut)) - int(min(off[u], cut)) - K + 1, 0) for u in range(len(mu))]
    exp = expected((clamped, place, cm, pl), 300, False)
    rc, no, st, out = raw_dev(model, (mu, place, cm, pl), 300, len(pl), n_ubases=cut)
    assert rc == 0 and bands_intact(out, len(pl), len(pl))
    assert out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and no == exp[2] and out[1][GUARD:GUARD + no].tobytes() == exp[1].tobytes()


# ---- capacities and empty inputs
def test_range_leaves_the_list_untouched_and_the_handle_usable(model):
    case = F.random_case(256, 2, 12)
    pl = case[3]
    exp = expected(case, 300)
    n_out = exp[2]
    assert 1 < n_out < len(pl)
    with pytest.raises(KmxError) as e:
        run_host(model, case, 300, capacity=n_out - 1)
    assert e.value.code == -5 and e.value.needed == n_out and e.value.result[0].tobytes() == exp[0].tobytes() and [e.value.result[1][f] for f in F.STAT_FIELDS] == exp[3]
    rc, no, st, out = raw_dev(model, case, 300, n_out - 1)
    assert rc == -5 and no == n_out and [st[f] for f in F.STAT_FIELDS] == exp[3]
    assert out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and np.all(out[1] == 0xA5)
    same(run_dev(model, case, 300, capacity=n_out), exp, "the exact capacity")
    same(run_host(model, case, 300, capacity=n_out), exp, "the exact capacity: host")
    # the sizing call: no list, the records and n_out only
    rc, no, st, out = raw_dev(model, case, 300, 0, lists=False)
    assert rc == 0 and no == n_out and out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and bands_intact(out, len(pl), 0)
    rec, lout, st = model.unitig_pair_lift_flat(K, offsets_of(case[0]), place_array(case[1]), crec_array(case[2]), F.plinks_array(pl), 300, lists=False)
    assert lout is None and rec.tobytes() == exp[0].tobytes() and st["n_out"] == n_out


def test_no_unitig_and_no_entry(model):
    mu, place, cm, pl = F.random_case(33, 2, 12)
    exp = both(model, ([], [], [], pl), 300, "U == 0")
    assert exp[3][1] == len(pl) and exp[2] == 0 and np.all(exp[0]["out"] == F.NO_OUT)
    exp = both(model, (mu, place, cm, []), 300, "n_plinks == 0")
    assert not any(exp[3]) and exp[2] == 0
    both(model, ([], [], [], []), 300, "nothing at all")


# ---- the refusals
def test_bad_arguments_are_refused_before_anything_runs(model):
    import torch
    m = model
    mu, place, cm, pl = F.random_case(33, 2, 12)
    off, arr, pla, cra = offsets_of(mu), F.plinks_array(pl), place_array(place), crec_array(cm)
    n, nu, nc = len(arr), len(mu), len(cm)
    fresh = lambda: np.full(n, 0x5A, dtype=np.uint8).repeat(32).view(F.PAIR_LIFT_DTYPE)
    rec = fresh()
    lout = np.zeros(n, dtype=P.PAIR_LINK_DTYPE)
    st, no = PairLiftStats(), C.c_uint64(0)
    good = PairLiftParams(300, 0)

    def host(k=K, off=off, nu=nu, pla=pla, cra=cra, nc=nc, arr=arr, n=n, par=good, rec=rec, lout=lout, cap=n, no=no, st=st, pl_ptr=None):
        p = lambda a: a.ctypes.data if a is not None else None
        return m.L.kmx_unitig_pair_lift(m.h, k, p(off), nu, p(pla), p(cra), nc, p(arr) if pl_ptr is None else pl_ptr, n, C.byref(par) if par is not None else None, p(rec), p(lout), cap,
                                        C.byref(no) if no is not None else None, C.byref(st) if st is not None else None)

    assert host() == 0
    rec[:] = fresh()
    bad_off, short = off.copy(), off.copy()
    bad_off[3] = bad_off[2] - 1 if bad_off[2] else 0
    bad_off[0] = 1
    short[1:] -= off[1] - np.uint64(K - 1)                       # the first unitig has k - 1 bytes
    beyond, outside, long_c = pla.copy(), pla.copy(), cra.copy()
    beyond["oc"][4] = 2 * nc
    outside["off"][4] = cm[place[4][0] >> 1] - mu[4] + 1
    long_c["n_kmers"][place[4][0] >> 1] = 2 ** 32
    cases = dict(even_k=dict(k=20), small_k=dict(k=3), large_k=dict(k=65), many_unitigs=dict(nu=2 ** 31), many_entries=dict(n=2 ** 31), more_contigs_than_unitigs=dict(nc=nu + 1),
                 reserved=dict(par=PairLiftParams(300, 1)), null_params=dict(par=None), null_n_out=dict(no=None), null_stats=dict(st=None), null_lrec=dict(rec=None), null_uoffsets=dict(off=None),
                 null_place=dict(pla=None), null_crec=dict(cra=None), null_plinks=dict(arr=None), capacity_without_a_list=dict(lout=None), overlap=dict(lout=rec.view(P.PAIR_LINK_DTYPE)),
                 in_out_overlap=dict(pl_ptr=lout.ctypes.data), bad_offsets=dict(off=bad_off), short_unitig=dict(off=short), unsorted=dict(arr=arr[::-1].copy()), contig_beyond_c=dict(pla=beyond),
                 unitig_outside_its_contig=dict(pla=outside), contig_too_long=dict(cra=long_c))
    for what, kw in cases.items():
        assert host(**kw) == -1, what
        assert np.all(rec.view(np.uint8) == 0x5A), f"{what}: something ran"
    # the device form: parameters, NULL and overlap only
    d_off, d_pl = to_dev(off, np.int64), to_dev(arr.view(np.uint8).reshape(-1, 32))
    d_place, d_crec = to_dev(pla.view(np.uint8).reshape(-1, 8)), to_dev(cra.view(np.uint8).reshape(-1, 64))
    d_rec = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    d_lout = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")

    def dev(k=K, nu=nu, nc=nc, n=n, par=good, rec=d_rec.data_ptr(), lout=d_lout.data_ptr(), cap=n, no=no, st=st, pl=d_pl.data_ptr(), pla=d_place.data_ptr(), cra=d_crec.data_ptr()):
        return m.L.kmx_unitig_pair_lift_dev(m.h, k, d_off.data_ptr(), nu, int(off[-1]), pla, cra, nc, pl, n, C.byref(par) if par is not None else None, rec, lout, cap,
                                            C.byref(no) if no is not None else None, C.byref(st) if st is not None else None)

    for what, kw in dict(even_k=dict(k=22), many_unitigs=dict(nu=2 ** 31), many_entries=dict(n=2 ** 31), more_contigs_than_unitigs=dict(nc=nu + 1), reserved=dict(par=PairLiftParams(300, 7)),
                         null_params=dict(par=None), null_n_out=dict(no=None), null_stats=dict(st=None), null_lrec=dict(rec=None), null_plinks=dict(pl=None), null_place=dict(pla=None),
                         null_crec=dict(cra=None), capacity_without_a_list=dict(lout=None), overlap=dict(lout=d_rec.data_ptr()), in_out_overlap=dict(lout=d_pl.data_ptr())).items():
        assert dev(**kw) == -1, what
        torch.cuda.synchronize()
        assert bool((d_rec == 0x5A).all()), f"{what}: something ran"
    assert dev() == 0
    with pytest.raises(KmxError):
        m.unitig_pair_lift_fold(2)
    same(run_dev(m, (mu, place, cm, pl), 300), expected((mu, place, cm, pl), 300), "the handle after the refusals")


def test_a_handle_serves_a_larger_then_a_smaller_list():
    m = KModel(1, 1023, NH, NB)
    for n in (513, 63, 257):
        both(m, F.random_case(n, 2, 12), 300, f"reuse {n}")
    m.set_profile(1)
    case = F.runs_case(F.RUN_EDGES)
    same(run_dev(m, case, F.ALL), expected(case, F.ALL), "under the profile")
    ph = m.unitig_pair_lift_phases()
    assert set(ph) == {"classify", "sort", "fold", "store"} and all(v > 0 for v in ph.values())
    m.set_profile(0)


# ---- the acceptance case: consequence (d) through the real calls
@pytest.mark.parametrize("seed,holes", X.ISLAND_CASES)
def test_lifted_list_is_the_remapped_list_and_scaffolds_the_genome(seed, holes):
    """the pairs mapped onto the pieces of the three islands, the contigs from the walks' link hits, the lift on the device; the
    same pairs mapped onto the contigs: the two lists are equal byte for byte, the SAME sums agree, and the scaffold of the lifted
    list after the reduction is the genome with both holes as N"""
    import torch
    c = F.islands_lifted(seed, holes)                              # asserts the preconditions of (d) on the CPU
    k, pieces, rows, reads, genome = c["k"], c["pieces"], c["rows"], c["reads"], c["genome"]
    m = KModel(1, 1023, NH, NB)
    buf, off = R.join(pieces)
    loff = np.cumsum([0] + [len(r) for r in rows], dtype=np.uint64).astype(np.uint64)
    links = np.array([t for r in rows for t in r], dtype=np.uint32)
    m.unitig_map_begin(U.pack(c["km"], k), k, buf, off)
    hits = np.zeros(links.size, dtype=np.uint64)
    urec, ulist, ust, _, uwo, _ = m.seq_to_pairs(reads, loff, links, F.ISLAND_MAX_DIST, k, 0, n_bins=64, link_hits=hits)
    m.unitig_map_end()
    assert ust["n_far"] == 0 and np.all(np.diff(uwo.astype(np.int64)) == 1) and ulist.tobytes() == F.plinks_array(c["ulist"]).tobytes()
    d_buf, d_off, d_loff, d_links, d_hits = to_dev(buf), to_dev(off, np.int64), to_dev(loff, np.int64), to_dev(links, np.int32), to_dev(hits, np.int64)
    out, (nc, ncb, ncl), cst = m.unitig_contigs_dev(k, d_buf, d_off, d_loff, d_links, d_hits, 1, 0)
    assert nc == 3
    d_cseq, d_coff, d_crec, _, d_place, d_cloff, d_clinks, _ = out
    d_pl = to_dev(ulist.view(np.uint8).reshape(-1, 32))
    exp = F.flat(c["lifted"])
    for fold in FOLDS:
        m.unitig_pair_lift_fold(fold)
        (d_lrec, d_lout), n_out, lst = m.unitig_pair_lift_dev(k, d_off, len(buf), d_place, d_crec, nc, d_pl, len(ulist), F.ISLAND_MAX_DIST)
        same((d_lrec.cpu().numpy().reshape(-1).view(F.PAIR_LIFT_DTYPE), d_lout.cpu().numpy()[:n_out], n_out, lst), exp, f"the islands, {fold} fold")
    # the same pairs mapped onto the contigs, with the contig graph's CSR
    cbuf, coff = d_cseq.cpu().numpy()[:ncb], d_coff.cpu().numpy()[:nc + 1].view(np.uint64)
    cloff, clinks = d_cloff.cpu().numpy()[:2 * nc + 1].view(np.uint64), d_clinks.cpu().numpy()[:ncl].view(np.uint32)
    m.unitig_map_begin(U.pack(c["km"], k), k, cbuf, coff)
    crec, clist, cpst, _, cwo, _ = m.seq_to_pairs(reads, cloff, clinks, F.ISLAND_MAX_DIST, k, 0, n_bins=64)
    m.unitig_map_end()
    assert cpst["n_far"] == 0 and np.all(np.diff(cwo.astype(np.int64)) == 1)
    assert np.all(urec["cls"][crec["cls"] == P.LINK] == P.LINK)     # every contig-level LINK pair is a LINK on the pieces
    assert d_lout.cpu().numpy()[:n_out].tobytes() == clist.tobytes() and n_out == len(clist) == 3
    same_d = lambda rec: int(rec["d"][rec["cls"] == P.SAME].sum())
    assert same_d(urec) + lst["sum_same_d"] == same_d(crec) and lst["n_same_back"] == 0
    # reduce, then scaffold, where the lift call left the list
    (d_rrec, d_red, _), n_red, rst = m.unitig_pair_reduce_dev(k, d_coff, ncb, d_lout, n_out, **{f: X.ISLAND_PAR[f] for f in ("inner", "tol", "min_pairs", "max_row")})
    sp = X.SCAFFOLD_PAR
    sout, (ns, nb), sst = m.unitig_scaffold_dev(k, d_cseq[:ncb], d_coff[:nc + 1], d_red, n_red, sp["inner"], sp["min_pairs"], sp["ratio"], sp["min_n"], sp["max_n"])
    torch.cuda.synchronize()
    s = sout[0].cpu().numpy()[:nb].tobytes().decode()
    s = s if s[:50] == genome[:50] else S.oriented(s, 1)
    assert (ns, nb) == (1, X.ISLAND_GENOME) and rst["n_transitive"] == 1
    assert all(x == g for x, g in zip(s, genome) if x != "N") and all(s[lo:hi] == "N" * (hi - lo) for lo, hi in holes)
    # the convenience of the Python layer, on host buffers
    place, crecs = d_place.cpu().numpy().reshape(-1).view(Cn.CONTIG_PLACE_DTYPE), d_crec.cpu().numpy().reshape(-1).view(Cn.CONTIG_DTYPE)[:nc]
    cstrs = [cbuf[int(coff[i]):int(coff[i + 1])].tobytes().decode() for i in range(nc)]
    got = m.lifted_scaffolds_from_pairs(k, pieces, place, crecs, cstrs, ulist, sp["inner"], F.ISLAND_MAX_DIST, sp["min_pairs"], sp["ratio"], sp["min_n"], sp["max_n"])
    assert got[6].tobytes() == clist.tobytes() and len(got[0]) == 3 and got[7]["n_out"] == 3      # the full lifted list: the skipping link keeps the three apart


# ---- the facade
def test_facade(tmp_path):
    """tests/facade_unitig_pair_lift.cpp prints the stats, the table of write_pair_lift_tsv and the lifted list"""
    mu, place, cm, pl = F.random_case(257, 2, 12)
    res = F.lift(mu, place, cm, pl, 300)
    for name, rows in (("list.txt", pl), ("place.txt", place), ("crec.txt", [(x,) for x in cm])):
        with open(tmp_path / name, "w") as f:
            f.write("".join(" ".join(map(str, e)) + "\n" for e in rows))
    exe = str(tmp_path / "facade_unitig_pair_lift")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_unitig_pair_lift.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    out = subprocess.check_output([exe, str(K), "300", ",".join(str(x + K - 1) for x in mu), str(tmp_path / "place.txt"), str(tmp_path / "crec.txt"), str(tmp_path / "list.txt")], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 3 and blocks[0] == " ".join(str(res["stats"][f]) for f in F.STAT_FIELDS[:15]) + "\n"
    assert blocks[1] == F.lift_tsv(pl, res) and blocks[2] == "".join(" ".join(map(str, e)) + "\n" for e in res["lout"])


# ---- the driver
def test_driver_scaffolds_the_contigs_from_the_lifted_list(tmp_path):
    """kmcEx -u1 -M -W21 -P400 -X1 -S2 -J on the reads of the three islands writes pairs.lifted.tsv as the restatement gives it, and
    scaffolds.fa, scaffolds.paths.tsv and scaffolds.agp (with -L and -F: every file) byte for byte as the run that maps the pairs
    onto the contigs; -J needs -X -S and does not go with -R"""
    import count_reads as CR
    seed, holes = X.ISLAND_CASES[0]
    k, strs, ipl, genome = X.three_islands(seed, holes)
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in X.island_reads(seed, holes)[1]])
    mu = [len(s) - k + 1 for s in strs]
    res = F.lift(mu, *F.identity_place(mu), ipl, P.MAX_DIST)       # no graph edge: every contig is one unitig
    exe = str(tmp_path / "kmcEx")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "kmcex_main.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    base = ["-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-X1", "-S2", f"-k{k}", "-nh3", "-nb2"]
    texts = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix in (".fa", ".tsv", ".gaf", ".gfa", ".agp")}
    for flags in ((), ("-L",), ("-L", "-F")):
        runs = {}
        for lift in ((), ("-J",)):
            work = tmp_path / ("run" + "".join(flags + lift))
            work.mkdir()
            log = subprocess.check_output([exe, *base, *flags, *lift, fa, "db", str(work)], timeout=120).decode()
            runs[lift] = texts(work / "db")
            assert ("pair links lifted to the contigs" in log) == bool(lift)
        plain, lifted = runs[()], runs[("-J",)]
        assert "pairs.lifted.tsv" not in plain and lifted.pop("pairs.lifted.tsv").decode() == F.lift_tsv(ipl, res), flags
        assert {"scaffolds.fa", "scaffolds.paths.tsv", "scaffolds.agp"} <= set(lifted) and lifted == plain, flags
        assert lifted["scaffolds.fa"].count(b">") == (1 if flags else 3)
    assert subprocess.call([exe, "-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-S2", "-J", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2     # -J without -X
    assert subprocess.call([exe, "-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-X1", "-J", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2     # -J without -S
    assert subprocess.call([exe, *base, "-R2", "-J", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
