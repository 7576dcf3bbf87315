"""kmx_unitig_pair_paths* on the MI355X: the records, steps, through, path_hits and stats equal, byte for byte, what the
plain-Python restatement of the rule (tests/unitig_pair_paths_ref.py) gives, for the host and the device form (the device form
always between guard bands): on the acceptance case through the live session (a repeat longer than a read, which the contigs cross
only with this call), on crafted graphs with every verdict at the block edges, the depth of the stack, max_visits at its
threshold, a hub, mirrored lists, accumulation, KMX_E_RANGE and psteps = NULL, the refusals, crafted device input, allocation
failures, the facade and the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pair_paths_ref as Q
import unitig_pairs_ref as P
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import KmxError, PairPathParams, PairPathStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the paths
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
PARTS = ("precs", "psteps", "through", "path_hits")


@pytest.fixture(scope="module")
def model():
    return KModel(1, 1023, NH, NB)


def params_of(par):
    q = dict(Q.PAR, **par)
    return q["min_pairs"], q["inner"], q["tol"], q["max_steps"], q["max_visits"]


def graph_of(g):
    """-> (k, uint64 uoffsets, uint64 link_offsets, uint32 links)"""
    _, off = R.join(g.strs)
    loff, lk = L.flat_links(g.rows)
    return g.k, off, loff, lk


def expected(g, plinks, through=None, path_hits=None, mirrored_graph=True, **par):
    q = dict(Q.PAR, **par)
    res = Q.pair_paths(g.mu, g.rows, plinks, through=through, path_hits=path_hits, **q)
    if through is None and path_hits is None:
        Q.check(g.mu, g.rows, plinks, res, q, mirrored_graph)
    return Q.flat(res)


def same(got, exp, what):
    for a, b, part in zip(got[:4], exp[:4], PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"
    assert got[4] == exp[4], f"{what}: stats differ: {got[4]} != {exp[4]}"


def run_host(m, g, plinks, through=None, path_hits=None, capacity=None, **par):
    k, off, loff, lk = graph_of(g)
    mp, inner, tol, ms, mv = params_of(par)
    t = np.zeros(16 * len(g.mu), np.uint64) if through is None else np.array(through, dtype=np.uint64)
    h = np.zeros(len(lk), np.uint64) if path_hits is None else np.array(path_hits, dtype=np.uint64)
    rec, pst, st = m.unitig_pair_paths_flat(k, off, loff, lk, Q.plinks_array(plinks), inner, tol, mp, ms, mv, through=t, path_hits=h, capacity=capacity)
    return rec, pst, t, h, st


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def raw_dev(m, k, off, loff, lk, plinks, cap, through=None, path_hits=None, n_plinks=None, n_links=None, steps=True, sums=True, **par):
    """one kmx_unitig_pair_paths_dev call whose four outputs lie between guard bands of GUARD elements -> (rc, n_psteps, stats, the
    four outputs with their bands as NumPy arrays)"""
    import torch
    nu, nl = len(off) - 1, len(lk)
    pl = Q.plinks_array(plinks) if isinstance(plinks, list) else plinks
    n = len(pl)
    d_pl = to_dev(pl.view(np.uint8).reshape(-1, 32)) if n else None
    d_off, d_loff, d_lk = to_dev(off, np.int64), to_dev(loff, np.int64), to_dev(lk if nl else np.zeros(1, np.uint32), np.int32)
    band = lambda body, fill, dt: torch.cat([torch.full((GUARD,) + tuple(body.shape[1:]), fill, dtype=dt, device="cuda"), body, torch.full((GUARD,) + tuple(body.shape[1:]), fill, dtype=dt, device="cuda")])
    precs = torch.full((n + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    psteps = torch.full((cap + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    t = band(to_dev(np.zeros(16 * nu, np.uint64) if through is None else np.array(through, dtype=np.uint64), np.int64), -7, torch.int64)
    h = band(to_dev(np.zeros(nl, np.uint64) if path_hits is None else np.array(path_hits, dtype=np.uint64), np.int64), -7, torch.int64)
    p, st, ns = PairPathParams(*params_of(par), 0), PairPathStats(), C.c_uint64(0)
    ptr = lambda x: x.data_ptr() if x is not None else None
    rc = m.L.kmx_unitig_pair_paths_dev(m.h, k, d_off.data_ptr(), nu, d_loff.data_ptr(), d_lk.data_ptr(), nl if n_links is None else n_links, ptr(d_pl), n if n_plinks is None else n_plinks, C.byref(p),
                                       precs[GUARD:].data_ptr(), psteps[GUARD:].data_ptr() if steps else None, cap if steps else 0, C.byref(ns), t[GUARD:].data_ptr() if sums else None,
                                       h[GUARD:].data_ptr() if sums else None, C.byref(st))
    torch.cuda.synchronize()
    return rc, ns.value, st.as_dict(), tuple(x.cpu().numpy() for x in (precs, psteps, t, h))


def bands_intact(out, n, cap, nu, nl):
    precs, psteps, t, h = out
    return (np.all(precs[:GUARD] == 0xA5) and np.all(precs[GUARD + n:] == 0xA5) and np.all(psteps[:GUARD] == -7) and np.all(psteps[GUARD + cap:] == -7) and
            np.all(t[:GUARD] == -7) and np.all(t[GUARD + 16 * nu:] == -7) and np.all(h[:GUARD] == -7) and np.all(h[GUARD + nl:] == -7))


def run_dev(m, g, plinks, through=None, path_hits=None, capacity=None, **par):
    """-> the five parts as run_host gives them, from kmx_unitig_pair_paths_dev between guard bands"""
    k, off, loff, lk = graph_of(g)
    n, nu, nl = len(plinks), len(g.mu), len(lk)
    cap = n * params_of(par)[3] if capacity is None else capacity
    rc, ns, st, out = raw_dev(m, k, off, loff, lk, plinks, cap, through, path_hits, **par)
    if rc:
        raise KmxError(rc, m.L.kmx_last_error().decode(errors="replace"))
    assert bands_intact(out, n, cap, nu, nl) and ns <= cap
    precs, psteps, t, h = out
    assert np.all(psteps[GUARD + ns:GUARD + cap] == -7)          # nothing behind what is promised
    return (precs[GUARD:GUARD + n].reshape(-1).view(Q.PAIR_PATH_DTYPE), psteps[GUARD:GUARD + ns].view(np.uint32), t[GUARD:GUARD + 16 * nu].view(np.uint64), h[GUARD:GUARD + nl].view(np.uint64), st)


def both(m, g, plinks, what, **par):
    exp = expected(g, plinks, **par)
    same(run_host(m, g, plinks, **par), exp, f"{what}: host")
    same(run_dev(m, g, plinks, **par), exp, f"{what}: device")
    return exp


# ---- the acceptance case, through the live session
def test_the_repeat_is_crossed_through_the_live_session():
    """map, walks, through hits and pairs from the library, then the pair paths, resolve and contigs: the genome as one contig of
    1800 bytes; the same chain without the new call leaves the 4 unitigs"""
    k, genome, km, cnt, strs, reads, rows = Q.acceptance()
    loff, lk = L.flat_links(rows)
    buf, off = R.join(strs)
    mm, md, bw, nb = P.READ_PARAMS
    m = KModel(1, 1023, NH, NB)
    m.unitig_map_begin(U.pack(km, k), k, buf, off)
    hits = np.zeros(len(lk), np.uint64)
    rec, lst, st, walks, wo, steps = m.seq_to_pairs(reads, loff, lk, md, k, 0, mm, bw, nb, pair_hits=hits, link_hits=hits)
    through, _ = m.unitig_through_flat(walks, steps, loff, lk)
    m.unitig_map_end()
    assert len(lst) == 6 and np.all(rec["d"][rec["cls"] == P.SAME] == 221) and not through.any()
    without = m.unitig_resolve_flat(k, buf, off, loff, lk, through, 2, 0, link_hits=hits)
    assert without[9]["n_unsupported"] == 1 and without[9]["n_resolved"] == 0
    assert m.unitig_contigs_flat(k, without[0], without[1], without[5], without[6], without[8], 1, 0)[8]["n_contigs"] == 4
    plinks = [tuple(int(x) for x in e) for e in lst]
    g = type("G", (), dict(k=k, strs=strs, mu=[len(s) - k + 1 for s in strs], rows=rows))
    exp = both(m, g, plinks, "the acceptance case", **Q.ACCEPT_PAR)
    assert exp[4]["n_path"] == 2 and exp[4]["n_adjacent"] == 4 and sorted(int(x) for x in exp[2][exp[2] > 0]) == [91, 91]
    assert [(int(r["n_steps"]), int(r["windows"])) for r in exp[0] if r["verdict"] == Q.PATH] == [(1, 130), (1, 130)]
    q = Q.ACCEPT_PAR
    prec, pst, pstats = m.unitig_pair_paths_flat(k, off, loff, lk, lst, q["inner"], q["tol"], q["min_pairs"], q["max_steps"], q["max_visits"], through=through, path_hits=hits)
    assert pstats == exp[4]
    r = m.unitig_resolve_flat(k, buf, off, loff, lk, through, 2, 0, link_hits=hits)
    assert r[9]["n_resolved"] == 1 and r[9]["n_unsupported"] == 0
    c = m.unitig_contigs_flat(k, r[0], r[1], r[5], r[6], r[8], 1, 0)
    assert c[8]["n_contigs"] == 1 and len(c[0]) == 1800 and c[0].tobytes().decode() in (genome, U.rc(genome))
    # the one call that does it all, with and without the pair evidence
    m.unitig_map_begin(U.pack(km, k), k, buf, off)
    cstrs, rst, pstats2, _ = m.resolved_contigs_from_pairs(k, buf, off, loff, lk, reads, md, max_gap=k, max_indel=0)
    four, rst0, none, _ = m.resolved_contigs_from_pairs(k, buf, off, loff, lk, reads, md, max_gap=k, max_indel=0, pair_paths=False)
    m.unitig_map_end()
    assert len(cstrs) == 1 and cstrs[0] in (genome, U.rc(genome)) and rst["n_resolved"] == 1 and pstats2 == exp[4]
    assert len(four) == 4 and rst0["n_unsupported"] == 1 and none is None


# ---- crafted graphs over the pair tests' unitig set: U = 100, m_u in 1, 2, 7, 64, 300
@pytest.mark.parametrize("n", P.CRAFT_SIZES)
def test_mixed_lists_at_the_block_edges(model, n):
    g, named = Q.crafted()
    lst = Q.crafted_list(n, n, Q.PAR)
    exp = both(model, g, lst, f"{n} entries")
    if n >= 255:
        assert min(exp[4][f] for f in ("n_ignored", "n_below_min", "n_no_path", "n_adjacent", "n_path", "n_ambiguous")) >= 1
    both(model, g, lst, f"{n} entries, a wide tolerance and few visits", tol=40, max_visits=6, min_pairs=1)
    # consequence (b): every entry mirrored (the list is no longer sorted: the device form takes it as it is)
    mir = [Q.mirrored(e) for e in lst]
    got = run_dev(model, g, mir)
    same(got, expected(g, mir), f"{n} entries mirrored")
    assert got[2].tobytes() == exp[2].tobytes() and np.array_equal(got[0]["verdict"], exp[0]["verdict"]) and np.array_equal(got[0]["windows"], exp[0]["windows"])


def test_every_named_gadget(model):
    """the 3-hop path, the division that floors, the bubbles at tol = 0 and at the difference of their arms, the ladder with max_visits
    at n_prefix and one below, max_steps = 1 and 16 on the chains of 16 and 17 (the deepest stack), the self-loop gone round twice,
    hi < 0, and the entries that are ignored or below min_pairs"""
    g, named = Q.crafted()
    for name, (e, q, verdict) in named.items():
        lst = sorted(e) if name == "hub" else [e]
        exp = both(model, g, lst, name, **q)
        assert set(int(v) for v in exp[0]["verdict"]) == {verdict}, name
    exp = both(model, g, [named["chain16"][0]], "chain16", max_steps=16)
    assert int(exp[0]["n_steps"][0]) == 16 and len(exp[1]) == 16 and exp[4]["n_added"] == 16
    assert int(both(model, g, [named["hi_negative"][0]], "hi < 0", tol=3)[0]["n_visited"][0]) == 0
    lad = named["ladder_below"]
    assert int(both(model, g, [lad[0]], "ladder", **lad[1])[0]["n_visited"][0]) == lad[1]["max_visits"] + 1


def test_a_hub_that_300_entries_pass(model):
    """300 atomics onto one cell of through and onto two cells of path_hits (device form: the list holds every key many times and in
    both of its forms), and the 16 keys of the hub through both forms"""
    g, named = Q.crafted()
    lst = Q.hub_list(300)
    exp = expected(g, lst)
    same(run_dev(model, g, lst), exp, "the hub")
    assert exp[4]["n_path"] == 300 and int(exp[2].max()) == sum(e[2] for e in lst) and int((exp[2] > 0).sum()) == 1 + 2 * 4
    both(model, g, sorted(named["hub"][0]), "the hub's keys")


def test_accumulation_into_arrays_that_hold_counts(model):
    g, named = Q.crafted()
    lst = Q.crafted_list(257, 9, Q.PAR)
    r = np.random.RandomState(5)
    t0 = [int(x) for x in r.randint(0, 1000, 16 * len(g.mu))]
    h0 = [int(x) for x in r.randint(0, 1000, sum(len(x) for x in g.rows))]
    t0[0], h0[0] = 2 ** 63, 2 ** 63                              # counts beyond 32 bits stay counts
    exp = expected(g, lst, through=t0, path_hits=h0)
    same(run_host(model, g, lst, through=t0, path_hits=h0), exp, "accumulation: host")
    same(run_dev(model, g, lst, through=t0, path_hits=h0), exp, "accumulation: device")
    plain = expected(g, lst)
    assert np.array_equal(exp[2][1:] - np.array(t0[1:], dtype=np.uint64), plain[2][1:])


def test_range_with_the_repeat_convention_and_no_list(model):
    """capacity one short: KMX_E_RANGE with the number needed, records, stats, through and path_hits complete, the steps that fit
    stored and nothing behind them; the repeated call with both sums NULL adds nothing twice; psteps = NULL builds no list"""
    m = model
    g, named = Q.crafted()
    lst = Q.crafted_list(513, 513, Q.PAR)
    exp = expected(g, lst)
    need = len(exp[1])
    assert need > 20
    k, off, loff, lk = graph_of(g)
    nu, nl, n = len(g.mu), len(lk), len(lst)
    for cap in (need - 1, 3, 0):
        rc, ns, st, out = raw_dev(m, k, off, loff, lk, lst, cap)
        assert rc == -5 and ns == need and st == exp[4] and bands_intact(out, n, cap, nu, nl)
        assert out[0][GUARD:GUARD + n].tobytes() == exp[0].tobytes() and out[1][GUARD:GUARD + cap].view(np.uint32).tobytes() == exp[1][:cap].tobytes()
        assert out[2][GUARD:GUARD + 16 * nu].view(np.uint64).tobytes() == exp[2].tobytes() and out[3][GUARD:GUARD + nl].view(np.uint64).tobytes() == exp[3].tobytes()
    rc, ns, st, out = raw_dev(m, k, off, loff, lk, lst, need, sums=False)     # the repeat: no sums
    assert rc == 0 and ns == need and st == exp[4] and out[1][GUARD:GUARD + need].view(np.uint32).tobytes() == exp[1].tobytes() and not out[2][GUARD:-GUARD].any()
    rc, ns, st, out = raw_dev(m, k, off, loff, lk, lst, 0, steps=False)
    assert rc == 0 and st == exp[4] and ns == need and out[0][GUARD:GUARD + n].tobytes() == exp[0].tobytes() and bands_intact(out, n, 0, nu, nl)
    with pytest.raises(KmxError) as e:
        run_host(m, g, lst, capacity=need - 1)
    assert e.value.code == -5 and e.value.needed == need and e.value.result[0].tobytes() == exp[0].tobytes() and e.value.result[1] == exp[4]
    same(run_host(m, g, lst, capacity=need), exp, "capacity exactly what is needed")
    rec, pst, st = m.unitig_pair_paths_flat(k, off, loff, lk, Q.plinks_array(lst), *params_of({})[1:3], steps=False)
    assert pst is None and rec.tobytes() == exp[0].tobytes() and st == exp[4]


# ---- the refusals
def test_refusals(model):
    import torch
    m = model
    g, named = Q.crafted()
    k, off, loff, lk = graph_of(g)
    nu, nl = len(g.mu), len(lk)
    lst = Q.crafted_list(40, 2, Q.PAR)
    pl = Q.plinks_array(lst)
    exp = expected(g, lst)
    rec, pst = np.zeros(len(pl), Q.PAIR_PATH_DTYPE), np.zeros(8 * len(pl), np.uint32)
    t, h = np.zeros(16 * nu, np.uint64), np.zeros(nl, np.uint64)
    d = dict(off=to_dev(off, np.int64), loff=to_dev(loff, np.int64), lk=to_dev(lk, np.int32), pl=to_dev(pl.view(np.uint8).reshape(-1, 32)), rec=to_dev(rec.view(np.uint8).reshape(-1, 32)),
             pst=to_dev(pst, np.int32), t=to_dev(t, np.int64), h=to_dev(h, np.int64))
    ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()

    def call(fn, kk=k, o=off, n=nu, lo=loff, l=lk, n_l=nl, p=pl, n_pl=len(pl), par=(2, 300, 0, 8, 4096, 0), r=rec, s=pst, c=None, count=True, tt=t, hh=h, stats=True):
        q, st, ns = (PairPathParams(*par) if par else None), PairPathStats(), C.c_uint64(0)
        return fn(m.h, kk, ptr(o), n, ptr(lo), ptr(l), n_l, ptr(p), n_pl, C.byref(q) if q else None, ptr(r), ptr(s), (8 * len(pl) if c is None else c), C.byref(ns) if count else None, ptr(tt), ptr(hh),
                  C.byref(st) if stats else None)

    host_rc = lambda **kw: call(m.L.kmx_unitig_pair_paths, **kw)
    dev_rc = lambda **kw: call(m.L.kmx_unitig_pair_paths_dev, **dict(dict(o=d["off"], lo=d["loff"], l=d["lk"], p=d["pl"], r=d["rec"], s=d["pst"], tt=d["t"], hh=d["h"]), **kw))
    assert host_rc() == 0 and dev_rc() == 0
    for kk in (20, 3, 65):
        assert host_rc(kk=kk) == -1 and dev_rc(kk=kk) == -1
    assert dev_rc(n=2 ** 31) == -1 and dev_rc(n_pl=2 ** 31) == -1 and host_rc(n_pl=2 ** 31) == -1
    for par in ((2, 300, 0, 0, 4096, 0), (2, 300, 0, 17, 4096, 0), (2, 300, 0, 8, 0, 0), (2, 300, 0, 8, 65537, 0), (2, 300, 0, 8, 4096, 1)):
        assert host_rc(par=par) == -1 and dev_rc(par=par) == -1
    assert host_rc(par=None) == -1 and host_rc(stats=False) == -1 and host_rc(count=False) == -1 and dev_rc(count=False) == -1
    assert host_rc(s=None, count=False) == 0 and host_rc(tt=None, hh=None) == 0 and dev_rc(s=None, count=False, tt=None) == 0     # what may be NULL
    for name in ("o", "lo", "l", "p", "r"):
        assert host_rc(**{name: None}) == -1 and dev_rc(**{name: None}) == -1, name
    assert host_rc(r=pst.view(Q.PAIR_PATH_DTYPE)) == -1 and host_rc(tt=off, n=1, lo=loff[:3].copy(), n_l=int(loff[2])) == -1 and host_rc(hh=lk[:4].view(np.uint64), n_l=2) == -1   # overlaps
    assert dev_rc(s=d["lk"]) == -1 and dev_rc(tt=d["h"], n_l=16 * nu) == -1
    swapped, above, short = off.copy(), off.copy(), off.copy()
    swapped[3], swapped[4] = off[4] + 1, off[3]
    above[0] = 1
    short[1:] -= np.uint64(int(off[1]) - k + 1)                   # unitig 0 has k - 1 bytes
    for bad in (swapped, above, short):
        assert host_rc(o=bad) == -1
    bad_l, bad_lo = lk.copy(), loff.copy()
    bad_l[5] = 2 * nu
    bad_lo[7] = bad_lo[8] + 1
    assert host_rc(l=bad_l) == -1 and host_rc(lo=bad_lo) == -1 and host_rc(n_l=nl - 1) == -1
    for bad in ([(4, 9, 1, 1, 1, 1), (4, 9, 1, 1, 1, 1)], [(4, 9, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)], [(5, 0, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)]):
        assert host_rc(p=Q.plinks_array(bad), n_pl=2) == -1
    # n_plinks == 0: KMX_OK with all-zero stats; U == 0: every entry is ignored
    q, st, ns = PairPathParams(2, 300, 0, 8, 4096, 0), PairPathStats(), C.c_uint64(9)
    assert m.L.kmx_unitig_pair_paths(m.h, k, off.ctypes.data, nu, loff.ctypes.data, lk.ctypes.data, nl, None, 0, C.byref(q), None, None, 0, C.byref(ns), None, None, C.byref(st)) == 0
    assert ns.value == 0 and st.as_dict() == dict.fromkeys(Q.STAT_FIELDS, 0)
    assert m.L.kmx_unitig_pair_paths_dev(m.h, k, d["off"].data_ptr(), nu, d["loff"].data_ptr(), d["lk"].data_ptr(), nl, None, 0, C.byref(q), None, None, 0, C.byref(ns), None, None, C.byref(st)) == 0
    assert st.as_dict() == dict.fromkeys(Q.STAT_FIELDS, 0)
    zero, r3 = np.zeros(1, np.uint64), np.full(3, 0xA5A5A5A5, np.uint32).repeat(8).view(Q.PAIR_PATH_DTYPE)
    assert m.L.kmx_unitig_pair_paths(m.h, k, zero.ctypes.data, 0, zero.ctypes.data, None, 0, pl.ctypes.data, 3, C.byref(q), r3.ctypes.data, None, 0, None, None, None, C.byref(st)) == 0
    assert st.as_dict() == dict(dict.fromkeys(Q.STAT_FIELDS, 0), n_entries=3, n_ignored=3) and not r3.view(np.uint8).any()
    d_r3 = torch.full((3, 32), 0xA5, dtype=torch.uint8, device="cuda")
    assert m.L.kmx_unitig_pair_paths_dev(m.h, k, d["off"].data_ptr(), 0, d["loff"].data_ptr(), None, 0, d["pl"].data_ptr(), 3, C.byref(q), d_r3.data_ptr(), None, 0, None, None, None, C.byref(st)) == 0
    assert st.as_dict() == dict(dict.fromkeys(Q.STAT_FIELDS, 0), n_entries=3, n_ignored=3) and not d_r3.cpu().numpy().any()
    same(run_host(m, g, lst), exp, "after the refusals: host")
    same(run_dev(m, g, lst), exp, "after the refusals: device")


# ---- crafted device input between guard bands
def test_crafted_device_input_stays_inside_the_buffers(model):
    """the _dev form clamps: rows past n_links, row starts that decrease or are all ones, links >= 2 U, unitigs shorter than k and
    offsets that decrease (m_u = 0: the search then runs to max_steps or max_visits), a list that is not ascending or whose entries
    are no pair links: KMX_OK or KMX_E_RANGE, the call returns and the guard bands around the four outputs are intact"""
    m = model
    g, named = Q.crafted()
    k, off, loff, lk = graph_of(g)
    nu, nl = len(g.mu), len(lk)
    lst = Q.crafted_list(513, 21, Q.PAR)
    pl = Q.plinks_array(lst)
    n, cap = len(pl), 16 * len(pl)
    big = np.uint64(2 ** 64 - 1)
    r = np.random.RandomState(4)

    def ok(what, o=off, lo=loff, l=lk, p=pl, c=cap, **kw):
        rc, ns, st, out = raw_dev(m, k, o, lo, l, p, c, max_steps=16, tol=50, **kw)
        assert rc in (0, -5) and bands_intact(out, len(p), c, nu, len(l)) and st["n_entries"] == len(p), what
        assert sum(st[f] for f in Q.STAT_FIELDS[1:8]) == len(p) and st["n_added"] + st["n_missing"] == ns, what
        return st

    for i, lo in enumerate((loff + np.uint64(nl), loff[::-1].copy(), np.full(len(loff), big), np.where(np.arange(len(loff)) % 2 == 1, big, loff), loff * np.uint64(3))):
        ok(f"row bounds {i}", lo=lo)
    ok("fewer links than the rows say", n_links=nl // 2)
    bad_l = np.where(np.arange(nl) % 3 == 0, np.uint32(2 * nu) + r.randint(0, 9, nl).astype(np.uint32), lk).astype(np.uint32)
    ok("links beyond 2 U", l=bad_l)
    ok("links all ones", l=np.full(nl, 0xFFFFFFFF, np.uint32))
    lo4, dense = np.arange(2 * nu + 1, dtype=np.uint64) * np.uint64(4), r.randint(0, 2 * nu, 8 * nu).astype(np.uint32)   # full rows of random targets: cycles everywhere
    for i, o in enumerate((off[::-1].copy(), np.zeros(len(off), np.uint64), np.full(len(off), big), np.arange(len(off), dtype=np.uint64) * np.uint64(k - 1))):
        st = ok(f"unitig offsets {i}", o=o, lo=lo4, l=dense, max_visits=65536)     # m_u = 0 everywhere: nothing is pruned by W, 4^16 prefixes
        assert st["n_complex"] > 100, i
    bad_lists = []
    for f, v in (("a", 2 * nu + r.randint(0, 9, n)), ("b", np.full(n, 0xFFFFFFFF)), ("n_pairs", np.zeros(n)), ("b", pl["a"] ^ np.uint32(1)), ("sum_dist", np.full(n, big)), ("n_pairs", np.full(n, big))):
        x = pl.copy()
        x[f] = np.where(np.arange(n) % 2 == 0, v, x[f]).astype(x[f].dtype)
        bad_lists.append(x)
    for i, x in enumerate(bad_lists):
        st = ok(f"list {i}", p=x)
        assert i >= 4 or st["n_ignored"] >= (n + 1) // 2, i
    ok("a list that is not ascending", p=pl[::-1].copy())
    rc, ns, st, out = raw_dev(m, k, off, loff, lk, pl, cap, n_plinks=n - 100)     # a shorter count reads a shorter list
    exp = expected(g, lst[:-100])
    assert rc == 0 and st == exp[4] and out[0][GUARD:GUARD + n - 100].tobytes() == exp[0].tobytes() and np.all(out[0][GUARD + n - 100:] == 0xA5)
    same(run_dev(m, g, lst), expected(g, lst), "after the crafted input")


# ---- allocation failures
def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first pair path call in turn, host and device form: the same call then succeeds with
    the right bytes"""
    g, named = Q.crafted()
    lst = Q.crafted_list(60, 3, Q.PAR)
    exp = expected(g, lst)
    failed = {"host": 0, "dev": 0}
    run = {"host": run_host, "dev": run_dev}
    for nth in range(1, 16):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run[variant](m, g, lst)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run[variant](m, g, lst), exp, f"after allocation {nth} failed, {variant}")
    assert failed["host"] >= 10 and failed["dev"] >= 3, failed


# ---- the facade and the driver
def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_pair_paths.cpp prints the stats, the path table, the resolve counts and the contigs for the acceptance
    reads; the driver's -u1 -M -W21 -P400 -X1 -R2 -T writes pairs.paths.tsv and contigs.fa with the genome as one contig, leaves four
    contigs without -T and every other output as it is"""
    import count_reads as CR
    k, genome, km, cnt, strs, reads, rows = Q.acceptance()
    mu = [len(s) - k + 1 for s in strs]
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

    plinks = [(0, 4, 91, 8190, 90, 90), (0, 6, 130, 28600, 220, 220), (3, 5, 91, 8190, 90, 90), (3, 7, 130, 28600, 220, 220), (4, 6, 130, 28600, 220, 220), (5, 7, 130, 28600, 220, 220)]
    q = Q.ACCEPT_PAR
    res = Q.pair_paths(mu, rows, plinks, **q)
    exe = build("tests/facade_unitig_pair_paths.cpp", "facade_unitig_pair_paths")
    out = subprocess.check_output([exe, fa, str(k), "1", lines, "1", str(P.MAX_DIST), str(q["min_pairs"]), str(q["inner"]), str(q["tol"]), str(q["max_steps"]), str(q["max_visits"]), "2"],
                                  timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 4 and blocks[0] == " ".join(str(res["stats"][f]) for f in Q.STAT_FIELDS) + "\n"
    assert blocks[1] == Q.paths_tsv(plinks, res) and blocks[2] == "1 1 0\n" and blocks[3].strip() in (genome, U.rc(genome))
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    base = ["-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-X1", "-R2", f"-k{k}", "-nh3", "-nb2"]
    texts = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix in (".fa", ".tsv", ".gaf", ".gfa", ".agp")}
    work = tmp_path / "plain"
    work.mkdir()
    subprocess.check_call([exe, *base, fa, "db", str(work)], stdout=subprocess.DEVNULL, timeout=120)
    before = texts(work / "db")
    assert "pairs.paths.tsv" not in before and before["contigs.fa"].count(b">") == 4
    for flag in ("-T", "-T21", "-T21,8"):
        work = tmp_path / f"paths{flag}"
        work.mkdir()
        log = subprocess.check_output([exe, *base, flag, fa, "db", str(work)], timeout=120).decode()
        after = texts(work / "db")
        assert after["pairs.paths.tsv"].decode() == Q.paths_tsv(plinks, res), flag
        seqs = [s for s in after["contigs.fa"].decode().split("\n") if s and s[0] != ">"]
        assert len(seqs) == 1 and seqs[0] in (genome, U.rc(genome)), flag
        changed = ("pairs.paths.tsv", "contigs.fa", "contigs.paths.tsv", "unitigs.resolved.tsv")
        assert {n: b for n, b in after.items() if n not in changed} == {n: b for n, b in before.items() if n not in changed}, flag
        assert "pair paths (tol 21, <= 8 steps, inner 221) :     2 of 6 links are one path (4 adjacent, 0 none, 0 ambiguous, 0 complex, 0 below 2 pairs, 0 ignored), 2 unitigs credited" in log
        assert "repeats resolved (>= 2 reads, <= 0 across) :     1 of 1 candidates" in log
    assert subprocess.call([exe, "-g", "-u1", "-M", "-W", f"-P{P.MAX_DIST}", "-X1", "-T", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2     # -T without -R
    assert subprocess.call([exe, "-g", "-u1", "-M", "-W", "-X1", "-R2", "-T", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2                   # -T without -P
    assert subprocess.call([exe, *base, "-T5,0", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2 and subprocess.call([exe, *base, "-T5,17", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
    assert subprocess.call([exe, *base, "-Tx", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
