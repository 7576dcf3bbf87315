"""kmx_unitig_scaffold* on the MI355X: the bases, offsets, records, steps, places and stats equal, byte for byte, what the
plain-Python restatement of the rule (tests/unitig_scaffold_ref.py) gives, for the host and the device form (the device form
always between guard bands): on the two islands through the live session, on crafted lists at the block edges, a hub, cycles of
every length, lists that are not canonical, the ratio at its threshold, every kind of gap estimate, one deep chain as a path and
as a cycle, the densest emit tile with every destination alignment; KMX_E_RANGE and the sizing call, the refusals, crafted device
input, allocation failures, the facade and the driver."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pairs_ref as P
import unitig_scaffold_ref as S
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE, KmxError, ScaffoldParams, ScaffoldStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the scaffolds
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
PAR = dict(min_pairs=2, ratio=0, inner=300, min_n=3, max_n=200)
PARTS = ("sseq", "soffsets", "srec", "steps", "place")


@pytest.fixture(scope="module")
def model():
    return KModel(1, 1023, NH, NB)


def params_of(par):
    q = dict(PAR, **par)
    return q["min_pairs"], q["ratio"], q["inner"], q["min_n"], q["max_n"]


def recs_of(n, seed=11):
    """random unitig records -> (UNITIG_DTYPE array, the (sum, min, max) the restatement reads)"""
    r = np.random.RandomState(seed)
    rec = np.zeros(n, dtype=UNITIG_DTYPE)
    rec["min_count"] = r.randint(1, 50, n)
    rec["max_count"] = rec["min_count"] + r.randint(0, 900, n).astype(np.uint32)
    rec["sum_count"] = rec["max_count"].astype(np.uint64) * 3 + np.uint64(7)
    return rec, [(int(a), int(b), int(c)) for a, b, c in zip(rec["sum_count"], rec["min_count"], rec["max_count"])]


def expected(k, strs, plinks, recs=None, **par):
    res = S.scaffold(k, strs, recs, plinks, *params_of(par))
    S.check(k, strs, plinks, res, params_of(par)[4])
    return S.flat(res)


def same(got, exp, what):
    for a, b, part in zip(got[:5], exp[:5], PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"
    assert got[5] == exp[5], f"{what}: stats differ: {got[5]} != {exp[5]}"


def run_host(m, k, strs, plinks, urec=None, capacity=None, **par):
    mp, ra, inner, mn, mx = params_of(par)
    buf, off = R.join(strs)
    return m.unitig_scaffold_flat(k, buf, off, S.plinks_array(plinks), inner, mp, ra, mn, mx, urec=urec, capacity=capacity)


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def raw_dev(m, k, buf, off, plinks, cap, urec=None, n_plinks=None, sizing=False, **par):
    """one kmx_unitig_scaffold_dev call whose five outputs lie between guard bands of GUARD elements -> (rc, n_scaffolds, n_sbases,
    stats, the five outputs with their bands as NumPy arrays)"""
    import torch
    nu, nb = len(off) - 1, len(buf)
    pl = S.plinks_array(plinks) if isinstance(plinks, list) else plinks
    d_pl = to_dev(pl.view(np.uint8).reshape(-1, 32)) if len(pl) else None
    d_buf, d_off = to_dev(buf if nb else np.zeros(1, np.uint8)), to_dev(off, np.int64)
    d_urec = to_dev(urec.view(np.uint8).reshape(-1, 40)) if urec is not None else None
    sseq = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    soffs = torch.full((nu + 1 + 2 * GUARD,), -7, dtype=torch.int64, device="cuda")
    srec = torch.full((nu + 2 * GUARD, 64), 0xA5, dtype=torch.uint8, device="cuda")
    steps = torch.full((nu + 2 * GUARD, 16), 0xA5, dtype=torch.uint8, device="cuda")
    place = torch.full((nu + 2 * GUARD, 16), 0xA5, dtype=torch.uint8, device="cuda")
    p, st, ns, nsb = ScaffoldParams(*params_of(par), 0), ScaffoldStats(), C.c_uint64(0), C.c_uint64(0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = m.L.kmx_unitig_scaffold_dev(m.h, k, d_buf.data_ptr(), d_off.data_ptr(), nu, nb, ptr(d_urec), ptr(d_pl), len(pl) if n_plinks is None else n_plinks, C.byref(p),
                                     None if sizing else sseq[GUARD:].data_ptr(), 0 if sizing else cap, soffs[GUARD:].data_ptr(), srec[GUARD:].data_ptr(), steps[GUARD:].data_ptr(),
                                     place[GUARD:].data_ptr(), C.byref(ns), C.byref(nsb), C.byref(st))
    torch.cuda.synchronize()
    return rc, ns.value, nsb.value, st.as_dict(), tuple(t.cpu().numpy() for t in (sseq, soffs, srec, steps, place))


def bands_intact(out, cap, nu):
    sseq, soffs, srec, steps, place = out
    return (np.all(sseq[:GUARD] == 0xA5) and np.all(sseq[GUARD + cap:] == 0xA5) and np.all(soffs[:GUARD] == -7) and np.all(soffs[GUARD + nu + 1:] == -7) and
            all(np.all(t[:GUARD] == 0xA5) and np.all(t[GUARD + nu:] == 0xA5) for t in (srec, steps, place)))


def run_dev(m, k, strs, plinks, urec=None, capacity=None, **par):
    """-> the six parts as run_host gives them, from kmx_unitig_scaffold_dev between guard bands"""
    buf, off = R.join(strs)
    nu = len(strs)
    cap = len(buf) + max(nu - 1, 0) * params_of(par)[4] if capacity is None else capacity
    rc, ns, nsb, st, out = raw_dev(m, k, buf, off, plinks, cap, urec=urec, **par)
    if rc:
        raise KmxError(rc, m.L.kmx_last_error().decode(errors="replace"))
    assert bands_intact(out, cap, nu) and nsb <= cap
    sseq, soffs, srec, steps, place = out
    assert np.all(sseq[GUARD + nsb:GUARD + cap] == 0xA5) and np.all(srec[GUARD + ns:GUARD + nu] == 0xA5) and np.all(soffs[GUARD + ns + 1:GUARD + nu + 1] == -7)   # nothing behind what is promised
    return (sseq[GUARD:GUARD + nsb], soffs[GUARD:GUARD + ns + 1].view(np.uint64), srec[GUARD:GUARD + ns].reshape(-1).view(S.SCAFFOLD_DTYPE),
            steps[GUARD:GUARD + nu].reshape(-1).view(S.STEP_DTYPE), place[GUARD:GUARD + nu].reshape(-1).view(S.PLACE_DTYPE), st)


def both(m, k, strs, plinks, what, urec=None, recs=None, **par):
    exp = expected(k, strs, plinks, recs, **par)
    same(run_host(m, k, strs, plinks, urec, **par), exp, f"{what}: host")
    same(run_dev(m, k, strs, plinks, urec, **par), exp, f"{what}: device")
    return exp


# ---- the two islands, through the live session
def test_two_islands_through_the_live_session():
    """map, walks and pairs from the library, then the scaffold: the reverse complement of genome[:950] + 100 N + genome[1050:]"""
    k, km, cnt, strs, reads, rows, genome = P.case("two_islands")
    loff, lk = L.flat_links(rows)
    mm, md, bw, nb = P.READ_PARAMS
    m = KModel(1, 1023, NH, NB)
    m.unitig_map_begin(U.pack(km, k), k, *R.join(strs))
    rec, lst, st, _, _, _ = m.seq_to_pairs(reads, loff, lk, md, k, 0, mm, bw, nb)
    m.unitig_map_end()
    assert [tuple(int(x) for x in e) for e in lst] == [(1, 2, 101, 10100, 100, 100)] and np.all(rec["d"][rec["cls"] == P.SAME] == 221)
    plinks = [tuple(int(x) for x in e) for e in lst]
    exp = both(m, k, strs, plinks, "two islands", **S.TWO_ISLANDS_PARAMS)
    want = U.rc(genome[1050:]) + "N" * 100 + U.rc(genome[:950])
    assert exp[0].tobytes().decode() == want and len(want) == 2000
    sstrs, srec, steps, place, stt = m.scaffolds_from_pairs(k, strs, lst, **S.TWO_ISLANDS_PARAMS)
    assert sstrs == [want] and stt["n_chain"] == 1 and steps.tolist() == [(1, 0, 0), (2, 100, 100)] and place.tolist() == [(1, 0, 0), (0, 1, 1050)]


# ---- crafted lists over the pair tests' unitig set: U = 100, m_u in 1, 2, 7, 64, 300
@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 513))
def test_crafted_lists_at_the_block_edges(model, n):
    k, km, strs, mu = P.craft_set()
    urec, recs = recs_of(len(strs))
    plinks = S.random_list(n, 40 + n)
    for par in (dict(), dict(ratio=3), dict(min_pairs=41)):
        both(model, k, strs, plinks, f"{n} entries {par}", urec, recs, **par)
    both(model, k, strs, plinks, f"{n} entries without records", min_pairs=5, ratio=2)


@functools.lru_cache(maxsize=None)
def hub_set():
    return [U.rand_seq(P.K + (1, 0, 6)[u % 3], 5000 + u) for u in range(320)]


def test_a_hub_of_300_kept_links(model):
    """nk above 255 and 300 atomics on one word: out of one oriented unitig of a set of 320 (both forms), and over the set of 100
    with every edge out of it listed in both of its forms and twice (device form)"""
    k = P.K
    strs = hub_set()
    o = 2 * 7 + 1
    hub = sorted(P.canonical(o, 2 * (20 + i) + i % 2) + (2 + i % 5, 10 * (2 + i % 5), 10, 10) for i in range(300))
    for par in (dict(), dict(ratio=2)):
        exp = both(model, k, strs, hub, f"hub {par}", **par)
    assert exp[5]["n_below_ratio"] > 0 and exp[5]["n_chain"] == 0
    assert both(model, k, strs, sorted(hub + [(0, 2, 9, 90, 10, 10)]), "hub and one link")[5]["n_chain"] == 1
    k, km, cstrs, mu = P.craft_set()
    targets = [b for b in range(2 * len(cstrs)) if b >> 1 != 3][:150]
    lst = [(6, b, 3, 30, 10, 10) for b in targets] + [(b ^ 1, 7, 3, 30, 10, 10) for b in targets]      # 300 edges out of 6, each edge twice
    same(run_dev(model, k, cstrs, lst), expected(k, cstrs, lst), "hub over 100 unitigs")
    assert expected(k, cstrs, lst)[5]["n_kept"] == 300


@pytest.mark.parametrize("n", range(2, 10))
def test_chains_closed_into_cycles_of_every_length(model, n):
    k, km, strs, mu = P.craft_set()
    urec, recs = recs_of(len(strs))
    order = [17, 3, 44, 9, 60, 2, 71, 30, 5][:n]
    flips = [1, 0, 0, 1, 1, 0, 1, 0, 0][:n]
    for closed in (False, True):
        exp = both(model, k, strs, S.chain_list(order, flips, closed), f"{n} steps closed={closed}", urec, recs)
        assert exp[5]["n_circular"] == int(closed) and exp[5]["n_multi"] == 1
    two = S.chain_list(order, flips, True) + S.chain_list([80, 81, 82, 83][:max(2, n // 2)], [0, 1, 1, 0], True) + S.chain_list([90, 50, 91], [1, 1, 0], False)
    assert both(model, k, strs, sorted(two), f"two cycles and a path, {n}", urec, recs)[5]["n_circular"] == 2


def test_lists_that_are_not_canonical_or_hold_a_key_twice(model):
    """device form only: the host form refuses them"""
    k, km, strs, mu = P.craft_set()
    plinks = S.random_list(257, 5)
    mir = [S.mirrored(e) if i % 3 == 0 else e for i, e in enumerate(plinks)]
    random.Random(3).shuffle(mir)
    exp = expected(k, strs, plinks)
    got = run_dev(model, k, strs, mir)
    same(got, exp, "mirrored and shuffled")                       # consequence (b): nothing but which entry is counted
    chain = S.chain_list([5, 9, 13, 2], [0, 1, 0, 0], False, canonical=False)
    twice = chain + [chain[1]] + [S.mirrored(chain[2])]           # a key twice, and an edge in both of its forms: two edges each
    e2 = expected(k, strs, twice)
    assert e2[5]["n_chain"] == 1 and e2[5]["n_kept"] == 5
    same(run_dev(model, k, strs, twice), e2, "a key twice")
    with pytest.raises(KmxError) as e:
        run_host(model, k, strs, twice)
    assert e.value.code == -1


def test_the_ratio_at_its_threshold_and_the_gap_estimates(model):
    k, km, strs, mu = P.craft_set()
    at = [(0, 2, 4, 40, 10, 10), (0, 4, 12, 120, 10, 10)]
    below = [(0, 2, 4, 40, 10, 10), (0, 4, 13, 130, 10, 10)]
    assert both(model, k, strs, at, "n_pairs * ratio == best", ratio=3)[5]["n_kept"] == 2
    assert both(model, k, strs, below, "one below", ratio=3)[5]["n_below_ratio"] == 1
    big = [(0, 2, 2 ** 63, 2 ** 63, 1, 1), (4, 9, 1, 5, 0, 0)]
    exp = both(model, k, strs, big, "2^63 pairs", ratio=65536)
    assert exp[5]["n_chain"] == 1 and exp[2]["sum_pairs"][0] == 2 ** 63
    # est negative, inside [min_n, max_n] and above max_n; inner < D + 1; a distance that wraps; min_n = max_n = 0
    gaps = [(0, 2, 3, 3 * 290, 1, 1), (4, 6, 3, 3 * 200, 1, 1), (8, 10, 3, 3, 1, 1), (12, 14, 2, 2 * 5000, 1, 1), (16, 18, 1, 2 ** 64 - 1, 1, 1)]
    exp = both(model, k, strs, gaps, "gap estimates", min_pairs=1)
    assert sorted(exp[3]["est"][:10].tolist()) == [-4721, -11, 0, 0, 0, 0, 0, 79, 278, 280] and sorted(exp[3]["n_gap"][:10].tolist()) == [0, 0, 0, 0, 0, 3, 3, 79, 200, 200]
    exp = both(model, k, strs, gaps, "no N at all", min_pairs=1, min_n=0, max_n=0)
    assert exp[0].size == sum(map(len, strs)) and exp[5]["n_multi"] == 5
    both(model, k, strs, gaps, "inner = 0", min_pairs=1, inner=0)
    both(model, k, strs, gaps, "the largest inner and max_n", min_pairs=1, inner=2 ** 32 - 1, min_n=0, max_n=100000)


# ---- one deep chain
@pytest.mark.parametrize("closed", (False, True))
def test_one_deep_chain(model, closed):
    """100 000 unitigs of k + 2 bytes in shuffled order and random orientation as one path and as one cycle: 17 doubling rounds or
    more, and as many again behind the cut"""
    k, n = 21, 100000
    strs, plinks = S.deep_chain(n, k, closed)
    par = dict(inner=100, min_n=0, max_n=40)
    exp = both(model, k, strs, plinks, f"deep chain closed={closed}", **par)
    assert exp[5]["n_scaffolds"] == 1 and exp[5]["n_chain"] == n - (0 if closed else 1) and exp[5]["n_circular"] == int(closed)
    assert model.unitig_scaffold_phases()["rounds"] >= (34 if closed else 17)


# ---- the densest tile
@functools.lru_cache(maxsize=None)
def dense_case():
    """k = 5: 3000 unitigs of exactly 5 bytes chained in index order, half of them reversed, the N in front cycling through 0, 1,
    15, 16, 17; behind them short, long reversed (more than two tiles), short, long forward, short"""
    k, inner = 5, 100
    r = random.Random(8)
    strs = [U.rand_seq(5, 9000 + u) for u in range(3000)] + [U.rand_seq(n, 9900 + n) for n in (5, 9001, 6, 8200, 5)]
    gap = lambda i: (0, 1, 15, 16, 17)[i % 5]
    flips = [r.randrange(2) for _ in range(3000)]
    plinks = []
    for i in range(2999):
        a, b = P.canonical(2 * i + flips[i], 2 * (i + 1) + flips[i + 1])
        plinks.append((a, b, 2, 2 * (inner - 5 - gap(i)), 0, 0))
    for i, (da, db) in enumerate(((0, 1), (1, 0), (0, 0), (0, 1))):
        a, b = P.canonical(2 * (3000 + i) + da, 2 * (3001 + i) + db)
        plinks.append((a, b, 2, 2 * (inner - 5 - gap(i + 2)), 0, 0))
    return k, strs, sorted(plinks), dict(inner=inner, min_n=0, max_n=17)


def test_the_densest_tile_and_every_alignment(model):
    k, strs, plinks, par = dense_case()
    exp = both(model, k, strs, plinks, "dense", **par)
    assert exp[5]["n_scaffolds"] == 2 and sorted(set(exp[3]["n_gap"].tolist())) == [0, 1, 15, 16, 17] and 1000 < int((exp[3]["o"] & 1).sum()) < 2000
    assert {int(x) % 16 for x in exp[4]["off"]} == set(range(16))   # every destination alignment
    buf, off = R.join(strs)                                       # ... and with the buffers themselves off the 16-byte grid
    import torch
    d = torch.zeros(len(buf) + 3, dtype=torch.uint8, device="cuda")
    d[3:] = to_dev(buf)
    out = torch.full((len(exp[0]) + 5 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")
    o5 = (out[5:5 + len(exp[0])], torch.zeros(len(strs) + 1, dtype=torch.int64, device="cuda"), z(len(strs), 64), z(len(strs), 16), z(len(strs), 16))
    mp, ra, inner, mn, mx = params_of(par)
    _, (ns, nsb), st = model.unitig_scaffold_dev(k, d[3:], to_dev(off, np.int64), to_dev(S.plinks_array(plinks).view(np.uint8).reshape(-1, 32)), len(plinks), inner, mp, ra, mn, mx, out=o5)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[5:5 + nsb].tobytes() == exp[0].tobytes() and np.all(got[:5] == 0xA5) and np.all(got[5 + nsb:] == 0xA5) and st == exp[5]


# ---- KMX_E_RANGE and the sizing call
def test_range_and_the_sizing_call(model):
    k, km, strs, mu = P.craft_set()
    plinks = S.random_list(257, 297)
    exp = expected(k, strs, plinks)
    need, nu = exp[0].size, len(strs)
    buf, off = R.join(strs)
    assert need > len(buf)
    rc, ns, nsb, st, out = raw_dev(model, k, buf, off, plinks, need)          # exact
    assert rc == 0 and nsb == need and out[0][GUARD:GUARD + need].tobytes() == exp[0].tobytes() and bands_intact(out, need, nu)
    for cap, sizing in ((need - 1, False), (0, True), (len(buf), False)):
        rc, ns, nsb, st, out = raw_dev(model, k, buf, off, plinks, cap, sizing=sizing)
        assert rc == -5 and nsb == need and ns == len(exp[1]) - 1 and st == exp[5]
        assert np.all(out[0] == 0xA5) and bands_intact(out, cap, nu)          # not one base is written
        got = (None, out[1][GUARD:GUARD + ns + 1].view(np.uint64), out[2][GUARD:GUARD + ns], out[3][GUARD:GUARD + nu], out[4][GUARD:GUARD + nu])
        for a, b, part in list(zip(got, exp, PARTS))[1:]:
            assert a.tobytes() == b.tobytes(), f"short by design: {part} differ"
    for cap in (need - 1, 0):
        with pytest.raises(KmxError) as e:
            run_host(model, k, strs, plinks, capacity=cap)
        assert e.value.code == -5 and e.value.needed == need
        soffs, srec, steps, place, stt = e.value.result
        assert soffs.tobytes() == exp[1].tobytes() and srec.tobytes() == exp[2].tobytes() and steps.tobytes() == exp[3].tobytes() and place.tobytes() == exp[4].tobytes() and stt == exp[5]
    same(run_host(model, k, strs, plinks, capacity=need), exp, "exact capacity: host")


# ---- refusals
def test_refusals(model):
    """KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31, n_plinks >= 2^31, ratio > 65536, min_n > max_n,
    reserved != 0, a NULL required buffer, an output that overlaps another buffer; in the host form also bad uoffsets, a unitig
    shorter than k and a list that is not strictly ascending; the handle then answers as if nothing had happened"""
    import torch
    m = model
    k, km, strs, mu = P.craft_set()
    plinks = S.random_list(255, 255)
    exp = expected(k, strs, plinks)
    buf, off = R.join(strs)
    nu, nb, cap = len(strs), len(buf), len(buf) + 99 * 200
    pl = S.plinks_array(plinks)
    sseq, soffs, srec, steps, place = np.zeros(cap, np.uint8), np.zeros(nu + 1, np.uint64), np.zeros(nu, S.SCAFFOLD_DTYPE), np.zeros(nu, S.STEP_DTYPE), np.zeros(nu, S.PLACE_DTYPE)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def host_rc(kk=k, b=buf, o=off, n=nu, lst=pl, n_pl=None, par=(2, 0, 300, 3, 200, 0), ss=sseq, c=cap, so=soffs, sr=srec, stp=steps, plc=place, counts=True, stats=True):
        p, st, ns, nsb = ScaffoldParams(*par) if par else None, ScaffoldStats(), C.c_uint64(0), C.c_uint64(0)
        return m.L.kmx_unitig_scaffold(m.h, kk, ptr(b), ptr(o), n, None, ptr(lst), len(pl) if n_pl is None else n_pl, C.byref(p) if par else None, ptr(ss), c, ptr(so), ptr(sr), ptr(stp), ptr(plc),
                                       C.byref(ns) if counts else None, C.byref(nsb), C.byref(st) if stats else None)

    d = {name: to_dev(a if a.dtype != np.uint64 else a.view(np.int64)) for name, a in (("buf", buf), ("off", off), ("pl", pl.view(np.uint8)), ("sseq", sseq), ("soffs", soffs),
                                                                                          ("srec", srec.view(np.uint8)), ("steps", steps.view(np.uint8)), ("place", place.view(np.uint8)))}

    def dev_rc(kk=k, n=nu, n_pl=len(pl), par=(2, 0, 300, 3, 200, 0), c=cap, **swap):
        t = dict(d, **swap)
        g = lambda name: t[name].data_ptr() if t[name] is not None else None
        p, st, ns, nsb = ScaffoldParams(*par), ScaffoldStats(), C.c_uint64(0), C.c_uint64(0)
        return m.L.kmx_unitig_scaffold_dev(m.h, kk, g("buf"), g("off"), n, nb, None, g("pl"), n_pl, C.byref(p), g("sseq"), c, g("soffs"), g("srec"), g("steps"), g("place"), C.byref(ns), C.byref(nsb),
                                           C.byref(st))

    assert host_rc() == 0 and dev_rc() == 0
    for kk in (20, 3, 65):
        assert host_rc(kk=kk) == -1 and dev_rc(kk=kk) == -1
    assert dev_rc(n=2 ** 31) == -1 and dev_rc(n_pl=2 ** 31) == -1 and host_rc(n_pl=2 ** 31) == -1
    for par in ((2, 65537, 300, 3, 200, 0), (2, 0, 300, 201, 200, 0), (2, 0, 300, 3, 200, 1)):
        assert host_rc(par=par) == -1 and dev_rc(par=par) == -1
    assert host_rc(par=None) == -1 and host_rc(counts=False) == -1 and host_rc(stats=False) == -1
    for name in ("b", "o", "lst", "ss", "so", "sr", "stp", "plc"):
        assert host_rc(**{name: None}) == -1, name
    for name in ("buf", "off", "pl", "sseq", "soffs", "srec", "steps", "place"):
        assert dev_rc(**{name: None}) == -1, name
    assert host_rc(ss=buf, c=nb) == -1 and host_rc(so=off) == -1 and host_rc(sr=sseq[:nu * 64].view(S.SCAFFOLD_DTYPE)) == -1 and host_rc(stp=place.view(S.STEP_DTYPE)) == -1   # overlaps
    assert dev_rc(sseq=d["buf"], c=nb) == -1 and dev_rc(steps=d["place"]) == -1
    swapped, above, short = off.copy(), off.copy(), off.copy()
    swapped[3], swapped[4] = off[4] + 1, off[3]
    above[0] = 1
    short[1:] -= np.uint64(1)                                     # unitig 0 has k - 1 bytes
    for bad in (swapped, above, short):
        assert host_rc(o=bad) == -1
    for bad in ([(4, 9, 1, 1, 1, 1), (4, 9, 1, 1, 1, 1)], [(4, 9, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)], [(5, 0, 1, 1, 1, 1), (4, 8, 1, 1, 1, 1)]):
        assert host_rc(lst=S.plinks_array(bad), n_pl=2) == -1
    # U == 0: KMX_OK, soffsets[0] = 0, all counts zero but the entries, which are all ignored
    p, st, ns, nsb = ScaffoldParams(2, 0, 300, 3, 200, 0), ScaffoldStats(), C.c_uint64(9), C.c_uint64(9)
    so = np.full(1, 77, np.uint64)
    assert m.L.kmx_unitig_scaffold(m.h, k, None, so.ctypes.data, 0, None, pl.ctypes.data, 3, C.byref(p), None, 0, so.ctypes.data, None, None, None, C.byref(ns), C.byref(nsb), C.byref(st)) == -1   # soffsets over uoffsets
    zero = np.zeros(1, np.uint64)
    assert m.L.kmx_unitig_scaffold(m.h, k, None, zero.ctypes.data, 0, None, pl.ctypes.data, 3, C.byref(p), None, 0, so.ctypes.data, None, None, None, C.byref(ns), C.byref(nsb), C.byref(st)) == 0
    assert so[0] == 0 and ns.value == nsb.value == 0 and st.as_dict() == dict(dict.fromkeys(S.STAT_FIELDS, 0), n_entries=3, n_ignored=3)
    d_so = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    assert m.L.kmx_unitig_scaffold_dev(m.h, k, None, d["off"].data_ptr(), 0, 0, None, None, 0, C.byref(p), None, 0, d_so.data_ptr(), None, None, None, C.byref(ns), C.byref(nsb), C.byref(st)) == 0
    assert int(d_so.cpu()[0]) == 0
    same(run_host(m, k, strs, plinks), exp, "after the refusals: host")
    same(run_dev(m, k, strs, plinks), exp, "after the refusals: device")


# ---- crafted device input between guard bands
def test_crafted_device_input_stays_inside_the_buffers(model):
    """the _dev form clamps: a, b >= 2 U, a >> 1 == b >> 1 and n_pairs = 0 are ignored; offsets beyond n_ubases, decreasing, all ones
    and all zero give wrong scaffolds: KMX_OK or KMX_E_RANGE, and the guard bands around the five outputs are intact"""
    m = model
    k, km, strs, mu = P.craft_set()
    buf, off = R.join(strs)
    nu, nb = len(strs), len(buf)
    good = S.random_list(513, 13)
    pl = S.plinks_array(good)
    r = np.random.RandomState(4)
    big = np.uint64(2 ** 64 - 1)
    bad_lists = []
    for f, v in (("a", 2 * nu + r.randint(0, 9, len(pl))), ("b", np.full(len(pl), 0xFFFFFFFF)), ("n_pairs", np.zeros(len(pl))), ("b", pl["a"] ^ np.uint32(1)), ("sum_dist", np.full(len(pl), big)),
                 ("n_pairs", np.full(len(pl), big))):
        x = pl.copy()
        x[f] = np.where(np.arange(len(pl)) % 2 == 0, v, x[f]).astype(x[f].dtype)
        bad_lists.append(x)
    exp_ignored = expected(k, strs, [tuple(int(t) for t in e) for e in bad_lists[0]])
    cap = nb + (nu - 1) * 200
    for i, x in enumerate(bad_lists):
        rc, ns, nsb, st, out = raw_dev(m, k, buf, off, x, cap)
        assert rc == 0 and bands_intact(out, cap, nu) and st["n_entries"] == len(pl) and st["n_links"] + st["n_ignored"] == len(pl), i
        if i < 4:
            assert st["n_ignored"] == (len(pl) + 1) // 2, i
    rc, ns, nsb, st, out = raw_dev(m, k, buf, off, bad_lists[0], cap)
    assert st == exp_ignored[5] and out[0][GUARD:GUARD + nsb].tobytes() == exp_ignored[0].tobytes()     # ignored entries change nothing else
    bad_offs = [off[::-1].copy(), off + np.uint64(nb), np.full(len(off), big), np.zeros(len(off), np.uint64), np.where(np.arange(len(off)) % 2 == 1, big, off), off * np.uint64(3)]
    for i, o in enumerate(bad_offs):
        for lst in (pl, bad_lists[0]):
            rc, ns, nsb, st, out = raw_dev(m, k, buf, o, lst, cap)
            assert rc in (0, -5) and ns <= nu and bands_intact(out, cap, nu), i
            assert rc == 0 or np.all(out[0] == 0xA5)
    rc, ns, nsb, st, out = raw_dev(m, k, buf, off, pl, cap, n_plinks=len(pl) - 100)     # a shorter count reads a shorter list
    exp = expected(k, strs, good[:-100])
    assert rc == 0 and st == exp[5] and out[0][GUARD:GUARD + nsb].tobytes() == exp[0].tobytes()
    same(run_dev(m, k, strs, good), expected(k, strs, good), "after the crafted input")


# ---- allocation failures
def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first scaffold call in turn, host and device form: the same call then succeeds with the
    right bytes"""
    k, km, strs, mu = P.craft_set()
    chain = S.chain_list([17, 3, 44, 9], [1, 0, 0, 1], True)
    plinks = sorted(chain + [e for e in S.random_list(50, 2)[40:] if e[:2] not in {c[:2] for c in chain}])
    exp = expected(k, strs, plinks)
    failed = {"host": 0, "dev": 0}
    run = {"host": run_host, "dev": run_dev}
    for nth in range(1, 24):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run[variant](m, k, strs, plinks)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run[variant](m, k, strs, plinks), exp, f"after allocation {nth} failed, {variant}")
    assert failed["host"] >= 15 and failed["dev"] >= 8, failed


# ---- the facade and the driver
def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_scaffold.cpp prints the stats and the three texts for the two islands; the driver's -u1 -M -W -P400 -S2
    writes scaffolds.fa, scaffolds.paths.tsv and scaffolds.agp, from the unitigs and, with -X1, from the contigs: all equal the
    restatement's text, and every other output stays as it is without -S"""
    import count_reads as CR
    k, km, cnt, strs, reads, rows, genome = P.case("two_islands")
    _, _, plinks, _ = S.two_islands()
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

    q = S.TWO_ISLANDS_PARAMS
    res = S.scaffold(k, strs, None, plinks, q["min_pairs"], q["ratio"], q["inner"], q["min_n"], q["max_n"])
    exe = build("tests/facade_unitig_scaffold.cpp", "facade_unitig_scaffold")
    out = subprocess.check_output([exe, fa, str(k), "1", lines, "1", str(P.MAX_DIST), str(q["min_pairs"]), str(q["ratio"]), str(q["inner"]), str(q["min_n"]), str(q["max_n"])], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 4 and blocks[0] == " ".join(str(res["stats"][f]) for f in S.STAT_FIELDS) + "\n"
    assert blocks[1] == S.fasta(res) and blocks[2] == S.paths_tsv(res) and blocks[3] == S.agp(res, strs)
    # the driver: inner is the floor of the mean d of the pairs on one unitig (221 for every one), min_n = 10, max_n = 2 max_dist
    res = S.scaffold(k, strs, None, plinks, 2, 0, 221, 10, 2 * P.MAX_DIST)
    assert res["sstrs"] == [U.rc(genome[1050:]) + "N" * 100 + U.rc(genome[:950])]
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    base = ["-g", "-u1", "-M", "-W", f"-P{P.MAX_DIST}", f"-k{k}", "-nh3", "-nb2"]
    names = ("scaffolds.fa", "scaffolds.paths.tsv", "scaffolds.agp")
    want = (S.fasta(res), S.paths_tsv(res), S.agp(res, strs))
    before = {}
    for extra, what in (((), "unitigs"), (("-X1",), "contigs")):
        work = tmp_path / f"plain_{what}"
        work.mkdir()
        subprocess.check_call([exe, *base, *extra, fa, "db", str(work)], stdout=subprocess.DEVNULL, timeout=120)
        texts = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix in (".fa", ".tsv", ".gaf", ".gfa", ".agp")}
        before[what] = texts(work / "db")
        assert not any(n in before[what] for n in names)
        work = tmp_path / f"scaf_{what}"
        work.mkdir()
        log = subprocess.check_output([exe, *base, *extra, "-S2", fa, "db", str(work)], timeout=120).decode()
        after = texts(work / "db")
        assert len(before[what]) >= 7
        assert tuple(after[n].decode() for n in names) == want, what
        assert {n: b for n, b in after.items() if n not in names} == before[what], what        # every existing output byte for byte
        assert f"scaffolds of {what} (links of >= 2 pairs, inner 221) :     1 scaffolds (1 of several, 0 circular), 1 of 1 links joined, 100 N" in log
    assert subprocess.call([exe, "-g", "-u1", "-M", "-W", "-S2", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2                    # -S without -P
    assert subprocess.call([exe, *base, "-X1", "-R2", "-S2", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2                                   # -S with -R
    assert subprocess.call([exe, *base, "-S", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2 and subprocess.call([exe, *base, "-S2,70000", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
