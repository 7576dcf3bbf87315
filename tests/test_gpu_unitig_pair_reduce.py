"""kmx_unitig_pair_reduce* on the MI355X: the records, the list that stays, origin, n_out and stats equal, byte for byte, what the
plain-Python restatement of the rule (tests/unitig_pair_reduce_ref.py) gives, for the host and the device form (the device form
always between guard bands): line lists at the group and block edges of both per-entry kernels, max_row around a hub's degree at
the edges of the 8-lane stride, both sides and r_a == r_c, a witness in both orientations, lists only the device form takes,
wrapping arithmetic, KMX_E_RANGE and the sizing call, the empty inputs, the refusals, the acceptance case into
kmx_unitig_scaffold_dev, a handle used twice, the facade and the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import unitig_map_ref as R
import unitig_pair_reduce_ref as X
import unitig_pairs_ref as P
import unitig_scaffold_ref as S
from kmcex_amd import KModel
from kmcex_amd.api import KmxError, PairReduceParams, PairReduceStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the list
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
K = X.LINE_K
PARTS = ("rrecs", "lout", "origin")
LINE_SIZES = (1, 2, 3, 31, 32, 33, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def model():
    return KModel(1, 1023, NH, NB)


def offsets_of(mu, k=K):
    return np.cumsum([0] + [m + k - 1 for m in mu], dtype=np.uint64).astype(np.uint64)


def params_of(par):
    q = dict(X.PAR, **par)
    return q["min_pairs"], q["inner"], q["tol"], q["max_row"]


def expected(mu, plinks, checked=True, **par):
    q = dict(X.PAR, **par)
    return X.flat(X.check(mu, plinks, q) if checked else X.reduce(mu, plinks, **q))


def same(got, exp, what):
    for a, b, part in zip(got[:3], exp[:3], PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"
    assert got[3] == exp[3], f"{what}: n_out {got[3]} != {exp[3]}"
    assert [got[4][f] for f in X.STAT_FIELDS] == list(exp[4]), f"{what}: stats differ: {got[4]} != {list(exp[4])}"


def run_host(m, mu, plinks, capacity=None, k=K, **par):
    mp, inner, tol, mr = params_of(par)
    rec, lout, org, st = m.unitig_pair_reduce_flat(k, offsets_of(mu, k), X.plinks_array(plinks), inner, tol, mp, mr, capacity=capacity)
    return rec, lout, org, len(lout), st


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def raw_dev(m, mu, plinks, cap, k=K, lists=True, n_ubases=None, **par):
    """one kmx_unitig_pair_reduce_dev call whose three outputs lie between guard bands of GUARD elements -> (rc, n_out, stats, the
    three outputs with their bands as NumPy arrays)"""
    import torch
    off = offsets_of(mu, k)
    pl = X.plinks_array(plinks)
    n = len(pl)
    d_pl = to_dev(pl.view(np.uint8).reshape(-1, 32)) if n else None
    d_off = to_dev(off, np.int64)
    rrecs = torch.full((n + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    lout = torch.full((cap + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    org = torch.full((cap + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    p, st, no = PairReduceParams(*params_of(par), 0), PairReduceStats(), C.c_uint64(0)
    rc = m.L.kmx_unitig_pair_reduce_dev(m.h, k, d_off.data_ptr(), len(mu), int(off[-1]) if n_ubases is None else n_ubases, d_pl.data_ptr() if n else None, n, C.byref(p), rrecs[GUARD:].data_ptr(),
                                        lout[GUARD:].data_ptr() if lists else None, org[GUARD:].data_ptr() if lists else None, cap if lists else 0, C.byref(no), C.byref(st))
    torch.cuda.synchronize()
    return rc, no.value, st.as_dict(), tuple(x.cpu().numpy() for x in (rrecs, lout, org))


def bands_intact(out, n, cap):
    rrecs, lout, org = out
    return (np.all(rrecs[:GUARD] == 0xA5) and np.all(rrecs[GUARD + n:] == 0xA5) and np.all(lout[:GUARD] == 0xA5) and np.all(lout[GUARD + cap:] == 0xA5) and
            np.all(org[:GUARD] == -7) and np.all(org[GUARD + cap:] == -7))


def run_dev(m, mu, plinks, capacity=None, k=K, **par):
    """-> the five parts as run_host gives them, from kmx_unitig_pair_reduce_dev between guard bands"""
    n = len(plinks)
    cap = n if capacity is None else capacity
    rc, no, st, out = raw_dev(m, mu, plinks, cap, k, **par)
    if rc:
        raise KmxError(rc, m.L.kmx_last_error().decode(errors="replace"))
    assert bands_intact(out, n, cap) and no <= cap
    rrecs, lout, org = out
    assert np.all(lout[GUARD + no:GUARD + cap] == 0xA5) and np.all(org[GUARD + no:GUARD + cap] == -7)   # nothing behind what is promised
    return rrecs[GUARD:GUARD + n].reshape(-1).view(X.PAIR_REDUCE_DTYPE), lout[GUARD:GUARD + no].reshape(-1).view(P.PAIR_LINK_DTYPE), org[GUARD:GUARD + no].view(np.uint32), no, st


def both(m, mu, plinks, what, checked=True, **par):
    exp = expected(mu, plinks, checked, **par)
    same(run_host(m, mu, plinks, **par), exp, f"{what}: host")
    same(run_dev(m, mu, plinks, **par), exp, f"{what}: device")
    return exp


# ---- the rule against the restatement
def test_line_lists_at_the_group_and_block_edges(model):
    for n in LINE_SIZES:
        mu, pl = X.line_list(n, 3, 1)
        for tol in (0, 1):
            exp = both(model, mu, pl, f"line {n} tol {tol}", tol=tol)
        assert n < 31 or (exp[0]["verdict"] == X.TRANSITIVE).sum() * 10 >= n       # the lists do hold what the call is about


@pytest.mark.parametrize("deg", (7, 8, 9, 65))
def test_max_row_around_a_hubs_degree(model, deg):
    mu, pl, i = X.hub_list(deg)
    for mr, verdict in ((deg - 1, X.COMPLEX), (deg, X.TRANSITIVE), (deg + 1, X.TRANSITIVE)):
        exp = both(model, mu, pl, f"hub {deg} max_row {mr}", inner=2000, tol=1, max_row=mr)
        assert exp[0]["verdict"][i] == verdict and exp[0]["side"][i] == 0 and (verdict == X.COMPLEX or exp[0]["n_via"][i] >= 3)


def test_both_sides_and_equal_rows(model):
    """a hub at a with a short row at c ^ 1, the reverse, and r_a == r_c: the enumerated side is the restatement's"""
    for extra_a, extra_c, side in ((20, 0, 1), (0, 20, 0), (0, 0, 0), (3, 3, 0)):
        mu, pl, i = X.hub_list(6, extra_a, extra_c)
        exp = both(model, mu, pl, f"sides {extra_a} {extra_c}", inner=2000, tol=2, max_row=64)
        assert exp[0]["side"][i] == side and exp[0]["verdict"][i] == X.TRANSITIVE and exp[0]["n_via"][i] == 5
    mu, pl, i = X.hub_list(40, 30, 0)                              # the longer side is above max_row, the shorter one is not
    exp = both(model, mu, pl, "long side over max_row", inner=2000, tol=0, max_row=40)
    assert exp[0]["side"][i] == 1 and exp[0]["verdict"][i] == X.TRANSITIVE


def both_orientations():
    """A -> C over unitig 2 in both orientations; over 4 + and 5 -, of which only one fits"""
    mu = [30, 40, 17, 9, 12]
    inner, G = 2000, 500
    pl = [X.entry(0, 2, G, inner)]
    for o, err in ((4, 0), (5, 0), (6, 3), (7, 0), (9, 9)):
        pl += [X.entry(0, o, 7, inner), X.entry(o, 2, G - 7 - mu[o >> 1] + err, inner)]
    return mu, sorted(pl), inner


def test_a_witness_in_both_orientations(model):
    mu, pl, inner = both_orientations()
    exp = both(model, mu, pl, "both orientations", inner=inner, tol=0)
    i = [e[:2] for e in pl].index(P.canonical(0, 2))
    assert (exp[0]["verdict"][i], exp[0]["via"][i], exp[0]["n_via"][i]) == (X.TRANSITIVE, 4, 3)


def test_delta_at_the_tolerance(model):
    for err, tol, verdict in ((5, 5, X.TRANSITIVE), (-5, 5, X.TRANSITIVE), (6, 5, X.KEPT), (-6, 5, X.KEPT), (0, 0, X.TRANSITIVE), (1, 0, X.KEPT)):
        mu, pl, i = X.hub_list(2, errs=(err,))
        exp = both(model, mu, pl, f"delta {err} tol {tol}", inner=2000, tol=tol)
        assert exp[0]["verdict"][i] == verdict and (verdict == X.KEPT or exp[0]["delta"][i] == -err)


def test_wrapping_arithmetic(model):
    """sum_dist near 2^63 and inner = 2^32 - 1: g and delta wrap as the restatement's do"""
    mu = [30, 40, 17]
    big = 2 ** 63 - 5
    pl = sorted([(0, 2, 1, big, 0, 0), (0, 4, 1, 2 ** 64 - 1, 0, 0), (4, 2, 2, 2 ** 64 - 2, 0, 0), (1, 5, 3, 7, 0, 0)])
    for inner, tol in ((2 ** 32 - 1, 2 ** 32 - 1), (0, 0), (2 ** 32 - 1, 0)):
        both(model, mu, pl, f"wrapping inner {inner}", min_pairs=1, inner=inner, tol=tol)
    inner, d = 2 ** 32 - 1, 2 ** 63 - 10                           # g(a -> b) + g(b -> c) wraps, and the sum meets g(a -> c) exactly
    pl = sorted([(0, 4, 1, d, 0, 0), (4, 2, 1, d, 0, 0), (0, 2, 1, (2 * d - (inner - 1) - mu[2]) % 2 ** 64, 0, 0)])
    for tol, verdict in ((0, X.TRANSITIVE), (3, X.TRANSITIVE)):
        exp = both(model, mu, pl, "a witness across the wrap", min_pairs=1, inner=inner, tol=tol)
        assert exp[0]["verdict"][0] == verdict and exp[0]["delta"][0] == 0
    pl[0] = pl[0][:3] + (pl[0][3] + 4,) + pl[0][4:]
    assert both(model, mu, pl, "a miss across the wrap", min_pairs=1, inner=inner, tol=3)[0]["verdict"][0] == X.KEPT


def test_ignored_and_below_min_entries_are_no_witnesses(model):
    mu, pl = X.line_list(40, 1, 1)
    nu = len(mu)
    keys = {e[:2] for e in pl}
    free = next((a, b) for a in range(2 * nu) for b in range(2 * nu) if a >> 1 != b >> 1 and (a, b) not in keys)
    pl = sorted(pl + [(2 * nu, 3, 5, 50, 10, 10), (4, 5, 9, 90, 10, 10), (6, 2 * nu + 7, 2, 20, 10, 10), free + (0, 0, 0, 0)])
    exp = both(model, mu, pl, "ignored and below min", checked=False, min_pairs=4, tol=1)
    assert exp[4][1] == 4 and exp[4][2] > 0 and exp[4][4] > 0


# ---- what only the device form takes
def test_device_lists_that_are_not_canonical(model):
    mu, pl = X.line_list(257, 3, 1)
    r = np.random.default_rng(5)
    dup = pl + [pl[i] for i in r.integers(0, len(pl), 40)] + [(e[0], e[1], e[2] + 1, e[3] + 3, e[4], e[5]) for e in pl[::9]]
    shuffled = [pl[i] for i in r.permutation(len(pl))]
    with_mirrors = sorted(pl + [X.mirrored(e) for e in pl[::3]])
    for what, lst in (("duplicate keys", sorted(dup)), ("not ascending", shuffled), ("an entry beside its mirror", with_mirrors), ("all three", [dup[i] for i in r.permutation(len(dup))] + with_mirrors)):
        exp = expected(mu, lst, checked=False, tol=1)
        same(run_dev(model, mu, lst, tol=1), exp, what)
        assert (exp[0]["verdict"] == X.TRANSITIVE).any()


def test_device_offsets_are_clamped(model):
    """offsets beyond n_ubases: m_u comes from the clamped values, and nothing is read or written outside a buffer"""
    mu, pl = X.line_list(33, 3, 1)
    off = offsets_of(mu)
    cut = int(off[len(mu) // 2])
    clamped = [max(int(min(off[u + 1], cut)) - int(min(off[u], cut)) - K + 1, 0) for u in range(len(mu))]
    exp = expected(clamped, pl, checked=False, tol=1)
    rc, no, st, out = raw_dev(model, mu, pl, len(pl), n_ubases=cut, tol=1)
    assert rc == 0 and bands_intact(out, len(pl), len(pl))
    assert out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and no == exp[3]


# ---- capacities and empty inputs
def test_range_leaves_the_list_untouched_and_the_handle_usable(model):
    mu, pl = X.line_list(256, 3, 1)
    exp = expected(mu, pl, tol=1)
    n_out = exp[3]
    assert 0 < n_out < len(pl)
    with pytest.raises(KmxError) as e:
        run_host(model, mu, pl, capacity=n_out - 1, tol=1)
    assert e.value.code == -5 and e.value.needed == n_out and e.value.result[0].tobytes() == exp[0].tobytes() and [e.value.result[1][f] for f in X.STAT_FIELDS] == list(exp[4])
    rc, no, st, out = raw_dev(model, mu, pl, n_out - 1, tol=1)
    assert rc == -5 and no == n_out and [st[f] for f in X.STAT_FIELDS] == list(exp[4])
    assert out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and np.all(out[1] == 0xA5) and np.all(out[2] == -7)
    same(run_dev(model, mu, pl, capacity=n_out, tol=1), exp, "the exact capacity")
    same(run_host(model, mu, pl, capacity=n_out, tol=1), exp, "the exact capacity: host")
    # the sizing call: no list, the verdicts and n_out only
    rc, no, st, out = raw_dev(model, mu, pl, 0, lists=False, tol=1)
    assert rc == 0 and no == n_out and out[0][GUARD:GUARD + len(pl)].tobytes() == exp[0].tobytes() and bands_intact(out, len(pl), 0)
    rec, lout, org, st = model.unitig_pair_reduce_flat(K, offsets_of(mu), X.plinks_array(pl), X.PAR["inner"], 1, lists=False)
    assert lout is None and org is None and rec.tobytes() == exp[0].tobytes() and st["n_out"] == n_out


def test_no_unitig_and_no_entry(model):
    mu, pl = X.line_list(33, 3, 1)
    exp = both(model, [], pl, "U == 0")
    assert exp[4][1] == len(pl) and exp[1].tobytes() == X.plinks_array(pl).tobytes() and np.all(exp[0]["via"] == X.NO_VIA)
    exp = both(model, mu, [], "n_plinks == 0")
    assert not exp[4].any() and exp[3] == 0
    both(model, [], [], "nothing at all")


def test_consequence_a_on_the_device(model):
    mu, pl = X.line_list(257, 3, 1)
    exp = both(model, mu, pl, "min_pairs above every entry", min_pairs=10, tol=40)
    assert exp[1].tobytes() == X.plinks_array(pl).tobytes() and exp[4][2] == len(pl)


# ---- the refusals
def test_bad_arguments_are_refused_before_anything_runs(model):
    import torch
    m = model
    mu, pl = X.line_list(33, 3, 1)
    off, arr = offsets_of(mu), X.plinks_array(pl)
    n, nu = len(arr), len(mu)
    rec = np.full(n, 0x5A, dtype=np.uint8).repeat(32).view(X.PAIR_REDUCE_DTYPE)
    lout, org = np.zeros(n, dtype=P.PAIR_LINK_DTYPE), np.zeros(n, dtype=np.uint32)
    st, no = PairReduceStats(), C.c_uint64(0)
    good = PairReduceParams(2, 600, 1, 64, 0)

    def host(k=K, off=off, nu=nu, arr=arr, n=n, par=good, rec=rec, lout=lout, org=org, cap=n, no=no, st=st, pl_ptr=None):
        p = lambda a: a.ctypes.data if a is not None else None
        return m.L.kmx_unitig_pair_reduce(m.h, k, p(off), nu, p(arr) if pl_ptr is None else pl_ptr, n, C.byref(par) if par is not None else None, p(rec), p(lout), p(org), cap,
                                          C.byref(no) if no is not None else None, C.byref(st) if st is not None else None)

    assert host() == 0
    rec[:] = np.full(n, 0x5A, dtype=np.uint8).repeat(32).view(X.PAIR_REDUCE_DTYPE)
    bad_off, short = off.copy(), off.copy()
    bad_off[3] = bad_off[2] - 1 if bad_off[2] else 0
    bad_off[0] = 1
    short[1:] -= off[1] - np.uint64(K - 1)                       # the first unitig has k - 1 bytes
    unsorted = arr[::-1].copy()
    overlap = rec.view(np.uint8)[:n * 4].view(np.uint32)
    cases = dict(even_k=dict(k=20), small_k=dict(k=3), large_k=dict(k=65), many_unitigs=dict(nu=2 ** 31), many_entries=dict(n=2 ** 31), max_row_0=dict(par=PairReduceParams(2, 600, 1, 0, 0)),
                 max_row_big=dict(par=PairReduceParams(2, 600, 1, 65537, 0)), reserved=dict(par=PairReduceParams(2, 600, 1, 64, 1)), null_params=dict(par=None), null_n_out=dict(no=None),
                 null_stats=dict(st=None), null_rrecs=dict(rec=None), null_uoffsets=dict(off=None), null_plinks=dict(arr=None), overlap=dict(org=overlap), in_out_overlap=dict(pl_ptr=lout.ctypes.data),
                 bad_offsets=dict(off=bad_off), short_unitig=dict(off=short), unsorted=dict(arr=unsorted))
    for what, kw in cases.items():
        assert host(**kw) == -1, what
        assert np.all(rec.view(np.uint8) == 0x5A), f"{what}: something ran"
    # the device form: parameters, NULL and overlap only
    d_off, d_pl = to_dev(off, np.int64), to_dev(arr.view(np.uint8).reshape(-1, 32))
    d_rec = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    d_lout, d_org = torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")

    def dev(k=K, nu=nu, n=n, par=good, rec=d_rec.data_ptr(), lout=d_lout.data_ptr(), org=d_org.data_ptr(), no=no, st=st, pl=d_pl.data_ptr()):
        return m.L.kmx_unitig_pair_reduce_dev(m.h, k, d_off.data_ptr(), nu, int(off[-1]), pl, n, C.byref(par) if par is not None else None, rec, lout, org, n, C.byref(no) if no is not None else None,
                                              C.byref(st) if st is not None else None)

    for what, kw in dict(even_k=dict(k=22), many_unitigs=dict(nu=2 ** 31), many_entries=dict(n=2 ** 31), max_row_0=dict(par=PairReduceParams(2, 600, 1, 0, 0)), reserved=dict(par=PairReduceParams(2, 600, 1, 64, 7)),
                         null_params=dict(par=None), null_n_out=dict(no=None), null_stats=dict(st=None), null_rrecs=dict(rec=None), null_plinks=dict(pl=None), overlap=dict(org=d_rec.data_ptr()),
                         in_out_overlap=dict(lout=d_pl.data_ptr())).items():
        assert dev(**kw) == -1, what
        torch.cuda.synchronize()
        assert bool((d_rec == 0x5A).all()), f"{what}: something ran"
    assert dev() == 0
    same(run_dev(m, mu, pl, tol=1), expected(mu, pl, tol=1), "the handle after the refusals")


# ---- the acceptance case, end to end on the device
@pytest.mark.parametrize("seed,holes", X.ISLAND_CASES)
def test_three_islands_come_out_as_one_scaffold(model, seed, holes):
    """reduce on the device, then kmx_unitig_scaffold_dev on the list that stays where the reduce call left it: the genome with
    both holes as N of their true length; on the full list the three unitigs stay apart"""
    import torch
    m = model
    k, strs, pl, genome = X.three_islands(seed, holes)
    buf, off = R.join(strs)
    arr = X.plinks_array(pl)
    d_buf, d_off, d_pl = to_dev(buf), to_dev(off, np.int64), to_dev(arr.view(np.uint8).reshape(-1, 32))
    sp = X.SCAFFOLD_PAR
    _, (ns, nb), _ = m.unitig_scaffold_dev(k, d_buf, d_off, d_pl, len(pl), sp["inner"], sp["min_pairs"], sp["ratio"], sp["min_n"], sp["max_n"])
    assert ns == 3
    (d_rec, d_lout, d_org), n_out, st = m.unitig_pair_reduce_dev(k, d_off, len(buf), d_pl, len(pl), **{f: X.ISLAND_PAR[f] for f in ("inner", "tol", "min_pairs", "max_row")})
    exp = X.flat(X.reduce([len(s) - k + 1 for s in strs], pl, **X.ISLAND_PAR))
    assert n_out == 2 == exp[3] and d_rec.cpu().numpy().reshape(-1).view(X.PAIR_REDUCE_DTYPE).tobytes() == exp[0].tobytes() and st["n_transitive"] == 1
    assert d_lout.cpu().numpy()[:n_out].tobytes() == exp[1].tobytes() and d_org.cpu().numpy()[:n_out].view(np.uint32).tobytes() == exp[2].tobytes()
    out, (ns, nb), sst = m.unitig_scaffold_dev(k, d_buf, d_off, d_lout, n_out, sp["inner"], sp["min_pairs"], sp["ratio"], sp["min_n"], sp["max_n"])
    torch.cuda.synchronize()
    s = out[0].cpu().numpy()[:nb].tobytes().decode()
    n_holes = sum(hi - lo for lo, hi in holes)
    assert (ns, nb) == (1, X.ISLAND_GENOME) and s.count("N") == n_holes and sst["n_chain"] == 2
    assert all(c == g for c, g in zip(s, genome) if c != "N") and all(s[lo:hi] == "N" * (hi - lo) for lo, hi in holes)
    want = S.scaffold(k, strs, None, [tuple(e) for e in exp[1].tolist()], **sp)
    assert want["sstrs"] == [s]
    # the convenience of the Python layer, on host buffers
    got = m.reduced_scaffolds_from_pairs(k, strs, arr, sp["inner"], sp["min_pairs"], sp["ratio"], sp["min_n"], sp["max_n"])
    assert got[0] == [s] and got[7]["n_transitive"] == 1


def test_a_handle_serves_a_larger_then_a_smaller_list():
    m = KModel(1, 1023, NH, NB)
    for n in (513, 31, 257):
        mu, pl = X.line_list(n, 3, 1)
        both(m, mu, pl, f"reuse {n}", tol=1)
    m.set_profile(1)
    mu, pl = X.line_list(513, 3, 1)
    same(run_dev(m, mu, pl, tol=1), expected(mu, pl, tol=1), "under the profile")
    ph = m.unitig_pair_reduce_phases()
    assert set(ph) == {"rows", "sort", "verdicts", "compact"} and all(v > 0 for v in ph.values())
    m.set_profile(0)


# ---- the facade and the driver
def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_pair_reduce.cpp prints the stats, the verdict table and the list that stays for a line list; the driver's
    -u1 -M -W21 -P400 -S2 -L writes pairs.reduced.tsv and scaffolds the three islands into one, leaves three without -L and every
    other output as it is, and runs the fill on the reduced list with -F"""
    import count_reads as CR

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    mu, pl = X.line_list(257, 3, 1)
    res = X.reduce(mu, pl, **dict(X.PAR, tol=1))
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("".join(" ".join(map(str, e)) + "\n" for e in pl))
    exe = build("tests/facade_unitig_pair_reduce.cpp", "facade_unitig_pair_reduce")
    out = subprocess.check_output([exe, str(K), str(X.PAR["min_pairs"]), str(X.PAR["inner"]), "1", str(X.PAR["max_row"]), ",".join(str(m + K - 1) for m in mu), lst], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 3 and blocks[0] == " ".join(str(res["stats"][f]) for f in X.STAT_FIELDS[:9]) + "\n"
    assert blocks[1] == X.reduce_tsv(pl, res) and blocks[2] == "".join(f"{i} {e[0]} {e[1]} {e[2]} {e[3]}\n" for i, e in zip(res["origin"], res["lout"]))
    seed, holes = X.ISLAND_CASES[0]
    k, strs, ipl, genome = X.three_islands(seed, holes)
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in X.island_reads(seed, holes)[1]])
    ires = X.reduce([len(s) - k + 1 for s in strs], ipl, **X.ISLAND_PAR)
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    base = ["-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-S2", f"-k{k}", "-nh3", "-nb2"]
    texts = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix in (".fa", ".tsv", ".gaf", ".gfa", ".agp")}
    work = tmp_path / "plain"
    work.mkdir()
    subprocess.check_call([exe, *base, fa, "db", str(work)], stdout=subprocess.DEVNULL, timeout=120)
    before = texts(work / "db")
    assert "pairs.reduced.tsv" not in before and before["scaffolds.fa"].count(b">") == 3
    for flags in (("-L",), (f"-L{k}",), ("-L0", "-F")):
        work = tmp_path / ("reduced" + "".join(flags))
        work.mkdir()
        log = subprocess.check_output([exe, *base, *flags, fa, "db", str(work)], timeout=120).decode()
        after = texts(work / "db")
        assert after["pairs.reduced.tsv"].decode() == X.reduce_tsv(ipl, ires), flags
        seqs = [s for s in after["scaffolds.fa"].decode().split("\n") if s and s[0] != ">"]
        assert len(seqs) == 1 and len(seqs[0]) == X.ISLAND_GENOME and seqs[0].count("N") == 20, flags
        s = seqs[0] if seqs[0][:50] == genome[:50] else S.oriented(seqs[0], 1)
        assert all(c == g for c, g in zip(s, genome) if c != "N") and all(s[lo:hi] == "N" * (hi - lo) for lo, hi in holes), flags
        changed = ("pairs.reduced.tsv", "scaffolds.fa", "scaffolds.paths.tsv", "scaffolds.agp", "scaffolds.filled.fa", "scaffolds.fill.tsv")
        assert {n: b for n, b in after.items() if n not in changed} == {n: b for n, b in before.items() if n not in changed}, flags
        assert "1 of 3 links skip a unitig (2 kept, 0 complex, 0 below 2 pairs, 0 ignored), 2 links stay" in log and "2 of 2 links joined, 20 N" in log, flags
        assert ("scaffolds.filled.fa" in after) == ("-F" in flags)
    assert subprocess.call([exe, "-g", "-u1", "-M", f"-W{k}", f"-P{P.MAX_DIST}", "-L", f"-k{k}", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2     # -L without -S
    assert subprocess.call([exe, *base, "-Lx", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
