"""The twelve unitig entry points (kmx_[count_]unitigs[_dev], kmx_[count_]unitig_graph[_dev], kmx_[count_]unitig_graph_clean[_dev])
on the MI355X as one family: the four routes of a tier (the caller's listing or the counted session's, host or device buffers)
return the same bytes; the tiers agree with each other and with the plain-Python restatements; one table of faults runs through
all twelve raw C calls on canary-filled buffers (the code, the counters, every canary); the phase figures say which tier ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import unitig_clean_ref as CL
import unitig_links_ref as UL
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import CleanParams, CleanStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
TIERS = ("unitigs", "unitig_graph", "unitig_graph_clean")
ROUTES = ("host", "dev", "count", "count_dev")
SESSION_K, SESSION_THR = 21, 1                                 # the reads at thr = 1: 2001 unitigs, and 1380 with 3772 links after three rounds
STAT_CANARY = 0x5A5A5A5A5A5A5A5A


def restated(km_s, cnt, k, thr):
    """the three tiers of the restatement for a listing of k-mer strings -> {tier: [bytes per array] (+ [stats])}"""
    strs, recs = U.unitigs(km_s, cnt, k, thr)
    off, lk = UL.flat_links(UL.links(km_s, cnt, k, thr, strs))
    res = CL.clean(km_s, cnt, k, thr)
    plain = [a.tobytes() for a in U.flat(strs, recs)]
    return {"unitigs": plain, "unitig_graph": plain + [off.tobytes(), lk.tobytes()], "unitig_graph_clean": [a.tobytes() for a in CL.flat(res)] + [res["stats"]]}


@functools.lru_cache(maxsize=None)
def caller_case(name):
    """(k, thr, packed k-mers, counts, restated) of a listing the caller brings: a crafted shape with a branch and a tip to clip
    at one-word k, a cycle at two-word k"""
    if name == "y_short_branch_goes":
        k, thr, km_s, cnt = CL.clean_case(name)[:4]
    else:
        k, thr, km_s, cnt = U.case(name)[:4]
    return k, thr, U.pack(km_s, k), np.asarray(cnt, dtype=np.uint32), restated(km_s, cnt, k, thr)


@functools.lru_cache(maxsize=None)
def session_ref():
    reads = U.CASES["reads_thr1"]()[2]
    km_s, cnt = U.listing_of(U.count_kmers(reads, SESSION_K))
    return reads, restated(km_s, cnt, SESSION_K, SESSION_THR)


@pytest.fixture(scope="module")
def session():
    """a handle whose counted session holds the reads' listing -> (handle, packed k-mers, counts)"""
    m = KModel(1, 1023, NH, NB)
    m.count_begin(SESSION_K)
    m.count_seqs(session_ref()[0])
    m.count_finish()
    km, cnt = m.count_listing()
    return m, km, cnt


def to_dev(km, cnt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(km).view(np.int64).reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(cnt).view(np.int32)).cuda()


def flat(got):
    """a result of the Python layer, NumPy or torch -> [bytes per array] (+ [stats])"""
    return [a if isinstance(a, dict) else np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes() for a in got]


def run(m, tier, route, km, cnt, k, thr):
    if route == "host":
        return flat(getattr(m, tier)(km, cnt, k, thr))
    if route == "dev":
        return flat(getattr(m, tier + "_dev")(*to_dev(km, cnt), k, thr))
    return flat(getattr(m, "count_" + tier + ("_dev" if route == "count_dev" else ""))(thr))


def tiers_agree(m, out, km, cnt, k, thr):
    """out: {tier: flat result}.  The strings-only tier is the head of the graph tier; the cleaned graph is the graph of the
    listing without the removed entries (whose first_node then counts the entries that are left: mapped back here)"""
    assert out["unitigs"] == out["unitig_graph"][:3]
    keep = np.frombuffer(out["unitig_graph_clean"][5], dtype=np.uint8) == 0
    assert len(keep) == len(cnt)
    buf, off, rec, loff, lk = m.unitig_graph(km[keep], cnt[keep], k, thr)
    rec = rec.copy()
    rec["first_node"] = np.flatnonzero(keep)[rec["first_node"].astype(np.int64)]
    assert flat((buf, off, rec, loff, lk)) == out["unitig_graph_clean"][:5]


def test_routes_and_tiers_agree_on_the_counted_listing(session):
    """each tier: the session's two routes and the caller's two on count_listing() give the same bytes, those of the restatement"""
    m, km, cnt = session
    want = session_ref()[1]
    out = {}
    for tier in TIERS:
        got = {route: run(m, tier, route, km, cnt, SESSION_K, SESSION_THR) for route in ROUTES}
        for route in ROUTES:
            assert got[route] == got["host"], f"{tier}: route {route} differs from the host route"
        assert got["host"] == want[tier], f"{tier} is not the restatement's"
        out[tier] = got["host"]
    assert len(out["unitig_graph_clean"][4]) > 0 and out["unitig_graph_clean"][6]["rounds_run"] == 3
    tiers_agree(m, out, km, cnt, SESSION_K, SESSION_THR)


@pytest.mark.parametrize("name", ["y_short_branch_goes", "k33_cycle400"])
def test_routes_and_tiers_agree_on_a_callers_listing(name):
    """one word per k-mer and two (the upload's size depends on it): host and device route, every tier, against the restatement"""
    k, thr, km, cnt, want = caller_case(name)
    assert (k > 32) == (name == "k33_cycle400") and km.size == len(cnt) * ((k + 31) // 32)
    m = KModel(1, 1023, NH, NB)
    out = {}
    for tier in TIERS:
        out[tier] = run(m, tier, "host", km, cnt, k, thr)
        assert run(m, tier, "dev", km, cnt, k, thr) == out[tier], f"{tier}: the device route differs from the host route"
        assert out[tier] == want[tier], f"{tier} is not the restatement's"
    if name == "y_short_branch_goes":
        assert out["unitig_graph_clean"][6]["n_tips"] == 1 and len(out["unitig_graph"][4]) > 0
    tiers_agree(m, out, km, cnt, k, thr)


# ---- the raw C calls
def c_name(tier, route):
    return "kmx_" + ("count_" if route.startswith("count") else "") + TIERS[tier] + ("_dev" if route.endswith("dev") else "")


CANARIES = {"seq": (np.uint8, 0xA5), "offs": (np.uint64, 0xA6A6A6A6A6A6A6A6), "rec": (np.uint8, 0xA5), "loffs": (np.uint64, 0xA7A7A7A7A7A7A7A7),
            "links": (np.uint32, 0xA8A8A8A8), "removed": (np.uint8, 0x5A)}


def raw(m, tier, route, k, km, cnt, thr, caps, h="own", null_counter=False, null_listing=False, no_offs=False, no_links=False, ops=7):
    """one raw call of entry point (tier, route) on buffers longer than the capacities it is told, every byte a canary; the
    counters start at 7, the stats as canaries -> (rc, counters, stats, {name: the buffer after the call})"""
    import torch
    dev, counted = route.endswith("dev"), route.startswith("count")
    n = len(cnt)
    seq_cap, rec_cap, link_cap = caps
    sizes = {"seq": seq_cap + 64, "offs": rec_cap + 1 + 8, "rec": (rec_cap + 2) * 40, "loffs": 2 * rec_cap + 1 + 8, "links": link_cap + 16, "removed": n + 16}
    host = {name: np.full(sizes[name], CANARIES[name][1], dtype=CANARIES[name][0]) for name in sizes}
    bufs = {name: torch.from_numpy(a.view(np.uint8)).cuda() for name, a in host.items()} if dev else host
    listing = to_dev(km, cnt) if dev else (km, cnt)

    def ptr(a):
        return a.data_ptr() if dev else a.ctypes.data

    ctr = [C.c_uint64(7) for _ in range(3 if tier else 2)]
    st = CleanStats(*[STAT_CANARY] * 8)
    P = CleanParams(ops, 2 * k, 2 * k, 16)
    args = [m.h if h == "own" else h]
    if not counted:
        args += [k, None if null_listing else ptr(listing[0]), ptr(listing[1]), n]
    args += [thr]
    if tier == 2:
        args += [C.addressof(P)]
    args += [ptr(bufs["seq"]), seq_cap, None if no_offs else ptr(bufs["offs"]), ptr(bufs["rec"]), rec_cap]
    if tier:
        args += [ptr(bufs["loffs"]), None if no_links else ptr(bufs["links"]), link_cap]
    args += [C.byref(c) for c in ctr[:-1]] + [None if null_counter else C.byref(ctr[-1])]
    if tier == 2:
        args += [ptr(bufs["removed"]), C.addressof(st)]
    rc = getattr(m.L, c_name(tier, route))(*args)
    if dev:
        torch.cuda.synchronize()
    after = {name: bufs[name].cpu().numpy().view(host[name].dtype) if dev else host[name] for name in host}
    return rc, tuple(c.value for c in ctr), {f: int(getattr(st, f)) for f, _ in CleanStats._fields_}, after


def untouched(after, names=tuple(CANARIES)):
    return all(np.all(after[name] == CANARIES[name][1]) for name in names)


@pytest.fixture(scope="module")
def other_handles():
    """a handle without a listing, and one whose session was counted at an even k"""
    bare, even = KModel(1, 1023, NH, NB), KModel(1, 1023, NH, NB)
    even.count_begin(20)
    even.count_seqs(session_ref()[0][:20])
    even.count_finish()
    return bare, even


# (fault, the arguments of raw() it changes, the code, the counters afterwards: "kept" = the 7s they held, "zero", "needs");
# the capacities one short follow in the test, which knows the needs
FAULTS = [
    ("null model", {"h": None}, -1, "kept"),
    ("a null counter", {"null_counter": True}, -1, "kept"),
    ("no listing", {}, -4, "kept"),                              # the count routes, on a handle that has none
    ("even k", {}, -1, "zero"),                                  # k = 20: in the arguments, or the session's
    ("n > 0 with a null listing", {"null_listing": True}, -1, "zero"),
    ("seq_out without offsets_out", {"no_offs": True}, -1, "zero"),
    ("seq_out without links", {"no_links": True}, -1, "zero"),
    ("ops = 0", {"ops": 0}, -1, "zero"),
    ("thr = 0", {}, -1, "zero"),
]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tier", [0, 1, 2])
def test_refusal_matrix(tier, route, session, other_handles):
    """every fault of the table that applies to the entry point: the code, the counters, the stats, and every canary; then each
    capacity one short: KMX_E_RANGE, the counters are the needs, nothing is written (the cleaning tier's stats and removed are
    complete); then the same handle gives the right answer into exact room, the canaries behind it intact.  The counted
    session's host routes zero the counters before they refuse a null buffer, as the other nine do."""
    m, km, cnt = session
    bare, even = other_handles
    counted = route.startswith("count")
    k, thr, n = SESSION_K, SESSION_THR, len(cnt)
    want = session_ref()[1][TIERS[tier]]
    nb, nu, nl = len(want[0]), len(want[1]) // 8 - 1, (len(want[4]) // 4 if tier else 0)
    needs = (nu, nb, nl) if tier else (nu, nb)
    assert nu > 1 and nb > 1 and (nl > 1 or not tier)
    roomy = (nb + 100, nu + 10, nl + 10)
    for fault, change, code, counters in FAULTS:
        if (fault == "no listing" and not counted) or (fault == "n > 0 with a null listing" and counted) or (fault == "seq_out without links" and tier == 0) or \
           (fault in ("ops = 0", "thr = 0") and tier != 2):
            continue
        handle = bare if fault == "no listing" else even if fault == "even k" and counted else m
        rc, ctr, st, after = raw(handle, tier, route, 20 if fault == "even k" else k, km, cnt, 0 if fault == "thr = 0" else thr, roomy, **change)
        assert rc == code, (fault, rc)
        written = ctr[:-1] if fault == "a null counter" else ctr
        assert written == (7,) * len(written) if counters == "kept" else written == (0,) * len(written), (fault, ctr)
        assert untouched(after), f"{fault}: a buffer was written"
        assert set(st.values()) == ({STAT_CANARY} if counters == "kept" or tier != 2 else {0}), (fault, st)
    for short in range(3 if tier else 2):
        caps = [nb, nu, nl]
        caps[short] -= 1
        rc, ctr, st, after = raw(m, tier, route, k, km, cnt, thr, tuple(caps))
        assert (rc, ctr) == (-5, needs), (short, rc, ctr)
        assert untouched(after, ("seq", "offs", "rec", "loffs", "links")), f"capacity {short} one short: a buffer was written"
        if tier == 2:
            assert st == want[6] and after["removed"][:n].tobytes() == want[5] and np.all(after["removed"][n:] == 0x5A), short
        else:
            assert untouched(after, ("removed",))
    rc, ctr, st, after = raw(m, tier, route, k, km, cnt, thr, (nb, nu, nl))
    assert (rc, ctr) == (0, needs)
    got = [after["seq"][:nb], after["offs"][:nu + 1], after["rec"][:nu * 40]] + ([after["loffs"][:2 * nu + 1], after["links"][:nl]] if tier else [])
    assert [a.tobytes() for a in got] == want[:len(got)], "after the refusals the answer differs"
    assert untouched({"seq": after["seq"][nb:], "offs": after["offs"][nu + 1:], "rec": after["rec"][nu * 40:]}, ("seq", "offs", "rec"))
    if tier:
        assert untouched({"loffs": after["loffs"][2 * nu + 1:], "links": after["links"][nl:]}, ("loffs", "links"))
    else:
        assert untouched(after, ("loffs", "links"))
    if tier == 2:
        assert st == want[6] and after["removed"][:n].tobytes() == want[5] and np.all(after["removed"][n:] == 0x5A)


def test_phases_say_which_tier_ran():
    """under set_profile(1): no time on the links between unitigs after a strings-only call, some after a graph call; a
    cleaning call's doubling rounds are summed over its rounds, so they are at least those of one graph call"""
    k, thr, km, cnt, _ = caller_case("y_short_branch_goes")
    m = KModel(1, 1023, NH, NB)
    m.set_profile(1)
    m.unitigs(km, cnt, k, thr)
    assert m.unitig_graph_phases()["unitig_links"] == 0 and m.unitigs_phases()["rounds"] >= 1
    m.unitig_graph(km, cnt, k, thr)
    graph = m.unitig_graph_phases()
    assert graph["unitig_links"] > 0
    m.unitig_graph_clean(km, cnt, k, thr)
    assert m.unitig_clean_phases()["rounds"] >= graph["rounds"]
    m.set_profile(0)
