"""Concurrent kmer_to_occ callers on ONE handle: the reference's own batch query is an OpenMP loop over the scalar
kmer_to_occ(string) on one KModel (kmodel.hpp:90-98), so callers ported from it query one handle from many threads at once.

Python threads drive the library through ctypes, which releases the GIL for the length of every call, so the calls overlap
inside libkmx.so.  Every expected answer comes from the CPU oracle, computed on the main thread before the concurrent part
starts; every thread has a seeded query set of its own (present k-mers from every count quartile, half of them
reverse-complemented, and absent draws), so answers that went to the wrong thread or the wrong slot cannot cancel out.
Answers are compared bit for bit, per thread and per index.  At most 8 caller threads.
"""
import threading

import numpy as np
import pytest

import oracle_lib as O
from common import CASE
from kmcex_amd import KModel, synth

pytestmark = pytest.mark.gpu

CASES = ["tiny_k31", "k55_nh9_nb6"]          # W = 1; W = 2 (the k > 32 canonicalisation quirk)
SUB = 1 << 14                                # kQuerySub of kmx_api.hip: strings per pipeline task


def _built(name):
    _, k, ci, cs, nh, nb, n = CASE[name]
    km, cnt = synth.make_stream(n, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    return k, km, cnt, m, o


def _query_set(km, cnt, k, n, seed):
    """n packed k-mers ([n] or [n, 2]): 3/4 present, drawn evenly from the four count quartiles, half of those
    reverse-complemented; 1/4 drawn at random (absent, as good as certainly); shuffled by the seed"""
    rng = np.random.default_rng(seed)
    W = (k + 31) // 32
    km = km.reshape(-1, W)
    quart = np.array_split(np.argsort(cnt, kind="stable"), 4)
    n_present = 3 * n // 4
    idx = np.concatenate([rng.choice(g, size=n_present // 4 + (j < n_present % 4), replace=True) for j, g in enumerate(quart)])
    q = km[idx].copy()
    h = len(q) // 2
    q[:h] = synth.revcomp(q[:h].reshape(-1), k).reshape(-1, W)
    absent = synth.random_kmers(n - len(q), k, seed_k=0x5EED0000 + 7919 * seed).reshape(-1, W)
    q = np.concatenate([q, absent])[rng.permutation(n)]
    return q.reshape(-1) if W == 1 else q


def _dirty_rows(rows, k, seed):
    """copies of uint8[n, k] rows with 'N', lower case or other bytes in two of every three rows"""
    rng = np.random.default_rng(seed)
    r = rows.copy()
    for i in range(len(r)):
        if i % 3:
            for _ in range(int(rng.integers(1, 4))):
                r[i, int(rng.integers(0, k))] = ord(str(rng.choice(list("NnacgtX-"))))
    return r


def _strs(rows, ln):
    return [bytes(r[:ln]).decode("latin-1") for r in rows]


def _run(fns, timeout=900, barriers=()):
    """every fn on a thread of its own, all released together; -> their results (the first exception is re-raised, after
    breaking `barriers`, the callers' own, so that nobody waits for a thread that has died)"""
    go = threading.Barrier(len(fns))
    out, errs = [None] * len(fns), []

    def body(i, f):
        try:
            go.wait()
            out[i] = f()
        except BaseException as e:  # noqa: BLE001
            errs.append((i, e))
            for b in (go, *barriers):
                b.abort()

    th = [threading.Thread(target=body, args=(i, f), daemon=True) for i, f in enumerate(fns)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "a caller thread did not finish"
    if errs:
        raise errs[0][1]
    return out


def _bad(got, want):
    """None when equal, else (number of differing answers, first differing index)"""
    got = np.asarray(got, dtype=np.int32)
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    d = np.nonzero(got != want)[0]
    return (len(d), int(d[0]))


# ------------------------------------------------------------------------------------------------ 1. scalar storm
@pytest.mark.parametrize("name", CASES)
def test_scalar_storm_on_one_handle(name):
    """8 threads, each calling kmer_to_occ(str) (kmx_query_ascii with n = 1: the reference's OpenMP loop body) over 300
    strings of its own, three times over: every answer is the oracle's for that thread's string."""
    k, km, cnt, m, o = _built(name)
    T, n = 8, 300
    sets = [_strs(synth.to_ascii(_query_set(km, cnt, k, n, seed=100 + t), k), k) for t in range(T)]
    want = [o.query_strings(s) for s in sets]

    def caller(t):
        return [[m.kmer_to_occ(s) for s in sets[t]] for _ in range(3)]

    got = _run([lambda t=t: caller(t) for t in range(T)])
    for t in range(T):
        for r, g in enumerate(got[t]):
            assert _bad(g, want[t]) is None, (t, r, _bad(g, want[t]))


# ------------------------------------------------------------------------------------------------ 2. batches of different sizes
@pytest.mark.parametrize("name", CASES)
def test_batches_of_different_sizes_while_the_feed_grows(name):
    """Small kmer_to_occ_rows batches (2^14 strings) loop on 6 threads while a 7th thread sends two much larger batches.

    The slots of the handle's query feed hold C = min(kQuerySlotBytes / item_bytes, n rounded up to 2^14) items
    (query_pipeline), and ensure_query_feed frees and reallocates all three slots whenever a batch needs a larger C.  The
    small threads' first batches size the feed for 2^14 strings (the big thread waits for them); then
      * the 2^20-string batch needs C = 2^20 > 2^14: the feed GROWS while the small threads keep running through it;
      * the second big batch (2^22 + 12345 strings at W = 1, 2^21 + 12345 at W = 2: more than 32 MB / (8 W) packed
        k-mers) needs C = 2^22 (2^21) and grows the feed again, then spans two chunks that reuse the slots.
    Among the small threads, one sends strings of another length than k (the byte-string pass alone, item_bytes = len)
    and one sends dirty strings ('N', lower case, 'X': the packed pass, then the byte-string pass over the dirty ones).
    """
    k, km, cnt, m, o = _built(name)
    W = (k + 31) // 32
    ln_other = k - 5
    small = []                                 # (rows, ln, separate, expected) per small thread
    for t in range(6):
        rows = synth.to_ascii(_query_set(km, cnt, k, SUB, seed=200 + t), k)
        if t == 4:
            small.append((rows, ln_other, True, o.query_strings(_strs(rows, ln_other))))
        elif t == 5:
            d = _dirty_rows(rows, k, seed=300 + t)
            small.append((d, k, False, o.query_strings(_strs(d, k))))
        else:
            q = synth.from_strings(_strs(rows, k), k)
            small.append((rows, k, t % 2 == 0, o.query_packed(k, q.reshape(-1))))
    big = []
    for j, nb in enumerate([1 << 20, (1 << 22 if W == 1 else 1 << 21) + 12345]):
        pool = _query_set(km, cnt, k, 1 << 16, seed=400 + j).reshape(-1, W)
        q = pool[np.random.default_rng(500 + j).integers(0, len(pool), size=nb)]
        big.append((synth.to_ascii(q.reshape(-1), k), o.query_packed(k, q.reshape(-1))))

    sized = threading.Barrier(len(small) + 1)  # the big thread starts once every small thread has been answered once
    big_done = threading.Event()

    def small_caller(t):
        rows, ln, sep, want = small[t]
        bad, it = [], 0
        while True:
            g = m.kmer_to_occ_rows(rows, ln, sep)
            if _bad(g, want) is not None:
                bad.append((it, _bad(g, want)))
            if it == 0:
                sized.wait()
            it += 1
            if big_done.is_set() and it >= 3:
                return bad, it

    def big_caller():
        sized.wait()
        try:
            return [_bad(m.kmer_to_occ_rows(rows, k, True), want) for rows, want in big]
        finally:
            big_done.set()

    got = _run([lambda t=t: small_caller(t) for t in range(len(small))] + [big_caller], barriers=[sized])
    for t in range(len(small)):
        bad, iters = got[t]
        assert bad == [], (t, iters, bad)
    assert got[-1] == [None, None], got[-1]
    for t in range(len(small)):                 # the grown feed still answers small batches
        rows, ln, sep, want = small[t]
        assert _bad(m.kmer_to_occ_rows(rows, ln, sep), want) is None, t


# ------------------------------------------------------------------------------------------------ 3. the four front doors
def _door_jobs(m, o, k, km, cnt, seed0, doors, n=20000, iters=3):
    """one job per entry of `doors` ("strings", "ascii", "scalar", "packed", "dev") with a query set of its own, and the
    oracle's answers for it; a job returns the list of (iteration, mismatch) it saw"""
    import torch
    jobs = []
    for t, door in enumerate(doors):
        nn = 300 if door == "scalar" else n
        q = _query_set(km, cnt, k, nn, seed=seed0 + t)
        want = o.query_packed(k, q.reshape(-1))

        def job(door=door, q=q, want=want, nn=nn):
            bad = []
            if door == "dev":
                d_q = torch.from_numpy(np.ascontiguousarray(q).reshape(-1).view(np.int64)).to("cuda")
                d_out = torch.empty(nn, dtype=torch.int32, device="cuda")
            else:
                rows = synth.to_ascii(q.reshape(-1), k)
                strs = _strs(rows, k)
            for it in range(iters):
                if door == "strings":
                    g = m.kmer_to_occ_rows(rows, k, True)               # kmx_query_strings
                elif door == "ascii":
                    g = m.kmer_to_occ_rows(rows, k, False)              # kmx_query_ascii, one buffer
                elif door == "scalar":
                    g = [m.kmer_to_occ(s) for s in strs]                 # kmx_query_ascii, n = 1
                elif door == "packed":
                    g = m.kmer_to_occ_packed(q.reshape(-1))              # kmx_query_packed (host buffers)
                else:
                    d_out.fill_(-7)
                    torch.cuda.synchronize()
                    m.kmer_to_occ_dev(d_q.data_ptr(), nn, d_out.data_ptr())   # kmx_query_packed_dev (this thread's device buffers)
                    torch.cuda.synchronize()
                    g = d_out.cpu().numpy()
                if _bad(g, want) is not None:
                    bad.append((it, _bad(g, want)))
            return bad
        jobs.append(job)
    return jobs


@pytest.mark.parametrize("name", CASES)
def test_all_four_front_doors_on_one_handle(name):
    """kmx_query_strings, kmx_query_ascii (a batch, and n = 1), kmx_query_packed and kmx_query_packed_dev, all at once on
    one handle from 8 threads; the device callers use torch buffers of their own, synchronised before the comparison."""
    k, km, cnt, m, o = _built(name)
    doors = ["strings", "strings", "ascii", "scalar", "packed", "packed", "dev", "dev"]
    jobs = _door_jobs(m, o, k, km, cnt, 600, doors)
    got = _run(jobs)
    for t, bad in enumerate(got):
        assert bad == [], (doors[t], t, bad)


# ------------------------------------------------------------------------------------------------ 4. accounting
@pytest.mark.parametrize("name", CASES)
def test_accounting_and_timing_under_concurrent_queries(name):
    """kmx_set_profile(m, 2): packed queries (host and device) from 4 threads at once count exactly what the same queries
    count one after another on a fresh build (query_accounted, query_neighbour_calls: integer counts, order-free).
    kmx_set_profile(m, 1): the same workload times every query kernel exactly once and answers the same."""
    k, km, cnt, m, o = _built(name)
    doors = ["packed", "packed", "dev", "dev"]
    n, iters = 20000, 3
    m.set_profile(2)
    jobs = _door_jobs(m, o, k, km, cnt, 700, doors, n=n, iters=iters)
    got = _run(jobs)
    for t, bad in enumerate(got):
        assert bad == [], (doors[t], t, bad)
    st = m.stats()
    seq = _built(name)[3]                                       # a fresh build: its counters start at zero like m's did
    seq.set_profile(2)
    sjobs = _door_jobs(seq, o, k, km, cnt, 700, doors, n=n, iters=iters)
    for t, job in enumerate(sjobs):
        assert job() == [], (doors[t], t)
    ss = seq.stats()
    assert st.query_accounted == ss.query_accounted == len(doors) * iters * n
    assert st.query_neighbour_calls == ss.query_neighbour_calls
    seq.close()

    m.set_profile(1)
    m.kernel_times(reset=True)
    jobs = _door_jobs(m, o, k, km, cnt, 700, doors, n=n, iters=iters)
    got = _run(jobs)
    for t, bad in enumerate(got):
        assert bad == [], ("profile 1", doors[t], t, bad)
    assert m.kernel_times()["query"]["launches"] == len(doors) * iters
    m.set_profile(0)
    assert m.stats().query_accounted == st.query_accounted      # timing does not account


# ------------------------------------------------------------------------------------------------ 5. two handles
def test_two_handles_on_one_device_queried_at_once():
    """Two models on one device (W = 1 and W = 2), each queried by 4 threads through several front doors at the same
    time: every handle answers with its own oracle's answers (the feeds are per handle)."""
    doors = ["strings", "ascii", "packed", "dev"]
    jobs, names = [], []
    keep = []
    for j, name in enumerate(CASES):
        k, km, cnt, m, o = _built(name)
        keep.append((m, o))
        js = _door_jobs(m, o, k, km, cnt, 800 + 10 * j, doors)
        jobs += js
        names += [(name, d) for d in doors]
    got = _run(jobs)
    for t, bad in enumerate(got):
        assert bad == [], (names[t], bad)
