"""An allocation that fails leaves the handle consistent: the same call on the same handle then succeeds, bit for bit.

KMX_FAIL_ALLOC=n (test hook, read with KMX_TEST_HOOKS=1 at every C entry point) makes the n-th device or pinned allocation
of that call return hipErrorOutOfMemory without calling HIP: nothing is provoked on the device.  Every entry point below is
walked with n = 1, 2, 3, ... until the armed call meets fewer than n allocations and succeeds.  Buffers are kept on the
handle, so every step starts on a handle that has not made that kind of call yet (a new one for the builds, a freshly built
one for the queries and for counting) and destroys it at its end.

"The same call" is the whole kmx_begin / kmx_insert_batch / kmx_finish sequence for the streamed build (a failed insert
leaves a partial build, which only kmx_begin restarts) and a new session on the same handle for counting (a session that
fails ends, include/kmx.h).  Free device memory is not asserted: other work may share the card.  Single-threaded.
"""
import os

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_reads as R
from kmcex_amd import KModel, api, synth
from kmcex_amd.api import KmxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 500                                    # (the host layer has fewer than 150 allocation sites: a stop for a broken countdown)
KMX_E_NODEVICE, KMX_E_NOMEM = -2, -6
CI, CS, NH, NB = 1, 1023, 7, 5                     # one handle shape for every case (the defect-1 case changes k on a handle)
N_DRAWS = {31: 20000, 55: 30000}                   # k-mers drawn per k: both leave a rest table (asserted below)


def walk(monkeypatch, fresh, call, check):
    """n = 1, 2, ...: on fresh() the armed call(m) fails with KMX_E_NOMEM / KMX_E_NODEVICE, the same call on the same handle
    then succeeds and check(m, result) holds; ends at the first n the armed call survives."""
    failed = 0
    for n in range(1, MAX_STEPS + 1):
        m = fresh()
        monkeypatch.setenv("KMX_FAIL_ALLOC", str(n))
        try:
            res = call(m)
            survived = True
        except KmxError as e:
            assert e.code in (KMX_E_NOMEM, KMX_E_NODEVICE), f"step {n}: {e}"
            survived = False
        finally:
            monkeypatch.delenv("KMX_FAIL_ALLOC")
        if not survived:
            failed += 1
            res = call(m)                          # nothing armed: the same call, the same handle
        check(m, res)
        assert m.L.kmx_destroy(m.h) == 0, f"step {n}: kmx_destroy"
        m.h = None
        if survived:
            print(f"{failed} allocations failed in turn, the call survived the countdown at n = {n}")
            assert failed > 0, "no allocation failed: the countdown is not wired in"
            return
    pytest.fail(f"the armed call still fails after {MAX_STEPS} steps")


_cases = {}


def case(k):
    """(k-mers, counts, n_bf, oracle) of the stream at k"""
    if k not in _cases:
        km, cnt = synth.make_stream(N_DRAWS[k], k, CI, CS)
        o = O.OracleModel(CI, CS, NH, NB)
        o.build(k, km, cnt)
        assert o.stats().rest_entries > 0, "an empty rest table: rest_sort would allocate nothing"
        _cases[k] = (km, cnt, [int((cnt == CI).sum())], o)
    return _cases[k]


def same_arrays(m, o):
    for a in range(NB):
        assert np.array_equal(m.download("tag", a), o.array_bytes("tag", a)), f"tag array {a}"
        assert np.array_equal(m.download("value", a), o.array_bytes("value", a)), f"value array {a}"
    assert np.array_equal(m.download("km_back"), o.array_bytes("km_back"))
    assert np.array_equal(m.download("bf", 0), o.array_bytes("bf", 0))
    assert np.array_equal(m.download("bf_back", 0), o.array_bytes("bf_back", 0))
    s, so = m.stats(), o.stats()
    assert (s.attempts, s.successes, s.rest_entries) == (so.attempts, so.successes, so.rest_entries)


def new_handle():
    return KModel(CI, CS, NH, NB)


def streamed(m, k):
    km, cnt, n_bf, _ = case(k)
    m.begin(k, n_bf, len(cnt))
    m.insert_batch(km, cnt)
    m.finish()


@pytest.mark.parametrize("k", [31, 55])
def test_build_host(k, monkeypatch):
    km, cnt, _, o = case(k)
    walk(monkeypatch, new_handle, lambda m: m.build_packed(k, km, cnt), lambda m, _: same_arrays(m, o))


@pytest.mark.parametrize("k", [31, 55])
def test_begin_insert_finish(k, monkeypatch):
    o = case(k)[3]
    walk(monkeypatch, new_handle, lambda m: streamed(m, k), lambda m, _: same_arrays(m, o))


def built(k):
    km, cnt, _, _ = case(k)
    m = new_handle()
    m.build_packed(k, km, cnt)
    return m


@pytest.mark.parametrize("k", [31, 55])
def test_query_strings(k, monkeypatch):
    km, _, _, o = case(k)
    q = np.concatenate([km[::3], synth.random_kmers(2000, k, seed_k=0xABCDEF0123)])
    rows = synth.to_ascii(q, k)
    rows[5::97, k // 2] = ord("N")                 # some strings the packed form cannot express: the byte-string pass runs too
    exp = o.query_strings([r.tobytes().decode() for r in rows])
    walk(monkeypatch, lambda: built(k), lambda m: m.kmer_to_occ_rows(rows, k), lambda m, got: np.testing.assert_array_equal(got, exp))


@pytest.mark.parametrize("k", [31, 55])
def test_query_seqs(k, monkeypatch):
    o = case(k)[3]
    buf, off = R.flatten(R.make_reads(20000, k, n_reads=300, long_read=3000))
    exp = R.oracle_per_base(o, buf, off, k)
    walk(monkeypatch, lambda: built(k), lambda m: m.seq_to_occ_flat(buf, off), lambda m, got: np.testing.assert_array_equal(got, exp))


@pytest.mark.parametrize("k", [31, 55])
def test_counting_session(k, monkeypatch):
    buf, off = R.flatten(R.make_reads(20000, k, n_reads=1500, long_read=3000))
    lkm, lcnt = CR.count(buf, off, k, CI, CS)
    o = O.OracleModel(CI, CS, NH, NB)
    o.build(k, lkm, lcnt)

    def session(m):
        m.count_begin(k)
        m.count_seqs(buf, off)
        return m.count_finish()

    def check(m, n_listed):
        assert n_listed == len(lcnt)
        got_km, got_c = m.count_listing()
        assert np.array_equal(got_km, lkm) and np.array_equal(got_c, lcnt)
        same_arrays(m, o)

    walk(monkeypatch, lambda: built(k), session, check)


def test_build_from_kmc(monkeypatch):
    db = os.path.join(ROOT, "tests", "golden", "tiny", "db")
    k, _, km, cnt = api.kmc_list(db)
    o = O.OracleModel(CI, CS, NH, NB)
    o.build(k, km, cnt)
    walk(monkeypatch, new_handle, lambda m: m.init(db), lambda m, _: same_arrays(m, o))


def test_slots_that_failed_to_grow_are_not_trusted_later(monkeypatch):
    """One handle: a streamed build at k = 31 (one-word slots), the same at k = 55 whose n-th allocation inside
    kmx_insert_batch -- the growth of the pinned and device slots to two words -- fails, then k = 31 again, which must not
    take the recorded capacity of a slot that is gone for a slot."""
    o31 = case(31)[3]
    km55, cnt55, n_bf55, _ = case(55)
    failed = 0
    for n in range(1, MAX_STEPS + 1):
        m = new_handle()
        streamed(m, 31)
        m.begin(55, n_bf55, len(cnt55))
        monkeypatch.setenv("KMX_FAIL_ALLOC", str(n))
        try:
            m.insert_batch(km55, cnt55)
            survived = True
        except KmxError as e:
            assert e.code in (KMX_E_NOMEM, KMX_E_NODEVICE), f"step {n}: {e}"
            survived = False
        finally:
            monkeypatch.delenv("KMX_FAIL_ALLOC")
        streamed(m, 31)
        same_arrays(m, o31)
        assert m.L.kmx_destroy(m.h) == 0, f"step {n}: kmx_destroy"
        m.h = None
        failed += not survived
        if survived:
            break
    else:
        pytest.fail(f"the armed kmx_insert_batch still fails after {MAX_STEPS} steps")
    print(f"{failed} allocations of kmx_insert_batch failed in turn")
    assert failed >= 2, "the slots of a two-word build grow by at least a pinned and a device buffer"
