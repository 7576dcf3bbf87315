"""An allocation that fails inside kmx_build_from_kmc_multi_ex ends the call with an error on every handle's thread, and the same
call on the same handles then builds the reference's files: the walk of tests/test_gpu_alloc_failure.py (read its header) applied
to api.init_multi.

KMX_FAIL_ALLOC=n makes the n-th device or pinned allocation of the call return out-of-memory without calling HIP: nothing is
provoked on the device.  The countdown is one atomic shared by all of the build's host threads, so exactly one allocation fails,
on whichever rank reaches it; what is tested is that every rank then skips the same steps (kmcex_amd/csrc/rank_crew.h) -- the
call RETURNS, with KMX_E_NOMEM or KMX_E_NODEVICE -- and leaves nothing behind that a second build trips over.  n = 1, 2, ... on
fresh handles until the armed call survives.  The parametrisations are the smallest at which each transport runs its rounds; with
KMX_RANGE_CAPX=20000 the RCCL build is void (a region overflows) and is repeated through the inboxes, failures in the repeat included.
Two handles allocate 123 (ring) and 137 (range) times, the void RCCL build and its repeat 95 times: those walks are cut into
ranges of n, a parametrisation each, so that none takes much more than five seconds; no n is left out.
"""
import os

import pytest

from common import CASE, sha_file
from kmcex_amd import KModel, api, kmcdb, synth
from kmcex_amd.api import KmxError

pytestmark = pytest.mark.gpu
MAX_STEPS = 500                                    # (a stop for a broken countdown: a handle's share of a build allocates fewer than 100 times)
KMX_E_NODEVICE, KMX_E_NOMEM = -2, -6
NAME = "tiny_k31"


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    _, k, ci, cs, nh, nb, n = CASE[NAME]
    km, cnt = synth.make_stream(n, k, ci, cs)
    path = str(tmp_path_factory.mktemp("multi_failure") / "db")
    kmcdb.write_kmc1(path, km, cnt, k, ci, cs)
    return path


THIRDS, HALVES, WHOLE = [(1, 50), (51, 100), (101, MAX_STEPS)], [(1, 50), (51, MAX_STEPS)], [(1, MAX_STEPS)]       # n from .. to, both included
WALKS = [("ring", 2, None, THIRDS), ("range", 2, None, THIRDS), ("range", 1, None, WHOLE), ("range-rccl", 1, None, WHOLE), ("range-rccl", 1, "20000", HALVES)]


@pytest.mark.parametrize("partition,handles,capx,n_from,n_to", [(p, h, c, lo, hi) for p, h, c, parts in WALKS for lo, hi in parts])
def test_an_allocation_fails_in_a_build_by_several_handles(partition, handles, capx, n_from, n_to, db, golden, tmp_path, monkeypatch, capfd):
    _, k, ci, cs, nh, nb, n = CASE[NAME]
    g = golden["cases"][NAME]
    want = (g["stats"]["attempts"], g["stats"]["successes"], g["stats"]["rest_entries"])
    out = str(tmp_path / "m")
    os.makedirs(out)
    if capx:
        monkeypatch.setenv("KMX_RANGE_CAPX", capx)
        monkeypatch.setenv("KMX_INIT_TRACE", "1")                  # (the library says on stderr when it repeats a void build)
    failed = 0
    for step in range(n_from, n_to + 1):
        ms = [KModel(ci, cs, nh, nb) for _ in range(handles)]
        monkeypatch.setenv("KMX_FAIL_ALLOC", str(step))
        try:
            api.init_multi(ms, db, partition)
            survived = True
        except KmxError as e:
            assert e.code in (KMX_E_NOMEM, KMX_E_NODEVICE), f"step {step}: {e}"
            survived = False
        finally:
            monkeypatch.delenv("KMX_FAIL_ALLOC")
        if not survived:
            failed += 1
            capfd.readouterr()
            api.init_multi(ms, db, partition)                     # nothing armed: the same call, the same handles
            if capx:
                assert "overflowed" in capfd.readouterr().err, "the regions did not overflow: this case does not reach the repeat"
        for j, m in enumerate(ms):
            m.save(out)
            for f in ("header", "km.bin", "rest.bin"):
                assert sha_file(os.path.join(out, f)) == g["sha256"][f], (step, j, f)
            st = m.stats()
            assert (st.attempts, st.successes, st.rest_entries) == want, (step, j)
            m.close()
        if survived:
            print(f"{partition}, {handles} handles, capx {capx}: {failed} allocations failed in turn, the call survived the countdown at n = {step}")
            assert failed > 0 or n_from > 1, "no allocation failed: the countdown is not wired in"      # (n_from > 1: every n below it failed, or the walk ended, in the ranges before)
            return
    assert n_to < MAX_STEPS, f"the armed call still fails after {MAX_STEPS} steps"
