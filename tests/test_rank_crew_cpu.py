"""The crew of host threads behind kmx_build_from_kmc_multi_ex (kmcex_amd/csrc/rank_crew.h: HostBarrier, RankCrew) on the CPU:
tests/rank_crew_driver.cpp includes the header into a plain C++ program, built as it is, with TSan and with ASan + UBSan, and run
as a program.  What is asked of it is the agreement rule: an error noted, or an exception thrown, by one rank in step s is every
rank's answer from the barrier of step s on -- every rank ran the steps up to s, no rank ran a later one, every rank's step()
returned the same at every step -- and the first error, with its message, is what the crew reports after run().  Every run must
exit 0 (no terminate, every thread joined) with nothing on stderr.  No GPU, and nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OOM, INTERNAL = -6, -1                             # the codes the driver gives the crew for bad_alloc / any other exception
RANKS = (1, 2, 3, 8)
S_LONG, S = 200, 40                                # steps of the walk without an error (the barrier is reused 200 times) / of the others
BUILDS = {"plain": (), "tsan": ("-fsanitize=thread", "-g"), "asan_ubsan": ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rank_crew") / ("driver_" + request.param))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", *BUILDS[request.param], os.path.join(ROOT, "tests", "rank_crew_driver.cpp"), "-o", exe])

    def run(cases):
        """[(P, S, kind, r1, r2, s)] -> [(code, message, bodies ended, agreed, first failed step, its return, [(steps run, leading)] per rank)]"""
        p = subprocess.run([exe], input="".join(" ".join(str(x) for x in c) + "\n" for c in cases).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and not p.stderr, (request.param, p.returncode, p.stderr.decode()[-2000:])
        rows = [x.split("\t") for x in p.stdout.decode().splitlines()]
        assert len(rows) == len(cases)
        return [(int(r[0]), r[1], int(r[2]), int(r[3]), int(r[4]), int(r[5]), [tuple(int(v) for v in x.split(":")) for x in r[6:]]) for r in rows]
    return run


def stopped_after(got, P, s, code):
    """every rank ran the steps 0 .. s and nothing later, every step() returned the same: 0 before step s, `code` from it on"""
    _, _, ended, agreed, first, ret, ran = got
    assert ended == P and agreed == 1
    assert (first, ret) == (s, code)
    assert ran == [(s + 1, s + 1)] * P


def test_no_error_every_rank_runs_every_step(driver):
    for P, got in zip(RANKS, driver([(P, S_LONG, "N", 0, 0, 0) for P in RANKS])):
        assert got == (0, "", P, 1, -1, 0, [(S_LONG, S_LONG)] * P), P


def places(P):
    return [(r, s) for r in sorted({0, P - 1}) for s in (0, S // 2, S - 1)]       # the caller's thread and the last spawned one; first, middle and last step


def test_an_error_noted_in_step_s_stops_every_rank_behind_step_s(driver):
    cases = [(P, S, "E", r, 0, s) for P in RANKS for r, s in places(P)]
    for c, got in zip(cases, driver(cases)):
        P, _, _, r, _, s = c
        assert got[:2] == (100 + r, f"rank {r} step {s}"), c                       # (s = S - 1: an error of the last step is still there after run())
        stopped_after(got, P, s, 100 + r)


def test_two_ranks_note_different_errors_in_one_step(driver):
    cases = [(P, S, "D", 0, P - 1, s) for P in RANKS if P > 1 for s in (0, S // 2, S - 1)] + [(8, S, "D", 3, 4, 7)]
    for c, got in zip(cases, driver(cases)):
        P, _, _, r1, r2, s = c
        assert got[0] in (100 + r1, 100 + r2) and got[1] == f"rank {got[0] - 100} step {s}", (c, got)   # exactly one of them, with its own message
        stopped_after(got, P, s, got[0])


@pytest.mark.parametrize("kind,code,message", [("A", OOM, "out of host memory"), ("X", INTERNAL, "internal error: x")])
def test_a_rank_throws_in_step_s(driver, kind, code, message):
    cases = [(P, S, kind, r, 0, s) for P in RANKS for r, s in places(P)]
    for c, got in zip(cases, driver(cases)):
        assert got[:2] == (code, message), c
        stopped_after(got, c[0], c[5], code)
