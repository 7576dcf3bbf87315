"""The argument checks the graph calls share (kmcex_amd/csrc/graph_checks.h: check_link_csr, check_unitig_lengths, check_spans)
on the CPU: tests/graph_checks_driver.cpp includes the header into a plain C++ program, built once as it is and once with
ASan + UBSan, and answers one return code per case.  The hand-made cases are the smallest at which a check can go wrong (0 to 3
unitigs) with their codes written out; then every small valid CSR the restatements' case generators make passes the strict check,
and fails it with any single edge taken out whose mirror stays.  No GPU, and nothing is loaded into Python."""
import functools
import os
import subprocess

import pytest

import unitig_contigs_ref as G
import unitig_resolve_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG = 0, -1
BUILDS = {"plain": (), "sanitized": ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("graph_checks") / ("driver_" + request.param))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", *BUILDS[request.param], os.path.join(ROOT, "tests", "graph_checks_driver.cpp"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="".join(x + "\n" for x in lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0 and not p.stderr, (request.param, p.returncode, p.stderr.decode()[-2000:])
        got = [int(x) for x in p.stdout.split()]
        assert len(got) == len(lines)
        return got
    return run


def arr(v):
    return " ".join(str(x) for x in [len(v), *v])


def csr(strict, n_u, n_links, offs, links):
    return f"C {int(strict)} {n_u} {n_links} {arr(offs)} {arr(links)}"


def of_rows(strict, rows):
    offs = G.offsets_of(rows)
    return csr(strict, len(rows) // 2, offs[-1], offs, [b for row in rows for b in row])


# (unitigs, n_links, link_offsets, links) -> (the code with strict, the code without)
FOUR = (3, 8, [0, 4, 4, 5, 6, 7, 8], [2, 3, 4, 5, 1, 1, 1, 1])            # 0 -> 2, 3, 4, 5 and the four mirrors into 1
FIVE = (3, 9, [0, 5, 5, 6, 7, 8, 9], [2, 3, 4, 5, 1, 1, 1, 1, 1])         # ... and the hairpin 0 -> 1, which is its own mirror
CSR_CASES = {
    "empty graph": ((0, 0, [0], []), (OK, OK)),
    "empty graph, one link": ((0, 1, [0], [0]), (ARG, ARG)),
    "first offset 1": ((1, 1, [1, 1, 1], [1]), (ARG, ARG)),
    "offsets decrease": ((1, 0, [0, 1, 0], [1]), (ARG, ARG)),
    "last offset one short": ((1, 2, [0, 1, 1], [1, 1]), (ARG, ARG)),
    "last offset one over": ((1, 2, [0, 1, 3], [1, 1]), (ARG, ARG)),
    "row of 4": (FOUR, (OK, OK)),
    "row of 5": (FIVE, (ARG, OK)),
    "hairpin a -> a ^ 1, the target 2 U - 1": ((1, 1, [0, 1, 1], [1]), (OK, OK)),
    "target 2 U": ((1, 1, [0, 1, 1], [2]), (ARG, ARG)),
    "target 0xFFFFFFFF": ((1, 1, [0, 1, 1], [0xFFFFFFFF]), (ARG, ARG)),
    "self-loop with its mirror": ((1, 2, [0, 1, 2], [0, 1]), (OK, OK)),
    "self-loop without its mirror": ((1, 1, [0, 1, 1], [0]), (ARG, OK)),
    "one edge and its mirror": ((2, 2, [0, 1, 1, 1, 2], [2, 1]), (OK, OK)),
    "one edge, its mirror removed": ((2, 1, [0, 1, 1, 1, 1], [2]), (ARG, OK)),
    "one edge, the mirror's target wrong": ((2, 2, [0, 1, 1, 1, 2], [2, 0]), (ARG, OK)),
    "null link_offsets": ((0, 0, [], []), (ARG, ARG)),
}
# (unitigs, k, uoffsets) -> the code
LENGTH_CASES = {
    "k - 1 bytes": ((1, 5, [0, 4]), ARG), "k bytes": ((1, 5, [0, 5]), OK), "no unitig": ((0, 5, [0]), OK), "the last of three has k - 1": ((3, 7, [0, 7, 15, 21]), ARG),
    "three of k and more": ((3, 7, [0, 7, 15, 22]), OK), "k = 63, 62 bytes": ((1, 63, [0, 62]), ARG),
}
# [(address, bytes, is an output)] -> the code
SPAN_CASES = {
    "two outputs share one byte": ([(1000, 10, 1), (1009, 10, 1)], ARG), "two outputs touch": ([(1000, 10, 1), (1010, 10, 1)], OK), "an output is an input": ([(1000, 10, 0), (1000, 10, 1)], ARG),
    "an output inside an input": ([(1000, 10, 0), (4000, 8, 0), (1004, 1, 1)], ARG), "null with 0 bytes": ([(0, 0, 1), (1000, 10, 0)], OK), "null with 1 byte": ([(1000, 10, 0), (0, 1, 0)], ARG),
    "two inputs overlap": ([(1000, 10, 0), (1005, 10, 0)], OK), "an empty output inside an input": ([(1000, 10, 0), (1004, 0, 1)], OK), "no buffer": ([], OK),
}


def test_hand_made_cases(driver):
    lines, want, names = [], [], []
    for name, (c, codes) in CSR_CASES.items():
        for strict, code in zip((True, False), codes):
            lines.append(csr(strict, *c))
            want.append(code)
            names.append((name, strict))
    for name, ((n_u, k, offs), code) in LENGTH_CASES.items():
        lines.append(f"L {n_u} {k} {arr(offs)}")
        want.append(code)
        names.append(name)
    for name, (spans, code) in SPAN_CASES.items():
        lines.append(f"S {len(spans)} " + " ".join(f"{p} {n} {o}" for p, n, o in spans))
        want.append(code)
        names.append(name)
    got = driver(lines)
    assert [(n, g) for n, g in zip(names, got)] == [(n, w) for n, w in zip(names, want)]


@functools.lru_cache(maxsize=None)
def generated_rows():
    """name -> rows of every case of the two restatement modules with at most 130 unitigs"""
    out = {}
    for name in G.LISTED_CASES:
        if name not in ("k21_noisy", "k5_complete"):                       # 777 and 512 unitigs
            out[name] = G.listed_case(name)[7]
    for n in (x for x in G.CUT_N if x <= 17):
        for k in G.CUT_K:
            for ring in (False, True):
                out[f"cut {n} {k} {ring}"] = G.cut_case(n, k, ring)[2]
    for name in X.PLANTED:
        out["planted " + name] = X.planted_case(name)[7]
    out["geometry"] = X.geometry_case(21, 0)[2]
    for n in (1, 2, 3, 10):
        out[f"ladder {n}"] = X.ladder_case(n, 5, seed=n)[2]
    assert all(len(rows) <= 260 for rows in out.values())
    return out


def test_generated_graphs_pass_and_miss_every_single_mirror(driver):
    lines, want, names = [], [], []
    for name, rows in generated_rows().items():
        assert all(len(set(row)) == len(row) <= 4 for row in rows), name         # no edge twice: a removed one is then missed
        lines.append(of_rows(True, rows))
        want.append(OK)
        names.append(name)
        for a, row in enumerate(rows):
            for j, b in enumerate(row):
                cut = [list(r) for r in rows]
                del cut[a][j]
                for strict in (True, False):
                    lines.append(of_rows(strict, cut))
                    want.append(ARG if strict and b != a ^ 1 else OK)            # (a hairpin a -> a ^ 1 is its own mirror: nothing is left behind)
                    names.append((name, a, b, strict))
    got = driver(lines)
    assert len(lines) > 2000 and want.count(ARG) > 1000
    wrong = [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not wrong, wrong[:10]
