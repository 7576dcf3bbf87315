"""The cases of tests/test_gpu_unitig_scale.py pinned on the CPU by facts that do not come from the restatements' own logic: a chain
case without forks is one contig whose string is the sequence it was cut from (cut_expected's closed form); with forks the counts
follow from n and m by arithmetic (unitig_contigs_ref.fork_counts); the verdicts of a gadget case are the planned ones; a ladder
resolves every centre; and the dense cases do hold the unitig starts per 4096-byte tile of the flat input that they are there for.

The sizes the GPU tests use and what one restatement call takes on the CPU (one core, seconds; generator / restatement):
    chain_case   n = 20000   k = 5   lens (5,)              0.1 / 0.4      820 starts per tile
    chain_case   n = 131072  k = 5   lens (5, 6)            0.7 / 1.8      (65536 and 65537: about half)
    chain_case   n = 65537   k = 21  lens (21, 22, 40)      0.3 / 1.0      (CPU only: the issue's third line)
    chain_case   n = 4020    k = 5   200 fives, one 9000    0.1 / 0.1      201 starts in a tile at the most
    chain_case   n = 6006    k = 5   1000 fives, one 9000   0.1 / 0.1      tiles of 820 starts beside tiles inside a long piece
    chain_case   n = 60000   k = 21  lens (21, 22, 40), fork_every 7      0.3 / 1.1      17143 contigs (ring: 17142)
    gadget_case  576 gadgets  k = 5   lens (5, 6, 13, 4100)        0.3 / 0.02     4032 unitigs, 0.6 MB, 5 tiles of 500 starts or more
    gadget_case  960 gadgets  k = 21  lens (21, 22, 4095, 4097)    0.9 / 0.03     6720 unitigs, 2.1 MB, 768 resolved, 1536 copies added
    ladder_case  n = 3000     k = 5 and 31                         0.3 / 0.2      9002 unitigs, 13 tiles of about 710 starts at k = 5
The resolve restatement was not measured at larger sizes; rings of the chain cases take what lines take."""
import pytest

import unitig_contigs_ref as G
import unitig_resolve_ref as X

MIXED = (5,) * 200 + (9000,)                                   # long pieces, forward and reverse, beside runs of 200 starts
MIXED_FULL = (5,) * 1000 + (9000,)                             # the same with runs that fill a whole tile: 820 starts, then a long piece
DENSE_CHAINS = ((20000, (5,)), (20000, (5, 6)), (20000, (5, 5, 5, 9)), (4020, MIXED), (6006, MIXED_FULL))
DEEP_N = (65536, 65537, 131072)
FORKED = (60000, 21, (21, 22, 40), 7)
GADGETS = {5: (576, (5, 6, 13, 4100)), 21: (960, (21, 22, 4095, 4097))}
SPOIL_EVERY = 5
LADDER_N = 3000
ONE_CONTIG = [(n, 5, lens) for n, lens in DENSE_CHAINS] + [(n, 5, (5, 6)) for n in DEEP_N] + [(65537, 21, (21, 22, 40))]


@pytest.mark.parametrize("ring", (False, True), ids=("line", "ring"))
@pytest.mark.parametrize("n,k,lens", ONE_CONTIG, ids=lambda v: str(v) if isinstance(v, int) else f"lens{len(v)}")
def test_a_chain_without_forks_is_one_contig(n, k, lens, ring):
    kk, strs, rows, hits, text = G.chain_case(n, k, lens, ring)
    res = G.want_chain(n, k, lens, ring)
    assert len(strs) == n and [len(s) for s in strs[:2 * len(lens)]] == [lens[u % len(lens)] for u in range(min(n, 2 * len(lens)))]
    assert len(res["cstrs"]) == 1 and res["cstrs"][0] == G.chain_expected(n, k, lens, ring)
    assert res["crecs"][0]["circular"] == int(ring) and res["crecs"][0]["n_steps"] == n and res["stats"]["n_contigs"] == 1
    assert len(text) == sum(len(s) - k + 1 for s in strs) + k - 1
    if not ring:
        assert res["cstrs"][0] == text
    assert 0 < sum(o & 1 for o in res["steps"]) < n, "forward and reverse steps"


@pytest.mark.parametrize("ring", (False, True), ids=("line", "ring"))
@pytest.mark.parametrize("n,k,lens,m", [FORKED, (15, 5, (5, 6), 7), (14, 5, (5,), 7), (16, 21, (21,), 2), (9, 5, (7,), 3)], ids=lambda v: str(v) if isinstance(v, int) else f"lens{len(v)}")
def test_forks_cut_the_chain_where_arithmetic_says(n, k, lens, m, ring):
    """fork_counts states the formula: F = (n - 1) // m forks on a line, n // m on a ring; 2 F + 1 (ring: 2 F) contigs; every piece of
    the chain holds several unitigs but, on a line, a last piece of n - F m = 1; 4 F edges of the contig graph"""
    kk, strs, rows, hits, text = G.chain_case(n, k, lens, ring, m)
    res = G.want_chain(n, k, lens, ring, m)
    f = n // m if ring else (n - 1) // m
    assert len(strs) == n + f and all(len(s) == k for s in strs[n:])
    assert (res["stats"]["n_contigs"], res["stats"]["n_multi"], sum(map(len, res["crows"]))) == G.fork_counts(n, m, ring)
    assert res["stats"]["n_circular"] == 0 and res["stats"]["n_kept"] == res["stats"]["n_links"] == 2 * (n if ring else n - 1) + 2 * f
    if n < 100:
        G.check(k, strs, None, rows, res, node_graph=False)


@pytest.mark.parametrize("n,lens", DENSE_CHAINS, ids=lambda v: str(v) if isinstance(v, int) else f"lens{len(v)}")
def test_dense_chains_fill_a_tile_with_starts(n, lens):
    """asserted on the input: a 4096-byte window of useq with at least 800 unitig starts, none with more than 1024"""
    for ring in (False, True):
        per_tile = [a for a, _ in X.tile_starts(G.chain_case(n, 5, lens, ring)[1])]
        assert max(per_tile) <= 1024
        if lens == (5,):
            assert min(per_tile[:-1]) >= 819 and len(per_tile) >= 20
        elif lens == MIXED:
            assert max(per_tile) >= 200 and min(per_tile) <= 1 and len(per_tile) >= 40      # a tile inside a piece of 9000 bytes
        elif lens == MIXED_FULL:
            assert max(per_tile) >= 800 and min(per_tile) <= 1 and 0 < sum(a >= 800 for a in per_tile) < len(per_tile) // 4
        else:
            assert min(per_tile[:-1]) >= 4096 // max(lens) and len(per_tile) >= 20
    assert max(a for a, _ in X.tile_starts(G.chain_case(20000, 5, (5,), False)[1])) >= 800


@pytest.mark.parametrize("k", sorted(GADGETS))
def test_gadget_verdicts_are_the_planned_ones(k):
    n_gadgets, lens = GADGETS[k]
    kk, strs, rows, t = X.gadget_case(n_gadgets, k, lens, SPOIL_EVERY)
    plan = X.gadget_plan(n_gadgets, SPOIL_EVERY)
    res = X.resolve(k, strs, None, rows, None, t, *X.GADGET_PIN)
    st = res["stats"]
    good = [(p, number) for p, number, spoiled in plan if spoiled is None]
    assert st["n_candidates"] == n_gadgets and st["n_resolved"] == len(good) == n_gadgets - n_gadgets // SPOIL_EVERY
    for kind in ("ambiguous", "crossed", "unsupported"):
        assert st["n_" + kind] == sum(spoiled == kind for _, _, spoiled in plan) >= n_gadgets // SPOIL_EVERY // 3
    assert st["n_copies_added"] == sum(p - 1 for p, _ in good)
    assert len(set(good)) == 2 + 6 + 24
    seen = {(n, tuple(X.verdict(rows, u, t, *X.GADGET_PIN)[1])) for u, (first, n) in enumerate(res["rplace"]) if n > 1}
    assert len(seen) == 2 + 6 + 24, "every permutation of 2, 3 and 4 ways, as stored"
    X.check_resolved(k, strs, rows, res)
    assert sum(len(s) >= 4095 for s in strs) == n_gadgets // 2 if k == 21 else sum(len(s) == 4100 for s in strs) == n_gadgets // 4
    for pair in X.PARAMS:                                      # what the spoiled ones become at the pairs every case runs at
        other = X.resolve(k, strs, None, rows, None, t, *pair)["stats"]
        assert other["n_candidates"] == n_gadgets and len(good) <= other["n_resolved"] < n_gadgets and other["n_ambiguous"] > 0
    assert X.resolve(k, strs, None, rows, None, t, 2, 0)["stats"]["n_crossed"] > 0 and X.resolve(k, strs, None, rows, None, t, 2, 1)["stats"]["n_unsupported"] > 0


def test_the_dense_gadget_case_mixes_resolved_and_unresolved_starts_in_a_tile():
    """asserted on the input: a 4096-byte window with at least 500 starts of which at least 100 belong to resolved unitigs, at least
    three windows of 500 starts, none above 1024; copy counts 2, 3 and 4 side by side"""
    n_gadgets, lens = GADGETS[5]
    k, strs, rows, t = X.gadget_case(n_gadgets, 5, lens, SPOIL_EVERY)
    for pair in X.PARAMS + (X.GADGET_PIN,):
        res = X.resolve(k, strs, None, rows, None, t, *pair)
        resolved = {u for u, (first, n) in enumerate(res["rplace"]) if n > 1}
        per_tile = X.tile_starts(strs, resolved)
        assert max(a for a, _ in per_tile) <= 1024
        assert any(a >= 500 and b >= 100 for a, b in per_tile) and sum(a >= 500 for a, _ in per_tile) >= 3
        assert any(a <= 2 for a, _ in per_tile), "tiles inside long centres"
        first = next(i for i, (a, b) in enumerate(per_tile) if a >= 500 and b >= 100)
        at, inside = 0, []
        for u, s in enumerate(strs):
            if at // 4096 == first:
                inside.append(res["rplace"][u][1])
            at += len(s)
        assert {1, 2, 3, 4} == set(inside)


@pytest.mark.parametrize("k", (5, 31))
def test_a_ladder_resolves_every_centre(k):
    kk, strs, rows, t = X.ladder_case(LADDER_N, k)
    assert len(strs) == 3 * LADDER_N + 2
    for pair in X.PARAMS:
        res = X.resolve(k, strs, None, rows, None, t, *pair)
        assert res["stats"]["n_resolved"] == res["stats"]["n_candidates"] == LADDER_N and res["stats"]["n_copies_added"] == LADDER_N
    X.check_resolved(k, strs, rows, res)
    resolved = {u for u, (first, n) in enumerate(res["rplace"]) if n > 1}
    both = sum(1 for o, row in enumerate(rows) if o >> 1 in resolved for b in row if b >> 1 in resolved)
    assert both == 2 * (LADDER_N - 1), "every edge between two centres, and its mirror, is renamed at both ends"
    assert 0 < sum(X.verdict(rows, u, t, 2, 0)[1] == [1, 0] for u in resolved) < LADDER_N, "both permutations"
    if k == 5:
        assert min(a for a, _ in X.tile_starts(strs)[:-1]) >= 500


def test_small_ladders_and_gadgets_hold_too():
    for n in (1, 2, 3, 10):
        k, strs, rows, t = X.ladder_case(n, 5, seed=n)
        res = X.resolve(k, strs, None, rows, None, t, 2, 0)
        assert res["stats"]["n_resolved"] == n
        X.check_resolved(k, strs, rows, res)
    k, strs, rows, t = X.gadget_case(72, 21, GADGETS[21][1], SPOIL_EVERY)
    res = X.resolve(k, strs, None, rows, None, t, *X.GADGET_PIN)
    assert res["stats"]["n_resolved"] == 72 - 14 and len(strs) == sum(1 + 2 * p for p, _, _ in X.gadget_plan(72, SPOIL_EVERY))
    X.check_resolved(k, strs, rows, res)
