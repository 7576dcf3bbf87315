"""The inputs of tests/test_gpu_two_word_seqs.py proven good on the CPU oracle alone, without the code under test: the NumPy
restatement of quirk Q4 (tests/as_asked.py) equals the oracle's string min_kmer, the models built from as-asked listings answer
the windows of their texts, and the oracle-driven rules correct, edit, polish, walk and look ahead on them at two-word k --
which is what the suite's other k > 32 data never does.

Figures of the oracle, recipe of tests/as_asked.py (genome 20 000 with both strands, 400 reads, thr = 1, min_support = 1):
   k   windows answered >= 1   n_corrected / n_unfixable   edits sub / del / ins   polish, 3 passes
  33   39 933 of 39 936        178 / 373                    90 / 41 / 26            93 / 43 / 28
  34   39 931 of 39 934        165 / 356                    69 / 33 / 25
  35   39 926 of 39 932        126 / 392                    69 / 23 / 27
  55   39 883 of 39 892          8 / 242                     4 /  3 /  1
  63   19 938 of 39 876          5 / 711                     4 /  0 /  0
  64   39 874 of 39 874        274 / 223                   120 / 61 / 57            120 / 68 / 62
The model is a lossy structure: the oracle answers 0 for three to nine LISTED k-mers of a text at k = 33, 34, 35 and 55 (the
neighbour vote of kmer_to_bin), so "every window" is asserted of the listing -- the as-asked form of every window is in it --
and the oracle's own misses are pinned, as the found count of k = 63 is.  The GPU has to agree with every one of them."""
import numpy as np
import pytest

import as_asked as A
import oracle_lib as O
import seq_correct_ref as S
import seq_edit_ref as E
import seq_extend_ref as X
import seq_reads as R
from kmcex_amd import synth

# listed windows of genome + reverse complement that the oracle answers 0 (k = 63: see test_models_answer_their_texts)
ORACLE_MISSES = {33: 3, 34: 3, 35: 6, 55: 9, 64: 0}
FOUND_K63 = 19938


def _equal_to_own_rc(k: int, n: int, rng) -> np.ndarray:
    """k-mers whose low word equals rc: its last k - 32 bases are T and the 64 - k bases before them are their own reverse
    complement (so 64 - k is even); at k = 64 rc is all ones and the low word is 32 T"""
    m = k - 32
    half = (32 - m) // 2
    assert (32 - m) % 2 == 0
    h = rng.integers(0, 4, size=(n, half))
    codes = np.concatenate([rng.integers(0, 4, size=(n, m)), h, 3 - h[:, ::-1], np.full((n, m), 3)], axis=1)
    return synth.from_strings(["".join("ACGT"[c] for c in row) for row in codes], k)


@pytest.mark.parametrize("k", [33, 34, 35, 40, 55, 63, 64])
def test_as_asked_is_the_oracles_min_kmer(k):
    rng = np.random.default_rng(k)
    km = synth.random_kmers(2000, k, seed_k=1000 + k).reshape(-1, 2)
    if k % 2 == 0:                                                # (for odd k no low word equals its rc)
        eq = _equal_to_own_rc(k, 50, rng)
        km = np.concatenate([km, eq])
    got = A.as_asked(km, k)
    want = synth.from_strings([O.min_kmer(s) for s in synth.to_strings(km, k)], k)
    assert np.array_equal(got, want)
    changed = (got != km).any(axis=1)
    assert k == 64 or (changed[:2000].sum() > 500 and (~changed[:2000]).sum() > 500)     # both forms occur (at k = 64 every k-mer is asked as itself)
    if k % 2 == 0:
        strs = synth.to_strings(eq, k)
        assert not changed[2000:].any() and [O.min_kmer(s) for s in strs] == strs       # u == rc: asked as itself


@pytest.mark.parametrize("k", [33, 34, 35, 55, 63, 64])
def test_models_answer_their_texts(k):
    c = A.genome_case(k)
    buf, off = R.flatten(c["text"])
    windows = A.forward_windows(buf, off, k)
    asked = A.as_asked(windows, k)
    # the listing holds the as-asked form of EVERY window, with the number of windows that take it (capped at cs)
    key = lambda a: a[:, 0].astype(object) << 64 | a[:, 1].astype(object)
    pos = np.searchsorted(key(c["km"]), key(asked))
    assert (pos < len(c["km"])).all() and np.array_equal(c["km"][pos], asked)
    assert np.array_equal(np.minimum(np.bincount(pos, minlength=len(c["cnt"])), A.PARAMS[k][1]), c["cnt"])
    assert np.all(c["km"][1:, 0] >= c["km"][:-1, 0]) and len(np.unique(c["km"], axis=0)) == len(c["km"])
    ans = R.oracle_per_base(c["o"], buf, off, k)
    valid = R.valid_mask(off, k)
    assert valid.sum() == len(windows) == 2 * (A.N_GENOME - k + 1) and (ans[~valid] == -1).all()
    found = int((ans[valid] >= 1).sum())
    print(k, "windows", len(windows), "answered >= 1", found, "listing", len(c["cnt"]), "entries with hi == 0", int((c["km"][:, 0] == 0).sum()))
    if k != 63:
        assert found == len(windows) - ORACLE_MISSES[k]
        assert found >= 0.9997 * len(windows)
        assert k == 64 or (c["km"][:, 0] == 0).sum() > 10000      # the (0, rc) form is the common one
    else:
        # half the windows (low word starting with G or T) take one of TWO (0, rc) forms, A...A C T...T and A...A A T...T:
        # thousands of windows each, counted to the ceiling, and the oracle answers 0 for both
        big = np.nonzero(c["cnt"] == A.PARAMS[k][1])[0]
        assert len(big) == 2 and (c["km"][big, 0] == 0).all() and (c["km"][:, 0] == 0).sum() == 2
        assert (np.bincount(pos)[big] > 4095).all() and np.bincount(pos)[big].sum() == len(windows) - found
        assert c["o"].query_packed(k, c["km"][big]).tolist() == [0, 0]
        assert found == FOUND_K63


@pytest.mark.parametrize("k", [33, 34, 35, 55, 63, 64])
def test_reads_are_corrected_edited_and_polished(k):
    """non-degeneracy, judged on the oracle's results alone"""
    c = A.genome_case(k)
    out, rec = A.want_correct(k, 1, 1)
    tc = S.tallies(rec, c["buf"], out, c["off"])
    ed, erec = A.want_edit(k, 1, 1, 7)
    te = E.tallies(erec, ed)
    print(k, "correct", tc)
    print(k, "edit", te)
    assert R.dirty_windows(c["buf"], c["off"], k) > 100 and R.dirty_windows(c["ebuf"], c["eoff"], k) > 100
    if k in (55, 63):                                             # half their windows ignore their first 23 - 31 bases: few sites verify
        assert tc["n_sites"] >= 100 and te["n_sites"] >= 100
        return
    assert tc["n_corrected"] >= 100 and tc["n_unfixable"] >= 100
    assert te["n_sub"] >= 50 and te["n_del"] >= 15 and te["n_ins"] >= 15
    if k in (33, 64):
        p = A.want_polish(k, 1, 1, 8)
        print(k, "polish", {f: int(p["records"][f].sum()) for f in ("n_sub", "n_del", "n_ins")}, "passes", p["passes_run"], [len(h["edited"]) for h in p["history"]])
        assert p["passes_run"] >= 2 and len(p["history"][1]["edited"]) >= 1
        assert A.want_polish(k, 1, 1, 1)["passes_run"] == 1


@pytest.mark.parametrize("k", [32, 33, 34, 35, 63, 64])
def test_walks_run_on_and_look_ahead(k):
    c = A.extend_case(k)
    assert len(c["seeds"]) == A.N_SEEDS + A.N_REVERSED + 2 and c["seeds"][-2:] == [b"", b"N" * k]
    stops = set()
    for thr in (1, 3):
        for depth in (0, 1, 2, 3):
            ext, rec = A.want_extend(k, thr, depth)
            t = X.tallies(rec)
            print(k, "thr", thr, "depth", depth, t)
            stops |= set(np.unique(rec["stop"]).tolist())
            if depth == 3:
                assert t["n_lookahead"] >= 500 and t["n_ext"] >= 1000
            if depth == 0:
                assert t["n_lookahead"] == 0
            if k == 32 and thr == 3 and depth >= 2:
                assert t["max_ext"] >= 1
    assert {X.BRANCH, X.JOIN, X.DEAD_END, X.BAD_SEED} <= stops
    # walks to the left of reversed seeds: what left = True is tested with
    l_ext, l_rec, _ = X.extend_left(*R.flatten(c["seeds"][A.N_SEEDS:A.N_SEEDS + 50]), k, 1, A.MAX_EXT, 2, S.oracle_rows(c["o"], k))
    assert int(l_rec["n_ext"].sum()) >= 100
