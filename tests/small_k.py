"""Small k (4 ... 15): the recipe of tests/golden/small_k_golden.json, the query set, and reads whose counted listing is a
given listing.  Shared by tests/golden/make_small_k_golden.py and the tests; not a test itself.

At k <= 7 the rest table's prefix is the whole k-mer (rest.hpp:78-83: pre_len == k, no suffix bytes), at k <= 9 the
(k-2)-mer hash never fills an 8-byte MurmurHash block, and the radix sorts of the count run over 8 ... 30 key bits."""
import json
import os

import numpy as np

import common
from kmcex_amd import synth

# name, k, ci, cs, nh, nb, draws (None: every canonical k-mer, a full rest table at k <= 7), seed
CASES = [
    ("k4_full", 4, 1, 255, 3, 1, None, 4),
    ("k4_part", 4, 2, 255, 5, 2, 80, 41),
    ("k5_full", 5, 3, 1023, 7, 3, None, 5),
    ("k5_part", 5, 1, 255, 4, 1, 300, 51),
    ("k6_full", 6, 2, 255, 6, 2, None, 6),
    ("k6_part", 6, 1, 4095, 9, 4, 1200, 61),
    ("k7_full", 7, 1, 8191, 12, 2, None, 7),
    ("k7_part", 7, 3, 1023, 8, 5, 5000, 71),
    ("k8", 8, 1, 2047, 10, 5, 20000, 8),
    ("k9", 9, 2, 4095, 11, 3, 20000, 9),
    ("k10", 10, 1, 1023, 7, 1, 60000, 10),
    ("k11", 11, 3, 1023, 7, 6, 40000, 11),
    ("k12", 12, 1, 255, 5, 2, 30000, 12),
    ("k13", 13, 2, 1023, 9, 4, 30000, 13),
    ("k14", 14, 1, 4095, 3, 3, 10000, 14),
    ("k15", 15, 1, 1023, 8, 8, 30000, 15),
]
CASE = {c[0]: c for c in CASES}
ALL_QUERIES_K = 10                                             # up to this k the query set is every one of the 4^k k-mers
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_k_golden.json")


def all_canonical(k: int) -> np.ndarray:
    """every canonical k-mer, ascending (136 at k = 4, 8192 at k = 7)"""
    x = np.arange(4 ** k, dtype=np.uint64)
    return x[synth.canonical(x, k) == x]


def listing(name: str):
    """(k-mers ascending, counts) of a case: a KMC1 listing within [ci, cs]"""
    _, k, ci, cs, _, _, draws, seed = CASE[name]
    km = all_canonical(k) if draws is None else synth.sort_unique(synth.canonical(synth.random_kmers(draws, k, seed_k=seed), k))
    return km, synth.d1_counts(len(km), ci, cs, seed_c=seed)


def queries(k: int, km: np.ndarray) -> np.ndarray:
    """every possible k-mer for k <= ALL_QUERIES_K, else the query_set recipe of tests/common.py"""
    if k <= ALL_QUERIES_K:
        return np.arange(4 ** k, dtype=np.uint64)
    return common.query_set(km, k)


def reads_for_listing(km: np.ndarray, cnt: np.ndarray, k: int, ci: int, cs: int, seed: int):
    """(uint8 bases, uint64 offsets) whose counted listing at (ci, cs) is exactly (km, cnt): every k-mer written c times
    (half of them reverse-complemented, a tenth in lowercase), one k-mer more than cs times where c == cs (the cap), and
    k-mers outside the listing ci - 1 times (the floor).  Each k-mer is followed by an N, 16 of them to a sequence, so no
    window spans two of them."""
    rng = np.random.default_rng(seed)
    reps = cnt.astype(np.int64)
    top = np.nonzero(reps == cs)[0]
    reps[top] += rng.integers(1, cs + 1, size=len(top))
    occ = np.repeat(km, reps)
    if ci > 1:
        other = synth.sort_unique(synth.canonical(synth.random_kmers(4 * len(km) + 64, k, seed_k=seed + 1000), k))
        other = np.setdiff1d(other, km)[:2000]
        occ = np.concatenate([occ, np.repeat(other, ci - 1)])
    occ = occ[rng.permutation(len(occ))]
    flip = rng.random(len(occ)) < 0.5
    occ[flip] = synth.revcomp(occ[flip], k)
    rows = np.empty((len(occ), k + 1), dtype=np.uint8)
    rows[:, :k] = synth.to_ascii(occ, k)
    rows[rng.random(len(occ)) < 0.1, :k] += 32
    rows[:, k] = ord("N")
    per = 16
    ends = np.minimum(np.arange(per, len(occ) + per, per), len(occ))
    offsets = np.zeros(len(ends) + 1, dtype=np.uint64)
    offsets[1:] = ends.astype(np.uint64) * np.uint64(k + 1)
    return rows.reshape(-1), offsets


def load_golden() -> dict:
    with open(GOLDEN_PATH) as f:
        return json.load(f)["cases"]
