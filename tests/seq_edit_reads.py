"""Seeded reads with substitutions AND single-base insertions / deletions over a GENOME_CASES sequence, for kmx_edit_seqs:
seq_reads.make_reads' reads (strand flips, runs of N, lowercase stretches, IUPAC letters, the special short / long reads) with
the substitution step replaced by one draw per true base.  Shared by tests/golden/make_seq_edit_golden.py, the tests and
tools/bench_seq_edit.py; not a test itself."""
import numpy as np

import seq_reads as R

SUB_RATE, DROP_RATE, EXTRA_RATE = 0.004, 0.003, 0.003              # u < 0.004: substitute; < 0.007: drop; < 0.010: keep and append a random base


def with_errors(t: np.ndarray, rng) -> np.ndarray:
    """one draw u per true base: substitute it, drop it, or keep it and append a random base"""
    u = rng.random(len(t))
    sub = np.nonzero(u < SUB_RATE)[0]
    r = t.copy()
    r[sub] = R.ACGT[(np.searchsorted(R.ACGT, r[sub]) + rng.integers(1, 4, size=len(sub))) % 4]
    extra = (u >= SUB_RATE + DROP_RATE) & (u < SUB_RATE + DROP_RATE + EXTRA_RATE)
    appended = R.ACGT[rng.integers(0, 4, size=len(t))]
    pairs = np.stack([r, appended], axis=1)
    keep = np.stack([~((u >= SUB_RATE) & (u < SUB_RATE + DROP_RATE)), extra], axis=1)
    return pairs[keep]


def make_reads(n_bases: int, k: int, n_reads: int = 3000, len_min: int = 80, len_max: int = 300, seed: int = 23, long_read: int = 7000,
               dirty: bool = True):
    """-> (reads, truths): lists of bytes.  The truth of a read is what it was cut as, strand flip included, before the errors
    and the dirty bytes (N runs, lowercase, IUPAC; none with dirty = False)."""
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(seed)
    reads, truths = [], []
    for i in range(n_reads):
        ln = int(rng.integers(len_min, len_max + 1))
        a = int(rng.integers(0, n_bases - ln))
        t = g[a:a + ln].copy()
        if i % 2:
            t = R._COMP[t[::-1]]
        r = with_errors(t, rng)
        ln = len(r)
        kind = i % 10 if dirty and ln else -1
        if kind == 3:                                          # a run of N
            s, n = int(rng.integers(0, ln)), int(rng.integers(1, 12))
            r[s:s + n] = ord("N")
        elif kind == 5:                                        # soft-masked (lowercase) stretch
            s, n = int(rng.integers(0, ln)), int(rng.integers(5, 60))
            r[s:s + n] = r[s:s + n] + 32
        elif kind == 7:                                        # a few IUPAC letters
            pos = rng.integers(0, ln, size=int(rng.integers(1, 4)))
            r[pos] = R.IUPAC[rng.integers(0, len(R.IUPAC), size=len(pos))]
        reads.append(r.tobytes())
        truths.append(t.tobytes())
    for ln in (0, k - 1, k, k + 1, 0, k, k - 1):
        a = int(rng.integers(0, n_bases - max(ln, 1)))
        reads.append(g[a:a + ln].tobytes())
        truths.append(reads[-1])
    a = int(rng.integers(0, n_bases - long_read))
    lr = g[a:a + long_read].copy()
    truths.append(lr.tobytes())
    lr = with_errors(lr, rng)
    if dirty:
        lr[len(lr) // 3:len(lr) // 3 + 40] = ord("N")
        lr[len(lr) // 2:len(lr) // 2 + 100] += 32
    reads.append(lr.tobytes())
    order = rng.permutation(len(reads))                        # the special reads anywhere in the batch
    return [reads[j] for j in order], [truths[j] for j in order]


def dirty_reads(reads) -> np.ndarray:
    """True for the reads that hold a byte outside uppercase ACGT"""
    return np.array([bool(len(r)) and not np.isin(np.frombuffer(r, dtype=np.uint8), R.ACGT).all() for r in reads])
