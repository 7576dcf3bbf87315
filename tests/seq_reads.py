"""Seeded reads over a GENOME_CASES sequence for the sequence query (kmx_query_seqs), and the per-base answers the CPU
oracle gives them.  Shared by tests/golden/make_seq_golden.py and the tests; not a test itself."""
import numpy as np

from kmcex_amd import synth

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = np.frombuffer(b"RYKMSWBDHVN", dtype=np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
_COMP[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)

# the recipe of tests/golden/seq_golden.json: reads of one genome case
RECIPE = {"n_reads": 3000, "len_min": 80, "len_max": 300, "sub_rate": 0.01, "seed": 23, "long_read": 7000}


def genome_ascii(n_bases: int, seed: int = 11) -> np.ndarray:
    """synth.genome_bases as uint8 ASCII (ACGT)"""
    return ACGT[synth.genome_bases(n_bases, seed).astype(np.int64)]


def make_reads(n_bases: int, k: int, n_reads: int = 3000, len_min: int = 80, len_max: int = 300, sub_rate: float = 0.01,
               seed: int = 23, long_read: int = 7000):
    """Reads of 80-300 bases from random positions of the genome, half reverse-complemented, with 1 % substitutions, runs
    of N, lowercase stretches and a few IUPAC letters; plus an empty read, reads of k - 1, k and k + 1 bases and one read
    of `long_read` bases (longer than a test chunk).  Returns a list of bytes."""
    g = genome_ascii(n_bases)
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads):
        ln = int(rng.integers(len_min, len_max + 1))
        a = int(rng.integers(0, n_bases - ln))
        r = g[a:a + ln].copy()
        if i % 2:
            r = _COMP[r[::-1]]
        subs = np.nonzero(rng.random(ln) < sub_rate)[0]
        r[subs] = ACGT[(np.searchsorted(ACGT, r[subs]) + rng.integers(1, 4, size=len(subs))) % 4]
        kind = i % 10
        if kind == 3:                                          # a run of N
            s, n = int(rng.integers(0, ln)), int(rng.integers(1, 12))
            r[s:s + n] = ord("N")
        elif kind == 5:                                        # soft-masked (lowercase) stretch
            s, n = int(rng.integers(0, ln)), int(rng.integers(5, 60))
            r[s:s + n] = r[s:s + n] + 32
        elif kind == 7:                                        # a few IUPAC letters
            pos = rng.integers(0, ln, size=int(rng.integers(1, 4)))
            r[pos] = IUPAC[rng.integers(0, len(IUPAC), size=len(pos))]
        reads.append(r.tobytes())
    for ln in (0, k - 1, k, k + 1, 0, k, k - 1):
        a = int(rng.integers(0, n_bases - max(ln, 1)))
        reads.append(g[a:a + ln].tobytes())
    a = int(rng.integers(0, n_bases - long_read))
    lr = g[a:a + long_read].copy()
    lr[long_read // 3:long_read // 3 + 40] = ord("N")
    lr[long_read // 2:long_read // 2 + 100] += 32
    reads.append(lr.tobytes())
    order = rng.permutation(len(reads))                        # the special reads anywhere in the batch
    return [reads[j] for j in order]


def flatten(reads):
    """list of bytes -> (uint8 bases, uint64 offsets[n + 1])"""
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), offsets


def valid_mask(offsets: np.ndarray, k: int) -> np.ndarray:
    """True at every base where a k-mer window starts inside its sequence"""
    offsets = offsets.astype(np.int64)
    lens = np.diff(offsets)
    end = np.repeat(offsets[1:], lens)
    return np.arange(int(offsets[-1]), dtype=np.int64) + k <= end


def oracle_per_base(o, buf: np.ndarray, offsets: np.ndarray, k: int, threads: int = 8) -> np.ndarray:
    """The CPU oracle's kmer_to_occ of every window of the flat buffer (stride 1), -1 where no window of a sequence starts"""
    import ctypes as C
    n_bases = int(offsets[-1])
    out = np.full(n_bases, -1, dtype=np.int32)
    if n_bases >= k:
        got = np.zeros(n_bases - k + 1, dtype=np.int32)
        buf = np.ascontiguousarray(buf[:n_bases], dtype=np.uint8)
        if o.L.kmo_query_ascii(o.h, C.cast(buf.ctypes.data, C.c_char_p), k, 1, len(got), got.ctypes.data, threads):
            raise RuntimeError("kmo_query_ascii")
        out[:len(got)] = got
    out[~valid_mask(offsets, k)] = -1
    return out


def dirty_windows(buf: np.ndarray, offsets: np.ndarray, k: int) -> int:
    """windows of the sequences that hold a byte outside uppercase ACGT"""
    bad = ~np.isin(buf[:int(offsets[-1])], ACGT)
    c = np.concatenate([[0], np.cumsum(bad)])
    n = len(bad)
    starts = np.nonzero(valid_mask(offsets, k))[0]
    return int(((c[np.minimum(starts + k, n)] - c[starts]) > 0).sum())
