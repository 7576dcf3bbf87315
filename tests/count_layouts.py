"""Batches crafted for the launch geometry of k_count_windows (kmcex_amd/csrc/count_kernels.h) and the listing they must
give.  A lane rolls 16 consecutive windows, a wave reserves room for 1024, a block owns 4096 and stages 4096 + k - 1 bytes:
the text below is three blocks and a bit, its dirt sits on those edges, and every layout is a set of sequence boundaries
over that one text.  The expected listing is count_reads.count, checked once per case against count_reads.dict_count (the
plain-Python dictionary count).  No GPU import; shared by tests/test_gpu_count_geometry.py and tests/test_count_layouts_cpu.py;
not a test itself."""
import functools

import numpy as np

import count_reads as CR
import seq_reads as R

RUN, WAVE, BLOCK = 16, 1024, 4096                              # CNT_RUN, 64 lanes of it, CNT_WIN
PERIOD = 1500                                                  # the text repeats: every k-mer recurs about 8 times
N = 3 * BLOCK + 100
CI, CS = 1, 2 ** 32 - 1                                        # nothing filtered, nothing capped
KS = (5, 16, 17, 31, 32, 33, 55, 64)                           # every k a test of these batches uses
MIN_LISTED, MIN_MAX_COUNT = 150, 4

LAYOUTS = ("one_sequence", "cut_every_run", "all_length_k", "all_length_k_plus_1", "all_length_1", "shorter_than_k",
           "cuts_round_block_edge", "cuts_round_wave_edge", "empties_between", "random_with_empties")
LONG = ("one_sequence", "cuts_round_block_edge", "cuts_round_wave_edge", "empties_between", "random_with_empties")   # these keep long sequences


def text() -> np.ndarray:
    """N bases: a PERIOD-base genome tiled"""
    g = R.genome_ascii(PERIOD)
    return np.tile(g, N // PERIOD + 1)[:N].copy()


def n_positions(k: int):
    """where the dirty text holds N: the run, wave and block edges, the first and last halo byte of a tile, both ends"""
    return [0, RUN - 1, RUN, WAVE - 1, WAVE, BLOCK - 1, BLOCK, BLOCK + k - 2, BLOCK + k - 1, 2 * BLOCK - k, N - 1]


def dirty_text(k: int) -> np.ndarray:
    """the text with 15 lowercase stretches of 20 bytes (bases all the same), 15 IUPAC letters and the N of n_positions"""
    t = text()
    rng = np.random.default_rng(1000 + k)
    for s in rng.integers(0, N - 20, size=15):
        t[s:s + 20] |= 0x20
    pos = rng.integers(0, N, size=15)
    t[pos] = R.IUPAC[rng.integers(0, len(R.IUPAC) - 1, size=15)]       # (not N: those have their own places)
    t[n_positions(k)] = ord("N")
    return t


def _cuts(cuts, n=N) -> np.ndarray:
    """sorted cuts (repeats = empty sequences) -> offsets from 0 to n"""
    c = np.sort(np.asarray(list(cuts), dtype=np.int64))
    assert len(c) == 0 or (c[0] >= 0 and c[-1] <= n)
    return np.concatenate([[0], c, [n]]).astype(np.uint64)


def tail_bases(k: int) -> int:
    """the tail sequence of all_length_1: 200 bases hold at most 201 - k windows, fewer than MIN_LISTED from k = 52 on, so 2k more"""
    return 200 + 2 * k


def layout(name: str, k: int) -> np.ndarray:
    """the offsets [n_seqs + 1] of one layout over the N bases"""
    rng = np.random.default_rng(1 + k)                         # (a seed at which random_with_empties keeps a count of 4 at k = 64 too)
    if name == "one_sequence":
        return _cuts([])
    if name == "cut_every_run":                                # every boundary on a lane-run edge, every sequence longer than k
        length = -(-(k + 1) // RUN) * RUN
        return _cuts(range(length, N, length))
    if name == "all_length_k":
        return _cuts(range(k, N, k))
    if name == "all_length_k_plus_1":
        return _cuts(range(k + 1, N, k + 1))
    if name == "all_length_1":                                 # a boundary at every base, then one tail sequence so that something is listed
        return _cuts(range(1, N - tail_bases(k) + 1))
    if name == "shorter_than_k":
        lens = rng.integers(0, k, size=2 * N)
        c = np.cumsum(lens)
        return _cuts(c[c < N])                                 # (the last sequence is cut short at N: shorter still)
    if name == "cuts_round_block_edge":
        return _cuts(BLOCK + d for d in range(-k - 1, 3))
    if name == "cuts_round_wave_edge":
        return _cuts([WAVE + d for d in range(-k - 1, 3)] + [2 * BLOCK - k + 1, 2 * BLOCK])
    if name == "empties_between":                              # thousands of empty sequences inside one lane's walk, and across a block's bracket
        return _cuts([700] * 5001 + [BLOCK + 7] * 301)
    if name == "random_with_empties":
        c = rng.integers(1, N, size=400)
        return _cuts(np.repeat(c, rng.integers(1, 4, size=400)))
    raise KeyError(name)


def clip(off: np.ndarray, n: int) -> np.ndarray:
    """the layout over the first n bases only (what lay past n becomes empty sequences at the end)"""
    return np.minimum(off, np.uint64(n))


def split(buf: np.ndarray, off: np.ndarray):
    return [buf[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])]


def expected(buf: np.ndarray, off: np.ndarray, k: int):
    """(k-mers ascending, counts) of the batch with ci = 1 and no cap: count_reads.count, and the dictionary count agrees"""
    km, cnt = CR.count(buf, off, k, CI, CS)
    d = CR.dict_count(split(buf, off), k)
    ints = CR.packed_to_int(km)
    assert ints == sorted(d), "count_reads.count and dict_count list different k-mers"
    assert [d[x] for x in ints] == cnt.tolist(), "count_reads.count and dict_count disagree on a count"
    return km, cnt


@functools.lru_cache(maxsize=None)
def case(name: str, k: int, dirty: bool = False):
    """(bases, offsets, k-mers, counts) of one layout, read-only; asserts that the case is not vacuous"""
    buf = dirty_text(k) if dirty else text()
    off = layout(name, k)
    assert off[0] == 0 and off[-1] == N and np.all(np.diff(off.astype(np.int64)) >= 0)
    km, cnt = expected(buf, off, k)
    if name == "shorter_than_k":
        assert len(km) == 0
    else:
        assert len(km) >= MIN_LISTED, (name, k, dirty, len(km))
    if name in LONG:
        assert int(cnt.max()) >= MIN_MAX_COUNT, (name, k, dirty, int(cnt.max()))
    for a in (buf, off, km, cnt):
        a.setflags(write=False)
    return buf, off, km, cnt


def self_check(k: int) -> int:
    """every layout, clean and dirty, for one k; returns the cases checked"""
    n = 0
    for name in LAYOUTS:
        for dirty in (False, True):
            case(name, k, dirty)
            n += 1
    return n
