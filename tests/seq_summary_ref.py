"""NumPy reference of kmx_summarise_seqs: per-sequence records from the per-base answers of kmx_query_seqs (or of the CPU
oracle, seq_reads.oracle_per_base).  Shared by tests/golden/make_seq_summary_golden.py and the tests; not a test itself."""
import hashlib

import numpy as np

DTYPE = np.dtype([("n_windows", "<u8"), ("sum", "<u8"), ("min", "<i4"), ("max", "<i4"), ("n_ge", "<u8", (3,)),
                  ("first_below", "<u8"), ("last_below", "<u8")])


def summarise(per_base: np.ndarray, offsets: np.ndarray, k: int, thr=()) -> np.ndarray:
    """per_base: int32[n_bases], -1 where no window of a sequence starts; offsets: uint64[n_seqs + 1] -> DTYPE[n_seqs].
    Sequence i's windows are the first max(len_i - k + 1, 0) entries of per_base[offsets[i] : offsets[i + 1]]."""
    per_base = np.asarray(per_base, dtype=np.int32)
    offsets = np.asarray(offsets).astype(np.int64)
    thr = [int(t) for t in thr]
    assert len(thr) <= 3
    n = len(offsets) - 1
    out = np.zeros(n, dtype=DTYPE)
    lens = np.diff(offsets)
    nw = np.maximum(lens - k + 1, 0)
    out["n_windows"] = nw
    out["min"] = out["max"] = -1
    out["first_below"] = out["last_below"] = nw
    has = np.nonzero(nw > 0)[0]
    if len(has) == 0:
        return out
    # the windows of all sequences back to back, and where each sequence's run starts among them
    starts = np.zeros(len(has) + 1, dtype=np.int64)
    starts[1:] = np.cumsum(nw[has])
    seq_of = np.repeat(np.arange(len(has)), nw[has])
    within = np.arange(starts[-1], dtype=np.int64) - starts[seq_of]
    a = per_base[offsets[has][seq_of] + within].astype(np.int64)
    assert (a >= 0).all(), "a window without an answer"
    at = starts[:-1]
    out["sum"][has] = np.add.reduceat(a, at)
    out["min"][has] = np.minimum.reduceat(a, at)
    out["max"][has] = np.maximum.reduceat(a, at)
    for j, t in enumerate(thr):
        out["n_ge"][has, j] = np.add.reduceat((a >= t).astype(np.int64), at)
    if thr:
        below = a < thr[0]
        big = np.int64(1) << 62
        first = np.minimum.reduceat(np.where(below, within, big), at)
        last = np.maximum.reduceat(np.where(below, within, -1), at)
        some = first < big
        out["first_below"][has[some]] = first[some]
        out["last_below"][has[some]] = last[some]
    return out


def sha_records(rec: np.ndarray) -> str:
    """sha256 of the records' bytes (64 per sequence, little-endian)"""
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 64
    return hashlib.sha256(rec.tobytes()).hexdigest()


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """field for field: the bytes of two record arrays"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 64 and a.shape == b.shape and a.tobytes() == b.tobytes()


def tallies(rec: np.ndarray) -> dict:
    """the per-read tallies the GPU test asserts on the oracle's records (thr = three thresholds)"""
    nw, ge = rec["n_windows"].astype(np.int64), rec["n_ge"].astype(np.int64)
    w = nw > 0
    return {
        "reads_with_windows": int(w.sum()),
        "all_known": int((w & (ge[:, 0] == nw)).sum()),
        "partly_known": int(((ge[:, 0] > 0) & (ge[:, 0] < nw)).sum()),
        "median_reaches_thr1": int((w & (2 * ge[:, 1] > nw)).sum()),
        "median_below_thr1": int((w & ~(2 * ge[:, 1] > nw)).sum()),
        "median_reaches_thr2": int((w & (2 * ge[:, 2] > nw)).sum()),
    }
