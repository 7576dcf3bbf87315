"""Reference of kmx_correct_seqs in NumPy / Python: the rule of include/kmx.h over the per-base answers of kmx_query_seqs (or
of the CPU oracle, seq_reads.oracle_per_base) and a callback that answers rows of k bytes (kmx_query_ascii / the oracle).
Shared by tests/golden/make_seq_correct_golden.py, the tests and tools/bench_seq_correct.py; not a test itself."""
import ctypes as C
import hashlib

import numpy as np

FIELDS = ("n_windows", "n_weak", "n_runs", "n_sites", "n_corrected", "n_ambiguous", "n_unfixable", "reserved")
DTYPE = np.dtype([(f, "<u8") for f in FIELDS])
ACGT = b"ACGT"


def runs_of(flags: np.ndarray):
    """[(first, last)] of the maximal stretches of True"""
    w = np.concatenate([[0], flags.astype(np.int8), [0]])
    d = np.diff(w)
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def close_gaps(weak: np.ndarray) -> np.ndarray:
    """a window that is not weak between two weak ones counts as weak for run forming (judged on `weak` itself)"""
    c = weak.copy()
    if len(weak) >= 3:
        c[1:-1] |= weak[:-2] & weak[2:]
    return c


def sites_of_run(s: int, e: int, nw: int, k: int):
    """the shape table: [(base, v0, v1)] of the run [s, e] of a sequence with nw windows"""
    ln = e - s + 1
    has_l, has_r = s > 0, e < nw - 1
    if not has_l and not has_r:
        return []
    if has_r and not has_l:
        return [(e, max(s, e - k + 1), e)]
    if has_l and not has_r:
        return [(s + k - 1, s, min(e, s + k - 1))]
    if ln < k:
        return []
    if ln == k:
        return [(e, s, e)]
    return [(s + k - 1, s, min(s + k - 1, e - k)), (e, max(e - k + 1, s + k), e)]


def plan(per_base: np.ndarray, offsets: np.ndarray, k: int, thr: int, min_support: int):
    """-> (records with n_windows, n_weak, n_runs filled in, the tried sites [(sequence, b, v0, v1)] in absolute positions)"""
    per_base = np.asarray(per_base, dtype=np.int32)
    off = np.asarray(offsets).astype(np.int64)
    rec = np.zeros(len(off) - 1, dtype=DTYPE)
    sites = []
    for i in range(len(off) - 1):
        a, z = int(off[i]), int(off[i + 1])
        nw = max(z - a - k + 1, 0)
        rec["n_windows"][i] = nw
        if nw == 0:
            continue
        ans = per_base[a:a + nw]
        assert (ans >= 0).all(), "a window without an answer"
        weak = ans < thr
        rec["n_weak"][i] = int(weak.sum())
        if not weak.any():
            continue
        for s, e in runs_of(close_gaps(weak)):
            rec["n_runs"][i] += 1
            for b, v0, v1 in sites_of_run(s, e, nw, k):
                if v1 - v0 + 1 >= min_support:
                    sites.append((i, a + b, a + v0, a + v1))
    return rec, sites


def correct(per_base, buf, offsets, k: int, thr: int, min_support: int, query_rows):
    """-> (corrected bases uint8[n_bases], records DTYPE[n_seqs], verification windows asked).  query_rows(uint8[n, k]) ->
    int32[n]: the answer of each row of k bytes.  Every candidate of every site is asked in full (no early stop): the verdict
    of a candidate is a conjunction, so the result is the same."""
    assert 1 <= min_support <= 64
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n_bases = int(np.asarray(offsets)[-1])
    out = buf[:n_bases].copy()
    rec, sites = plan(per_base, offsets, k, thr, min_support)
    rows, owner = [], []
    for j, (_, b, v0, v1) in enumerate(sites):
        for ci, c in enumerate(ACGT):
            if buf[b] == c:
                continue
            for p in range(v0, v1 + 1):
                r = buf[p:p + k].copy()
                r[b - p] = c
                rows.append(r)
                owner.append(j * 4 + ci)
    ok = np.ones(len(sites) * 4, dtype=bool)
    if rows:
        ans = np.asarray(query_rows(np.stack(rows)), dtype=np.int32)
        np.logical_and.at(ok, np.array(owner), ans >= thr)
    for j, (i, b, _, _) in enumerate(sites):
        cand = [ci for ci, c in enumerate(ACGT) if buf[b] != c and ok[j * 4 + ci]]
        rec["n_sites"][i] += 1
        if len(cand) == 1:
            out[b] = ACGT[cand[0]]
            rec["n_corrected"][i] += 1
        elif cand:
            rec["n_ambiguous"][i] += 1
        else:
            rec["n_unfixable"][i] += 1
    return out, rec, len(rows)


def oracle_rows(o, k: int, threads: int = 8):
    """the callback over the CPU oracle (oracle_lib.OracleModel)"""
    def ask(rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        out = np.zeros(len(rows), dtype=np.int32)
        if len(rows) and o.L.kmo_query_ascii(o.h, C.cast(rows.ctypes.data, C.c_char_p), k, k, len(rows), out.ctypes.data, threads):
            raise RuntimeError("kmo_query_ascii")
        return out
    return ask


def oracle_correct(o, buf, offsets, k: int, thr: int, min_support: int):
    """the rule driven by the CPU oracle alone"""
    import seq_reads as R
    return correct(R.oracle_per_base(o, buf, offsets, k), buf, offsets, k, thr, min_support, oracle_rows(o, k))


def same(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 64 and a.shape == b.shape and a.tobytes() == b.tobytes()


def sha_records(rec: np.ndarray) -> str:
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 64
    return hashlib.sha256(rec.tobytes()).hexdigest()


def sha_bases(out: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(out, dtype=np.uint8).tobytes()).hexdigest()


def tallies(rec: np.ndarray, buf: np.ndarray, out: np.ndarray, offsets: np.ndarray) -> dict:
    """what the tests assert on the ORACLE's result before the GPU is compared, and the golden file pins"""
    n = int(np.asarray(offsets)[-1])
    buf, out = np.asarray(buf[:n]), np.asarray(out[:n])
    changed = buf != out
    t = {f: int(rec[f].sum()) for f in FIELDS}
    t["corrected_non_acgt"] = int((changed & ~np.isin(buf, np.frombuffer(ACGT, dtype=np.uint8))).sum())
    t["corrected_n"] = int((changed & (buf == ord("N"))).sum())
    c = np.concatenate([[0], np.cumsum(changed)])
    off = np.asarray(offsets).astype(np.int64)
    t["reads_changed"] = int((c[off[1:]] - c[off[:-1]] > 0).sum())
    return t
