"""Reference of kmx_extend_seqs in NumPy / Python: the rule of include/kmx.h over a callback that answers rows of k bytes
(kmx_query_ascii / KModel.kmer_to_occ_rows / the CPU oracle).  All live walks take a step together, so a step is a few calls
of the callback whatever the number of seeds.  Shared by tests/golden/make_seq_extend_golden.py, the tests and
tools/bench_seq_extend.py; not a test itself."""
import hashlib

import numpy as np

FIELDS = ("n_ext", "stop", "seed_occ", "min_occ", "max_occ", "n_lookahead", "sum_occ")
DTYPE = np.dtype([("n_ext", "<u4"), ("stop", "<u4"), ("seed_occ", "<i4"), ("min_occ", "<i4"), ("max_occ", "<i4"), ("n_lookahead", "<u4"), ("sum_occ", "<u8")])
DEAD_END, BRANCH, JOIN, CYCLE, MAX_EXT, BAD_SEED = 1, 2, 3, 4, 5, 6
STOP_NAMES = {DEAD_END: "dead_end", BRANCH: "branch", JOIN: "join", CYCLE: "cycle", MAX_EXT: "max_ext", BAD_SEED: "bad_seed"}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
_COMP[ACGT] = ACGT[::-1]


def revcomp(s: bytes) -> bytes:
    """reverse complement of an ACGT string; any other byte stays what it is (and makes a bad seed where it was one)"""
    return _COMP[np.frombuffer(s, dtype=np.uint8)[::-1]].tobytes()


def _children(x: np.ndarray, forward: bool) -> np.ndarray:
    """[m, k] -> [m, 4, k]: x[1:] + c (forward) or c + x[:-1] (backward), c in ACGT order"""
    m, k = x.shape
    out = np.empty((m, 4, k), dtype=np.uint8)
    if forward:
        out[:, :, :k - 1] = x[:, None, 1:]
        out[:, :, k - 1] = ACGT[None, :]
    else:
        out[:, :, 1:] = x[:, None, :k - 1]
        out[:, :, 0] = ACGT[None, :]
    return out


class _Asker:
    def __init__(self, ask, k):
        self.ask, self.k, self.n = ask, k, 0

    def __call__(self, rows):
        rows = np.ascontiguousarray(rows.reshape(-1, self.k))
        self.n += len(rows)
        return np.asarray(self.ask(rows), dtype=np.int64) if len(rows) else np.zeros(0, dtype=np.int64)


def _sup(q, x: np.ndarray, d: int, thr: int, forward: bool) -> np.ndarray:
    """sup_f / sup_b of every row of x; only the children of solid nodes are asked about"""
    if d == 0 or len(x) == 0:
        return np.ones(len(x), dtype=bool)
    ch = _children(x, forward)
    solid = (q(ch) >= thr).reshape(len(x), 4)
    idx = np.nonzero(solid)
    ok = np.zeros((len(x), 4), dtype=bool)
    ok[idx] = _sup(q, ch[idx], d - 1, thr, forward)
    return ok.any(axis=1)


def extend(buf: np.ndarray, offsets: np.ndarray, k: int, thr: int, max_ext: int, depth: int, ask):
    """-> (uint8 ext [n_seqs, max_ext], DTYPE records [n_seqs], rows asked).  ask(rows uint8 [m, k]) -> m answers."""
    assert 1 <= max_ext <= 65536 and 0 <= depth <= 3
    off = np.asarray(offsets).astype(np.int64)
    buf = np.asarray(buf, dtype=np.uint8)
    n = len(off) - 1
    ext = np.zeros((n, max_ext), dtype=np.uint8)
    rec = np.zeros(n, dtype=DTYPE)
    rec["seed_occ"] = rec["min_occ"] = rec["max_occ"] = -1
    q = _Asker(ask, k)
    good = np.zeros(n, dtype=bool)
    firsts = np.zeros((n, k), dtype=np.uint8)
    for i in range(n):
        if off[i + 1] - off[i] >= k:
            tail = buf[off[i + 1] - k:off[i + 1]]
            if np.isin(tail, ACGT).all():
                good[i] = True
                firsts[i] = tail
    rec["stop"][~good] = BAD_SEED
    live = np.nonzero(good)[0]
    if len(live):
        rec["seed_occ"][live] = q(firsts[live])
    cur = firsts[live].copy()
    while len(live):
        m = len(live)
        a = q(_children(cur, True)).reshape(m, 4)
        nxt_pred = _children(cur, False)                           # d + cur[:-1] ...
        nxt_pred[:, :, 1:] = cur[:, None, 1:]                       # ... but the rule asks d + cur[1:]: the predecessors of nxt
        b = q(nxt_pred).reshape(m, 4)
        S = a >= thr
        P = (b >= thr) & (ACGT[None, :] != cur[:, :1])
        looked = np.zeros(m, dtype=bool)
        if depth > 0:
            tie = S.sum(axis=1) > 1
            idx = np.nonzero(S & tie[:, None])
            if len(idx[0]):
                S[idx] = _sup(q, _children(cur, True)[idx], depth, thr, True)
            idx = np.nonzero(P)
            if len(idx[0]):
                P[idx] = _sup(q, nxt_pred[idx], depth, thr, False)
                looked[idx[0]] = True
            looked |= tie
        ns = S.sum(axis=1)
        stop = np.zeros(m, dtype=np.int64)
        stop[P.any(axis=1)] = JOIN
        stop[ns > 1] = BRANCH
        stop[ns == 0] = DEAD_END
        c = S.argmax(axis=1)
        nxt = np.concatenate([cur[:, 1:], ACGT[c][:, None]], axis=1)
        go = stop == 0
        stop[go & (nxt == firsts[live]).all(axis=1)] = CYCLE
        go = stop == 0
        g = live[go]
        a_c = a[np.arange(m), c][go]
        ne = rec["n_ext"][g].astype(np.int64)
        ext[g, ne] = ACGT[c[go]]
        first_step = ne == 0
        rec["min_occ"][g] = np.where(first_step, a_c, np.minimum(rec["min_occ"][g], a_c))
        rec["max_occ"][g] = np.where(first_step, a_c, np.maximum(rec["max_occ"][g], a_c))
        rec["sum_occ"][g] += a_c.astype(np.uint64)
        rec["n_lookahead"][g] += looked[go].astype(np.uint32)
        rec["n_ext"][g] = ne + 1
        stop[go & np.isin(live, g[ne + 1 == max_ext])] = MAX_EXT
        rec["stop"][live[stop != 0]] = stop[stop != 0]
        keep = stop == 0
        live, cur = live[keep], nxt[keep]
    return ext, rec, q.n


def extend_left(buf, offsets, k, thr, max_ext, depth, ask):
    """left=True of the Python facade: the walk of every seed's reverse complement"""
    off = np.asarray(offsets).astype(np.int64)
    rc = [revcomp(np.asarray(buf[off[i]:off[i + 1]], dtype=np.uint8).tobytes()) for i in range(len(off) - 1)]
    return extend(np.frombuffer(b"".join(rc), dtype=np.uint8), offsets_of(rc), k, thr, max_ext, depth, ask)


def offsets_of(seqs) -> np.ndarray:
    o = np.zeros(len(seqs) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return o


def oracle_extend(o, buf, offsets, k: int, thr: int, max_ext: int, depth: int):
    """the rule driven by the CPU oracle alone"""
    import seq_correct_ref as S
    return extend(buf, offsets, k, thr, max_ext, depth, S.oracle_rows(o, k))


def same(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize == 32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def sha_records(rec: np.ndarray) -> str:
    rec = np.ascontiguousarray(rec)
    assert rec.dtype.itemsize == 32
    return hashlib.sha256(rec.tobytes()).hexdigest()


def sha_ext(ext: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(ext, dtype=np.uint8).tobytes()).hexdigest()


def tallies(rec: np.ndarray) -> dict:
    """what the golden file pins beside the digests: seeds per stop code, appended bases, steps that looked ahead"""
    t = {name: int((rec["stop"] == code).sum()) for code, name in STOP_NAMES.items()}
    t["n_ext"] = int(rec["n_ext"].sum())
    t["n_lookahead"] = int(rec["n_lookahead"].sum())
    t["sum_occ"] = int(rec["sum_occ"].sum())
    return t
