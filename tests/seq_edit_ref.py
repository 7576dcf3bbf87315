"""Reference of kmx_edit_seqs / kmx_apply_edits in NumPy / Python: the rule of include/kmx.h over the per-base answers of
kmx_query_seqs (or of the CPU oracle) and a callback that answers rows of k bytes, like tests/seq_correct_ref.py.  Shared by
tests/golden/make_seq_edit_golden.py, the tests and tools/bench_seq_edit.py; not a test itself."""
import hashlib

import numpy as np

import seq_correct_ref as S

FIELDS = ("n_windows", "n_weak", "n_runs", "n_sites", "n_sub", "n_del", "n_ins", "n_ambiguous", "n_unfixable", "out_len")
DTYPE = np.dtype([(f, "<u8") for f in FIELDS])
ACGT = b"ACGT"
OPS_SUB, OPS_DEL, OPS_INS = 1, 2, 4
SUB, DEL, INS = 1, 2, 3


def edit(pos: int, op: int, code: int) -> int:
    return pos << 8 | op << 4 | code


def _sub(p, v0, v1, x):
    return [(SUB, p, ci, v0, v1) for ci, c in enumerate(ACGT) if x[p] != c]


def _del(p, L, k):
    return [(DEL, p, 0, max(0, p - k + 1), min(p - 1, L - 1 - k))]


def _ins(j, L, k, codes=range(4)):
    return [(INS, j, ci, max(0, j - k + 1), min(j, L + 1 - k)) for ci in codes]


def sites_of_run(s: int, e: int, x: np.ndarray, k: int, ops: int):
    """the shape table: the sites of the run [s, e] of the sequence x, each a list of candidates (op, position, code, v0, v1)
    in the order of the rule; positions and windows inside the sequence"""
    L = len(x)
    nw = L - k + 1
    ln = e - s + 1
    has_l, has_r = s > 0, e < nw - 1
    keep = lambda cands: [c for c in cands if ops & (1 << (c[0] - 1))]
    if not has_l and not has_r:
        return []
    if has_r and not has_l:
        return [keep(_sub(e, max(s, e - k + 1), e, x) + _del(e, L, k) + _ins(e + 1, L, k))]
    if has_l and not has_r:
        a = s + k - 1
        return [keep(_sub(a, s, min(e, a), x) + _del(a, L, k) + _ins(a, L, k))]
    if ln > k:
        return [keep(_sub(s + k - 1, s, min(s + k - 1, e - k), x)), keep(_sub(e, max(e - k + 1, s + k), e, x))]
    h = k - ln + 1
    core = x[e:s + k]
    assert len(core) == h
    cands = _sub(e, s, e, x) if ln == k else []
    if (core == core[0]).all():
        cands += _del(e, L, k)
    if h == 2:
        cands += _ins(e + 1, L, k)
    elif h >= 3:
        c = int(x[e + 1])
        if c in ACGT and (x[e + 1:s + k - 1] == c).all():
            cands += _ins(e + 1, L, k, [ACGT.index(c)])
    return [keep(cands)]


def window(x: np.ndarray, op: int, p: int, c: int, q: int, k: int) -> np.ndarray:
    """the k bytes at q of x edited by (op, p, c)"""
    if op == SUB:
        r = x[q:q + k].copy()
        r[p - q] = c
        return r
    if op == DEL:
        return np.concatenate([x[q:p], x[p + 1:q + k + 1]])
    return np.concatenate([x[q:p], np.array([c], dtype=np.uint8), x[p:q + k - 1]])


def edit_seqs(per_base, buf, offsets, k: int, thr: int, min_support: int, ops: int, query_rows):
    """-> (edits uint64[] ascending, records DTYPE[n_seqs], verification windows asked).  Every candidate of every site is
    asked in full (no early stop): the verdict of a candidate is a conjunction, so the result is the same."""
    assert 1 <= min_support <= 64 and 1 <= ops <= 7
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    n_bases = int(off[-1])
    base, _ = S.plan(per_base, offsets, k, thr, 1)
    rec = np.zeros(len(off) - 1, dtype=DTYPE)
    for f in ("n_windows", "n_weak", "n_runs"):
        rec[f] = base[f]
    rec["out_len"] = np.diff(off)
    per_base = np.asarray(per_base, dtype=np.int32)
    sites, rows, owner = [], [], []                                # sites: (sequence, start, [tried candidates])
    for i in range(len(off) - 1):
        a, z = int(off[i]), int(off[i + 1])
        nw = max(z - a - k + 1, 0)
        if nw == 0 or not rec["n_weak"][i]:
            continue
        x = buf[a:z]
        for s, e in S.runs_of(S.close_gaps(per_base[a:a + nw] < thr)):
            for cands in sites_of_run(s, e, x, k, ops):
                tried = [c for c in cands if c[4] - c[3] + 1 >= min_support]
                if not tried:
                    continue
                for ci, (op, p, code, v0, v1) in enumerate(tried):
                    assert 0 <= v0 and v1 + k <= len(x) + (op == INS) - (op == DEL)
                    for q in range(v0, v1 + 1):
                        r = window(x, op, p, ACGT[code], q, k)
                        assert len(r) == k
                        rows.append(r)
                        owner.append((len(sites), ci))
                sites.append((i, a, tried))
    ans = np.asarray(query_rows(np.stack(rows)), dtype=np.int32) if rows else np.zeros(0, np.int32)
    ok = [[True] * len(t) for _, _, t in sites]
    for (j, ci), good in zip(owner, (ans >= thr).tolist()):
        ok[j][ci] = ok[j][ci] and good
    edits = []
    for j, (i, a, tried) in enumerate(sites):
        rec["n_sites"][i] += 1
        won = [c for c, g in zip(tried, ok[j]) if g]
        if len(won) == 1:
            op, p, code = won[0][:3]
            edits.append(edit(a + p, op, code))
            rec[("n_sub", "n_del", "n_ins")[op - 1]][i] += 1
            if op != SUB:
                rec["out_len"][i] = int(rec["out_len"][i]) + (1 if op == INS else -1)
        elif won:
            rec["n_ambiguous"][i] += 1
        else:
            rec["n_unfixable"][i] += 1
    edits = np.array(sorted(edits), dtype=np.uint64)
    assert len(np.unique(edits >> np.uint64(4))) == len(edits), "(pos, op) is unique"
    assert len(edits) <= n_bases // 3 + 1, "the capacity bound of include/kmx.h"
    return edits, rec, len(rows)


def apply_edits(buf, offsets, edits):
    """-> (bases uint8[], offsets_out uint64[n_seqs + 1]): the definition of kmx_apply_edits; ValueError on a bad list"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    n = int(off[-1])
    e = np.asarray(edits, dtype=np.uint64)
    pos, op, code = (e >> np.uint64(8)).astype(np.int64), ((e >> np.uint64(4)) & np.uint64(15)).astype(np.int64), (e & np.uint64(15)).astype(np.int64)
    if len(e) and ((np.diff(e.astype(object)) <= 0).any() or (pos >= n).any() or ((op < 1) | (op > 3)).any() or (code > 3).any() or (code[op == DEL] != 0).any()):
        raise ValueError("bad edit list")
    if len(e) > 1 and ((pos[1:] == pos[:-1]) & (op[1:] != INS)).any():
        raise ValueError("SUB and DEL at one position")
    acgt = np.frombuffer(ACGT, dtype=np.uint8)
    x = buf[:n].copy()
    x[pos[op == SUB]] = acgt[code[op == SUB]]
    count = np.ones(n, dtype=np.int64)                             # bytes each input position emits
    count[pos[op == DEL]] = 0
    count[pos[op == INS]] += 1
    start = np.concatenate([[0], np.cumsum(count)])
    out = np.zeros(int(start[-1]), dtype=np.uint8)
    live = count > 0
    out[start[1:][live] - 1] = x[live]                             # the input byte (or its SUB base) is the last one emitted
    out[start[:-1][pos[op == INS]]] = acgt[code[op == INS]]
    return out, start[off].astype(np.uint64)


def oracle_edit(o, buf, offsets, k: int, thr: int, min_support: int, ops: int = 7):
    """the rule driven by the CPU oracle alone"""
    import seq_reads as R
    return edit_seqs(R.oracle_per_base(o, buf, offsets, k), buf, offsets, k, thr, min_support, ops, S.oracle_rows(o, k))


def same(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and a.tobytes() == b.tobytes()


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tallies(rec: np.ndarray, edits: np.ndarray) -> dict:
    t = {f: int(rec[f].sum()) for f in FIELDS}
    t["n_edits"] = int(len(edits))
    return t
