"""Reference of kmx_polish_seqs in NumPy / Python: the loop of include/kmx.h over a callback that is one kmx_edit_seqs (the CPU
oracle's rule, or the GPU's own seq_edit entry point) and tests/seq_edit_ref.py's apply.  Shared by
tests/golden/make_seq_polish_golden.py, the tests and tools/bench_seq_polish.py; not a test itself."""
import numpy as np

import seq_edit_ref as E

FIELDS = ("n_passes", "converged", "n_sub", "n_del", "n_ins", "out_len", "n_windows", "n_weak", "n_runs", "n_sites", "n_ambiguous", "n_unfixable")
DTYPE = np.dtype([(f, "<u8") for f in FIELDS])
LAST = ("out_len", "n_windows", "n_weak", "n_runs", "n_sites", "n_ambiguous", "n_unfixable")   # of the last pass that examined the read
SUMS = ("n_sub", "n_del", "n_ins")
MAX_PASSES = 16


def _flat(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8), off


def polish(edit_fn, buf, offsets, max_passes: int, retire: bool = True):
    """edit_fn(bases, offsets) -> (edits, kmx_seq_edits records) of one batch.
    retire = True: the definition, per read: a pass runs on the reads the pass before edited.
    retire = False: the host loop on the whole batch, until a pass returns an empty list or max_passes passes ran.
    -> dict: bases, offsets (uint64[n + 1]), records (DTYPE[n]), passes_run, per pass the reads examined for the first time
    since they were edited (`active`), the reads edited, and the reads after the pass (`reads`)."""
    assert 1 <= max_passes <= MAX_PASSES
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    n = len(off) - 1
    cur = [buf[off[i]:off[i + 1]].copy() for i in range(n)]
    rec = np.zeros(n, dtype=DTYPE)
    done = np.zeros(n, dtype=bool)
    passes, history = 0, []
    if n and off[-1] == 0:
        rec["n_passes"], rec["converged"], passes, done[:] = 1, 1, 1, True
    while n and not done.all() and passes < max_passes:
        passes += 1
        act = [i for i in range(n) if not (retire and done[i])]
        abuf, aoff = _flat([cur[i] for i in act])
        edits, r = edit_fn(abuf, aoff)
        out, ooff = E.apply_edits(abuf, aoff, edits)
        fresh, edited = [], []
        for j, i in enumerate(act):
            ed = bool(int(r["n_sub"][j]) + int(r["n_del"][j]) + int(r["n_ins"][j]))
            if done[i]:                                            # (the whole-batch loop asks a converged read again: nothing, and the same record)
                assert not ed and all(int(rec[f][i]) == int(r[f][j]) for f in LAST)
                continue
            fresh.append(i)
            rec["n_passes"][i] = passes
            rec["converged"][i] = not ed
            for f in SUMS:
                rec[f][i] += r[f][j]
            for f in LAST:
                rec[f][i] = r[f][j]
            if ed:
                cur[i] = out[int(ooff[j]):int(ooff[j + 1])].copy()
                assert len(cur[i]) == int(r["out_len"][j])
                edited.append(i)
            else:
                done[i] = True
        assert bool(len(edits)) == bool(edited)
        history.append({"active": fresh, "edited": edited, "reads": [c.tobytes() for c in cur]})
    bases, offs = _flat(cur)
    return {"bases": bases, "offsets": offs, "records": rec, "passes_run": passes, "history": history}


def oracle_fn(o, k: int, thr: int, min_support: int, ops: int = 7, cache=None):
    """the callback over the CPU oracle; cache: a dict that keeps the result per batch (the passes of a smaller max_passes
    are the first passes of a larger one)"""
    def fn(abuf, aoff):
        key = (E.sha(abuf), E.sha(aoff), thr, min_support, ops)
        if cache is not None and key in cache:
            return cache[key]
        res = E.oracle_edit(o, abuf, aoff, k, thr, min_support, ops)[:2]
        if cache is not None:
            cache[key] = res
        return res
    return fn


def wrong(reads, truths) -> int:
    return sum(r != t for r, t in zip(reads, truths))


def tallies(res: dict, truths) -> dict:
    """what the golden file pins beside the digests"""
    t = {f: int(res["records"][f].sum()) for f in FIELDS}
    t["passes_run"] = res["passes_run"]
    t["active_per_pass"] = [len(h["active"]) for h in res["history"]]
    t["edited_per_pass"] = [len(h["edited"]) for h in res["history"]]
    t["reads_wrong_after_pass"] = [wrong(h["reads"], truths) for h in res["history"]]
    return t
