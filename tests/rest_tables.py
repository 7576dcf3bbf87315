"""Rest tables written by hand: the file format, a plain restatement of the lookup, and one crafted table per shape.

Not a test itself and free of compiled code: k-mers are Python ints of 2k bits (A=0 C=1 G=2 T=3, first base in the most
significant position -- the packed layout of kmcex_amd/synth.py), tables are dicts of plain arrays.

`lookup` is KRestData::check_kmer as oracle/kmx_oracle.c and DESIGN.md state it: the prefix selects a group through
hash2index, a binary search runs over the rows [pre_buffer[g], pre_buffer[g + 1]] with the upper bound INCLUDED -- so the first
row of the next group can answer a k-mer that is greater than every row of its own group -- and a row index at or past
`entries` never matches (divergence D3).  It is not derived from the device code.

`crafted(k, pre_len)` lays out a table that makes those rules matter (see its docstring); `info(k, pre_len)` names the parts
the tests state conditions on.
"""
from __future__ import annotations

import functools
import random
import struct

import numpy as np

# (k, pre_len) the loader accepts: suffix bits 0, 8, 16, 40, 48, 56, 64 (exactly one word), 96, 112, 120; prefixes of 1 to 11 bases
SHAPES = [(31, 7), (31, 3), (31, 11), (32, 4), (33, 5), (36, 4), (39, 7), (55, 7), (63, 7), (64, 4), (12, 4), (8, 4), (7, 7), (6, 6), (5, 1)]

_BASES = "ACGT"
_CODE = {"C": 1, "G": 2, "T": 3}                      # every other byte is 0, as in the reference's 2-bit conversion


# ---------------------------------------------------------------------------------------------- k-mers as ints and strings
def to_str(v: int, k: int) -> str:
    return "".join(_BASES[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def from_str(s: str) -> int:
    v = 0
    for c in s:
        v = (v << 2) | _CODE.get(c, 0)
    return v


def revcomp(v: int, k: int) -> int:
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def canonical_u64(v: int, k: int) -> int:
    """The k-mer the reference looks up for `v`: its canonical form computed through ONE 64-bit word (min_kmer of
    oracle/kmx_oracle.c).  Exact for k <= 32; above, only the last 32 bases are compared and a reverse complement that wins
    keeps its last 32 bases alone.  tests/test_rest_lookup_cpu.py holds this against the oracle's own min_kmer."""
    m64 = (1 << 64) - 1
    u = v & m64
    r, w = 0, u
    for _ in range(k):
        r = ((r << 2) | ((~w) & 3)) & m64
        w >>= 2
    return v if u <= r else r & ((1 << (2 * k)) - 1)


def pack(vals, k: int) -> np.ndarray:
    """ints -> the packed uint64 layout the query calls take ([n] for k <= 32, [n, 2] above)"""
    m64 = (1 << 64) - 1
    if k <= 32:
        return np.array([v for v in vals], dtype=np.uint64)
    return np.array([[v >> 64, v & m64] for v in vals], dtype=np.uint64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------- rest.bin
def write_rest_bin(path, k: int, pre_len: int, rows, counts) -> None:
    """rest.bin as kmx_save writes it: int32 k, pre_len, map_size, pre_buffer_size; uint64 suff_bin_size, entries;
    hash2index[map_size]; pre_buffer[]; the suffix rows ((k - pre_len) / 4 bytes each, most significant first); int32 counts.
    `rows` are ints of 2k bits in ascending order (equal neighbours allowed)."""
    assert (k - pre_len) % 4 == 0 and len(rows) == len(counts)
    assert all(a <= b for a, b in zip(rows, rows[1:])), "rows must ascend"
    sbits, sg, map_size = 2 * (k - pre_len), (k - pre_len) // 4, 1 << (2 * pre_len)
    h2i = np.full(map_size, -1, dtype=np.int32)
    pre_buffer, suffix = [0], bytearray()
    prev = -1
    for e, v in enumerate(rows):
        p = v >> sbits
        if p != prev:
            h2i[p] = len(pre_buffer) - 1
            pre_buffer.append(e)
            prev = p
        pre_buffer[-1] = e + 1
        suffix += (v & ((1 << sbits) - 1)).to_bytes(sg, "big")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i2Q", k, pre_len, map_size, len(pre_buffer), len(suffix), len(rows)))
        f.write(h2i.astype("<i4").tobytes())
        f.write(np.array(pre_buffer, dtype="<i4").tobytes())
        f.write(bytes(suffix))
        f.write(np.array(counts, dtype="<i4").tobytes())


def read_rest_bin(path) -> dict:
    """the arrays of a rest.bin, plus `rows`: every row as the 2k-bit int of its prefix and suffix"""
    with open(path, "rb") as f:
        raw = f.read()
    k, pre_len, map_size, pbs, sbs, entries = struct.unpack_from("<4i2Q", raw, 0)
    off = 32
    h2i = np.frombuffer(raw, dtype="<i4", count=map_size, offset=off); off += 4 * map_size
    pre = np.frombuffer(raw, dtype="<i4", count=pbs, offset=off); off += 4 * pbs
    suffix = raw[off:off + sbs]; off += sbs
    counts = np.frombuffer(raw, dtype="<i4", count=entries, offset=off); off += 4 * entries
    assert off == len(raw), "rest.bin is longer or shorter than its header says"
    sg, sbits = (k - pre_len) // 4, 2 * (k - pre_len)
    rows = [0] * entries
    for p in np.nonzero(h2i >= 0)[0].tolist():
        g = int(h2i[p])
        for e in range(int(pre[g]), int(pre[g + 1])):
            rows[e] = (p << sbits) | int.from_bytes(suffix[e * sg:(e + 1) * sg], "big")
    return {"k": k, "pre_len": pre_len, "map_size": map_size, "entries": entries, "suff_group": sg, "hash2index": h2i,
            "pre_buffer": pre, "suffix": suffix, "counts": counts, "rows": rows}


def lookup(table: dict, kmer: int) -> int:
    """check_kmer, literally.  0 = not in the table."""
    k, pre_len, sg = table["k"], table["pre_len"], table["suff_group"]
    sbits = 2 * (k - pre_len)
    key = (kmer & ((1 << sbits) - 1)).to_bytes(sg, "big")
    g = int(table["hash2index"][kmer >> sbits])
    if g < 0:
        return 0
    low, high = int(table["pre_buffer"][g]), int(table["pre_buffer"][g + 1])     # `high` is one row past the group: included
    suffix = table["suffix"]
    while low <= high:
        mid = (low + high) // 2
        if mid >= table["entries"]:                         # D3: the row past the table never matches
            return 0
        row = suffix[mid * sg:(mid + 1) * sg]
        if key < row:                                       # bytes compare like memcmp
            high = mid - 1
        elif key > row:
            low = mid + 1
        else:
            return int(table["counts"][mid])
    return 0


# ---------------------------------------------------------------------------------------------- crafted tables
def _reachable_fix(v: int, k: int, pre_len: int) -> int:
    """Nudge a row so that a query can reach it, i.e. so that it is the canonical form the reference computes: k <= 32 -- the
    last base low enough against the first (first base A: last base not T); k > 32 -- of the last 32 bases the first an A and
    the base their reverse complement starts with not a T.  The prefix stays as it is wherever the suffix has a base."""
    if k <= 32:
        f, l = v >> (2 * (k - 1)), v & 3
        return v if f == 3 else (v & ~3) | min(l, 2 - f)
    sh = 2 * (k - 32)                                       # base 31 of the string: what the reverse complement of the last 32 starts with
    if k - 32 > pre_len:
        v &= ~(3 << 62)                                     # base k - 32: the first of the last 32 bases
    if (v >> sh) & 3 == 3 and sh != 62:
        v &= ~(1 << sh)                                     # T -> G
    return v


def _d3_suffix(k: int, pre_len: int):
    """The suffix of a key in the last prefix group (prefix T...T) that is its own canonical form and large, or None."""
    p, sb = pre_len, k - pre_len
    if k <= 32:
        a = (k - 2 * p) // 2                                # T^(p+a) A^b is canonical iff p + a <= b
        return from_str("T" * a + "A" * (sb - a)) if a >= 1 else None
    s, i0 = ["T"] * k, k - 32
    if i0 >= p:
        s[i0] = "G" if i0 == p else "A"
        s[31] = "A"
    else:                                                   # the last 32 bases start inside the prefix: their T's need A's opposite
        n = p - i0
        for j in range(n + 1):
            s[31 - j] = "A"
        s[p] = "G"
    return from_str("".join(s[p:]))


@functools.lru_cache(maxsize=None)
def info(k: int, pre_len: int) -> dict:
    """The crafted table of a shape and its parts: rows, counts, queries (ints), and
    run -- the rows that differ only in their last 6 bases; d3 -- keys above every row of the last group (a reachable one first,
    if the shape has one); next_first -- (query, count of the next group's first row, that row is greater than every row of the
    query's own group) for every existing prefix but the last; dup -- index of the second row of the duplicate pair;
    single -- a prefix whose group holds one row; prefixes -- the existing ones."""
    assert (k - pre_len) % 4 == 0 and 1 <= pre_len <= 12
    sbits, M = 2 * (k - pre_len), 1 << (2 * pre_len)
    S = 1 << sbits
    full = (1 << (2 * k)) - 1
    fix = lambda v: _reachable_fix(v, k, pre_len)
    if M > 4:
        prefixes = sorted({p for p in (0, 1, 3, 4, 9, 14, M // 4 + 4, M - 1) if p < M})
    else:
        prefixes = [0, 1, 2, 3]                             # pre_len 1: room for two small / large pairs, not for an empty prefix
    rows, run = set(), []
    if sbits == 0:                                          # the k-mer is all prefix: one row per group
        rows = {fix(p) for p in prefixes} | {M - 1}
        run = sorted({fix(256 + 3 * j) for j in range(60)})
        rows |= set(run)
        run_gi = single_gi = None
    else:
        # above 32 bases a reachable row has an A where its last 32 bases start: if that is the top of the suffix, "large" ends there
        top = S // 4 if (k > 32 and k - 32 == pre_len) else S
        d3s = _d3_suffix(k, pre_len)
        run_gi, single_gi = (4 if len(prefixes) > 4 else 0), 2
        for gi, p in enumerate(prefixes):
            hi_end = (d3s if d3s is not None else top) if gi == len(prefixes) - 1 else top
            if gi == len(prefixes) - 1 and k <= 32:
                # canonical rows behind a prefix of T's: T^p Y A^(p+1) with Y starting below T (T^p A^p where that is all of k)
                n = k - 2 * pre_len - 1
                ymax = from_str("G" + "T" * (n - 1)) if n >= 1 else 0
                sufs = [y << (2 * (pre_len + 1)) for y in ([0, 1, 2] if n == 1 else [ymax - 2, ymax - 1, ymax])] if n >= 1 else [0]
            elif gi == single_gi:
                sufs = [4 * gi + 1]
            elif gi % 2:                                    # near the top: the first row beats every row of the group before
                step = 64 if sbits >= 16 else 4
                sufs = [hi_end - 40 - gi * step, hi_end - 20 - gi * step, hi_end - 8 - gi * step]
            elif sbits >= 16:
                sufs = [4 + gi * 16 + 1, (1 << (sbits // 2)) | (gi * 4 + 2), (1 << (sbits - 6)) + gi * 4 + 1]
            else:
                sufs = [4 * gi + 1, 4 * gi + 33]
            group = {fix((p << sbits) | s) for s in sufs}
            if gi == run_gi:                                # >= 40 rows in one bucket of the top-bits index, among other rows
                if sbits >= 16:
                    base = 1 << (sbits - 4)
                    run = sorted({fix((p << sbits) | (base + j)) for j in range(0, 4096, 41)})
                    group.add(fix((p << sbits) | (base + 4096 + 5)))
                else:
                    run = sorted({fix((p << sbits) | j) for j in range(64, 180)})
                group |= set(run)
            assert all(v >> sbits == p for v in group)
            rows |= group
    rows = sorted(rows)
    assert len(run) >= 40 and len({v >> 12 for v in run}) == 1
    counts = [1 + (37 * i + 11) % 1000 for i in range(len(rows))]
    # the stale-slot duplicate: one row twice, side by side, with one count -- in a group that holds other rows
    dup = next(i for i in range(1, len(rows)) if sbits == 0 or (rows[i] >> sbits == rows[i - 1] >> sbits and rows[i] not in run))
    rows.insert(dup, rows[dup])
    counts.insert(dup, counts[dup])
    dup += 1

    groups = {}
    for i, v in enumerate(rows):
        groups.setdefault(v >> sbits, []).append(i)
    existing = sorted(groups)
    d3, next_first = [], []
    if sbits:
        last_p = existing[-1]
        top_row = rows[groups[last_p][-1]] & (S - 1)
        d3s = _d3_suffix(k, pre_len)
        d3 = [(last_p << sbits) | s for s in ([d3s] if d3s is not None else []) + [top_row + 1, S - 1] if s > top_row]
    for a, b in zip(existing, existing[1:]):
        s = rows[groups[b][0]] & (S - 1)
        next_first.append(((a << sbits) | s, counts[groups[b][0]], s > (rows[groups[a][-1]] & (S - 1))))

    q = list(rows) + [revcomp(v, k) for v in rows]
    for v in rows:                                          # one base step down and up, inside the prefix group
        lo, hi = (v >> sbits) << sbits, (((v >> sbits) + 1) << sbits) - 1
        q += [u for u in (v - 1, v + 1) if (lo <= u <= hi if sbits else 0 <= u <= full)]
    for p in existing:
        i = existing.index(p)
        own = [rows[groups[p][0]] & (S - 1), rows[groups[p][-1]] & (S - 1)]
        nxt = [rows[groups[existing[i + 1]][0]] & (S - 1)] if i + 1 < len(existing) else []
        for pp in (p - 1, p, p + 1):                        # the prefix and the empty prefixes beside it
            if 0 <= pp < M and (pp == p or pp not in groups):
                q += [(pp << sbits) | s for s in [0, S - 1] + own + nxt]
    q += [v for v, _, _ in next_first] + d3
    rng = random.Random(0x5EED0000 + 100 * k + pre_len)
    q += [rng.getrandbits(2 * k) for _ in range(2000)]
    return {"k": k, "pre_len": pre_len, "rows": rows, "counts": counts, "queries": q, "run": run, "d3": d3,
            "next_first": next_first, "dup": dup, "prefixes": existing,
            "single": next((p for p in existing if len(groups[p]) == 1), None)}


def crafted(k: int, pre_len: int):
    """(rows, counts, queries) of a deterministic table for one loader-accepted shape; queries are packed.

    The table: 8 prefix groups (4 at pre_len 1) with empty prefixes between them, at prefix 0 and at prefix map_size - 1; a
    group of one row; groups that alternate between small suffixes and suffixes near the top of the range, so that the first
    row of every second group is greater than all rows of the group before it (the inclusive bound then answers); in one group,
    beside other rows, at least 40 rows that differ only in their last 6 bases; one row twice with one count.  Rows are nudged
    to be canonical (`_reachable_fix`); behind the prefix T...T they are T^p Y A^(p+1) with Y below T, canonical as well, up to
    k = 32 (above, the oracle decides which rows a query reaches).  Where the suffix has no bases (k == pre_len) every group
    is one row, the alternation has nothing to vary and T...T is a row no query reaches; where it has 4 (sbits 8) the 40 rows
    fill most of their group; pre_len 1 has four prefixes, all taken.

    The queries: every row, its reverse complement, its neighbours one base step below and above; per existing prefix and the
    empty prefixes beside it the suffixes 0, all-ones, the group's first and last and the next group's first; keys above the
    last group's rows (D3); 2000 seeded random k-mers."""
    t = info(k, pre_len)
    return list(t["rows"]), list(t["counts"]), pack(t["queries"], k)


# ---------------------------------------------------------------------------------------------- numpy side: large tables
def genome_stream2(n_bases: int, k: int, ci: int, cs: int, seed: int = 11, seed_c: int = 2):
    """synth.genome_stream for 32 < k <= 64: the overlapping windows of synth.genome_bases packed into two words"""
    from kmcex_amd import synth
    assert 32 < k <= 64
    bases = synth.genome_bases(n_bases, seed)
    n = n_bases - k + 1
    v = np.zeros((n, 2), dtype=np.uint64)
    for j in range(k - 32):
        v[:, 0] = (v[:, 0] << np.uint64(2)) | bases[j:j + n]
    for j in range(k - 32, k):
        v[:, 1] = (v[:, 1] << np.uint64(2)) | bases[j:j + n]
    km = synth.sort_unique(synth.canonical(v, k))
    return km, synth.d1_counts(len(km), ci, cs, seed_c)


def neighbours_np(km: np.ndarray, k: int) -> np.ndarray:
    """the 4 successors and 4 predecessors of every packed k-mer: [8, n] (k <= 32) or [8, n, 2]"""
    two = np.uint64(2)
    if k <= 32:
        mask = np.uint64((1 << (2 * k)) - 1)
        return np.stack([((km << two) | np.uint64(x)) & mask for x in range(4)] +
                        [(km >> two) | (np.uint64(x) << np.uint64(2 * (k - 1))) for x in range(4)])
    hi, lo = km[:, 0], km[:, 1]
    hmask = np.uint64((1 << (2 * k - 64)) - 1)
    out = []
    for x in range(4):
        out.append(np.stack([((hi << two) | (lo >> np.uint64(62))) & hmask, (lo << two) | np.uint64(x)], axis=1))
    for x in range(4):
        out.append(np.stack([(hi >> two) | (np.uint64(x) << np.uint64(2 * k - 66)), (lo >> two) | ((hi & np.uint64(3)) << np.uint64(62))], axis=1))
    return np.stack(out)


def canonical_u64_np(km: np.ndarray, k: int) -> np.ndarray:
    """canonical_u64 over packed k-mers"""
    from kmcex_amd import synth
    if k <= 32:
        return synth.canonical(km, k)
    a = km.reshape(-1, 2)
    u, w, r = a[:, 1], a[:, 1].copy(), np.zeros(len(a), dtype=np.uint64)
    for _ in range(k):
        r = (r << np.uint64(2)) | ((~w) & np.uint64(3))
        w = w >> np.uint64(2)
    out = a.copy()
    take = u > r
    out[take, 0] = 0
    out[take, 1] = r[take]
    return out.reshape(km.shape)


def member_np(km: np.ndarray, rows: np.ndarray, k: int) -> np.ndarray:
    """which packed k-mers are among `rows` (packed alike)"""
    if k <= 32:
        return np.isin(km, rows)
    key = lambda a: np.ascontiguousarray(a.reshape(-1, 2)).view(np.dtype((np.void, 16))).reshape(-1)
    return np.isin(key(km), key(rows))


MODEL = (1, 1023, 7, 5)                                # ci, cs, nh, nb of the models the crafted tables are put into
_dirs = {}


def model_dirs(base, k: int, pre_len: int, rows=None, counts=None, tag: str = "crafted"):
    """(directory with the given table -- the crafted one by default --, directory with an empty table): header and km.bin of
    a 2 000-k-mer build of the CPU oracle, rest.bin replaced.  Written once per `base`, shape and tag."""
    import os
    import shutil

    import oracle_lib as O
    from kmcex_amd import synth
    key = (str(base), k, pre_len, tag)
    if key not in _dirs:
        ci, cs, nh, nb = MODEL
        d0 = os.path.join(str(base), f"k{k}_p{pre_len}_empty")
        if not os.path.isdir(d0):
            km, cnt = synth.make_stream(2000, k, ci, cs, seed_k=500 + k, seed_c=pre_len)
            o = O.OracleModel(ci, cs, nh, nb)
            o.build(k, km, cnt)
            o.save(d0)
            o.close()
            write_rest_bin(os.path.join(d0, "rest.bin"), k, pre_len, [], [])
        d1 = os.path.join(str(base), f"k{k}_p{pre_len}_{tag}")
        os.makedirs(d1)
        for f in ("header", "km.bin"):
            shutil.copy(os.path.join(d0, f), os.path.join(d1, f))
        if rows is None:
            rows, counts = info(k, pre_len)["rows"], info(k, pre_len)["counts"]
        write_rest_bin(os.path.join(d1, "rest.bin"), k, pre_len, rows, counts)
        _dirs[key] = (d1, d0)
    return _dirs[key]


def dirty_variants(s: str, limit: int = 4):
    """`s` with one of its A's replaced by N, n, X or - : the reference's 2-bit conversion reads each as an A"""
    pos = [i for i, c in enumerate(s) if c == "A"]
    out = []
    for j, c in enumerate("NnX-"[:limit]):
        if pos:
            i = pos[(j * 7 + len(s)) % len(pos)]
            out.append(s[:i] + c + s[i + 1:])
    return out
