"""The mapping rule of kmx_unitig_map_* (include/kmx.h) restated in plain Python: places, windows, segments, records, hits.
Built on the helpers of unitigs_ref.py, independent of the library, with the checks of its consequences and the cases the tests
and tests/golden/make_unitig_map_golden.py share.  Not a test."""
import random

import numpy as np

import unitig_clean_ref as UC
import unitigs_ref as U

SEQ_SEGMENT_DTYPE = np.dtype([("pos", "<u8"), ("n_windows", "<u4"), ("o", "<u4"), ("off", "<u4"), ("reserved", "<u4")])
REC_FIELDS = ("n_windows", "n_mapped", "n_segments", "n_gaps", "first_mapped", "last_mapped", "longest", "reserved")
SEQ_MAP_DTYPE = np.dtype([(f, "<u8") for f in REC_FIELDS])
BASES = set("ACGTacgt")                                        # the counting rule: either case, nothing else


def places(kmers, k: int, strs) -> dict:
    """{canonical k-mer: (u, j, f)} of a unitig set; ValueError when the set is not valid for the listing"""
    listed = set(kmers)
    pl = {}
    for u, s in enumerate(strs):
        if len(s) < k:
            raise ValueError(f"unitig {u} is shorter than k")
        if not set(s) <= set("ACGT"):
            raise ValueError(f"unitig {u} holds a byte outside uppercase ACGT")
        for j in range(len(s) - k + 1):
            y = s[j:j + k]
            c = U.canon(y)
            if c not in listed:
                raise ValueError(f"window {j} of unitig {u} is not listed")
            if c in pl:
                raise ValueError(f"window {j} of unitig {u}: its k-mer has a place already")
            pl[c] = (u, j, 0 if y == c else 1)
    return pl


def window_codes(pl, strs, k: int, read: str):
    """per window of the read: (o, off), or None when it is not mapped"""
    out = []
    for w in range(len(read) - k + 1):
        x = read[w:w + k]
        code = None
        if set(x) <= BASES:
            x = x.upper()
            c = U.canon(x)
            if c in pl:
                u, j, f = pl[c]
                d = f ^ (0 if x == c else 1)
                code = (2 * u + d, j if d == 0 else len(strs[u]) - k - j)   # m_u - 1 - j
        out.append(code)
    return out


def map_reads(kmers, k: int, strs, reads):
    """-> (segments as dicts, seg_offsets, records as dicts, hits per unitig)"""
    pl = places(kmers, k, strs)
    segs, seg_offsets, recs, hits = [], [0], [], [0] * len(strs)
    base = 0
    for read in reads:
        codes = window_codes(pl, strs, k, read)
        nw = len(codes)
        mine = []
        gaps = 0
        for w, c in enumerate(codes):
            if c is None:
                continue
            hits[c[0] >> 1] += 1
            prev = codes[w - 1] if w else None
            if w == 0 or prev is None or prev[0] != c[0] or prev[1] + 1 != c[1]:
                mine.append({"pos": base + w, "n_windows": 0, "o": c[0], "off": c[1], "reserved": 0})
            mine[-1]["n_windows"] += 1
            if w and prev is None:
                gaps += 1
        mapped = [w for w, c in enumerate(codes) if c is not None]
        if mapped and mapped[0] > 0:
            gaps -= 1                                          # the first mapped window is no gap
        recs.append({"n_windows": nw, "n_mapped": len(mapped), "n_segments": len(mine), "n_gaps": gaps,
                     "first_mapped": mapped[0] if mapped else nw, "last_mapped": mapped[-1] if mapped else nw,
                     "longest": max((s["n_windows"] for s in mine), default=0), "reserved": 0})
        segs += mine
        seg_offsets.append(len(segs))
        base += len(read)
    return segs, seg_offsets, recs, hits


def flat(segs, seg_offsets, recs, hits):
    """what the library returns: (SEQ_SEGMENT_DTYPE, uint64 [n + 1], SEQ_MAP_DTYPE, uint64 [U])"""
    s = np.zeros(len(segs), dtype=SEQ_SEGMENT_DTYPE)
    for i, g in enumerate(segs):
        for f, v in g.items():
            s[f][i] = v
    r = np.zeros(len(recs), dtype=SEQ_MAP_DTYPE)
    for i, g in enumerate(recs):
        for f, v in g.items():
            r[f][i] = v
    return s, np.array(seg_offsets, dtype=np.uint64), r, np.array(hits, dtype=np.uint64)


def join(reads):
    """(uint8 bases, uint64 offsets) of a list of str"""
    buf = np.frombuffer("".join(reads).encode("latin-1"), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    return buf, off


def oriented(strs, o: int) -> str:
    return strs[o >> 1] if not o & 1 else U.rc(strs[o >> 1])


def check(k: int, strs, reads, segs, seg_offsets, recs):
    """consequence (a) and what the records promise, asserted on an output (of the restatement or of the library)"""
    text = "".join(reads)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    assert len(seg_offsets) == len(reads) + 1 and seg_offsets[0] == 0 and seg_offsets[-1] == len(segs)
    assert all(a["pos"] < b["pos"] for a, b in zip(segs, segs[1:])), "segments are not in ascending pos"
    for i, (read, r) in enumerate(zip(reads, recs)):
        mine = segs[seg_offsets[i]:seg_offsets[i + 1]]
        assert r["n_windows"] == max(len(read) - k + 1, 0) and r["n_segments"] == len(mine) <= r["n_windows"]
        assert r["n_mapped"] == sum(s["n_windows"] for s in mine) and r["longest"] == max((s["n_windows"] for s in mine), default=0)
        assert r["reserved"] == 0
        if not mine:
            assert r["first_mapped"] == r["last_mapped"] == r["n_windows"] and r["n_gaps"] == 0
            continue
        assert r["first_mapped"] == mine[0]["pos"] - starts[i] and r["last_mapped"] == mine[-1]["pos"] + mine[-1]["n_windows"] - 1 - starts[i]
        assert r["n_gaps"] <= len(mine) - 1
        for s in mine:
            n = s["n_windows"] + k - 1
            assert s["n_windows"] >= 1 and s["reserved"] == 0
            assert starts[i] <= s["pos"] and s["pos"] + n <= starts[i + 1], "a segment leaves its read"
            assert oriented(strs, s["o"])[s["off"]:s["off"] + n] == text[s["pos"]:s["pos"] + n].upper(), "consequence (a)"


def mirrored(k: int, strs, segs, read_len: int):
    """the segment list of the reverse complement of ONE read (at flat position 0), from the read's own"""
    out = []
    for s in reversed(segs):
        m = len(strs[s["o"] >> 1]) - k + 1
        out.append({"pos": read_len - k + 1 - (s["pos"] + s["n_windows"]), "n_windows": s["n_windows"], "o": s["o"] ^ 1,
                    "off": m - s["off"] - s["n_windows"], "reserved": 0})
    return out


# ---- the cases, pinned by seed: name -> (k, k-mers, counts, thr, unitig strings, reads)
def special_reads(strs, k: int, seed: int):
    """reads cut from the unitig strings: both orientations, every short length, N first / middle / last, lowercase, IUPAC,
    a foreign read, an empty one"""
    r = random.Random(seed)
    long_ones = sorted(strs, key=len, reverse=True)[:4]
    s = long_ones[0]
    out = [s, U.rc(s), s.lower(), "", s[:k - 1], s[:k], s[:k + 1], U.rand_seq(3 * k, seed + 1)]
    mid = len(s) // 2
    out += ["N" + s[1:], s[:mid] + "N" + s[mid + 1:], s[:-1] + "N", s[:mid] + "R" + s[mid + 1:], s[:mid] + "n" + s[mid + 1:]]
    for t in long_ones[1:]:
        a = r.randrange(max(len(t) - k, 1))
        out += [t[a:], U.rc(t)[a:].lower()]
    out.append("".join(c.lower() if r.random() < 0.5 else c for c in s))
    return out


def twice_round(cycle_str: str, k: int) -> str:
    """a read that goes twice round the cycle of L nodes that periodic() / circular_seq() spelled in L + k - 1 bytes, and on"""
    L = len(cycle_str) - k + 1
    p = cycle_str[:L]
    return (p * (2 + (k + 2) // L + 1))[:2 * L + k + 2]


def _noisy():
    return U.noisy_reads(U.rand_seq(2000, 70), 400, 100, 0.01, 71)


def _from_unitig_case(name, reads_of):
    k, thr, km, cnt, strs, _ = U.case(name)
    return k, km, cnt, thr, strs, reads_of(strs, k)


def _noisy_case(thr, clean):
    reads = _noisy()
    km, cnt = U.listing_of(U.count_kmers(reads, 21))
    strs = UC.clean(km, cnt, 21, thr)["strs"] if clean else U.unitigs(km, cnt, 21, thr)[0]
    return 21, km, cnt, thr, strs, reads[:60] + special_reads(strs, 21, 72)


def _cycles_case():
    k = 31
    cyc = U.all_cycles(k)
    k, thr, km, cnt, strs, _ = U.case("k31_all_cycles")
    reads = [twice_round(cyc[L], k) for L in (2, 3, 4, 5, 31, 32, 33, 64, 65, 130)]
    return k, km, cnt, thr, strs, reads + [U.rc(x) for x in reads[:4]]


def _cycle_and_tip_case():
    k, thr, km, cnt, strs, _ = U.case("cycle_only_above_thr")
    seqs = U.cycle_and_tip()
    return k, km, cnt, thr, strs, [twice_round(seqs[0], k), U.rc(twice_round(seqs[0], k)), seqs[2]]


def _tangle_reads(kk):
    def f(strs, k):
        seqs = U.tangle(kk, kk)
        return seqs[:6] + [U.rc(s) for s in seqs[2:8]] + seqs[32:36] + special_reads(strs, k, 80 + kk)[:8]
    return f


MAP_CASES = {
    "k5_complete": lambda: _from_unitig_case("k5_complete", lambda strs, k: [U.rand_seq(300, 61), "", U.rand_seq(4, 62), U.rand_seq(5, 63), U.rand_seq(6, 64),
                                                                         U.rand_seq(40, 65).lower(), "ACGTACGTNACGTACGTT", U.rand_seq(17, 66)]),
    "k21_noisy": lambda: _noisy_case(1, False),
    "k21_noisy_clean": lambda: _noisy_case(2, True),
    "k31_tangle": lambda: _from_unitig_case("tangle_k31_thr1", _tangle_reads(31)),
    "k33_tangle": lambda: _from_unitig_case("tangle_k33_thr1", _tangle_reads(33)),
    "k63_tangle": lambda: _from_unitig_case("tangle_k63_thr2", _tangle_reads(63)),
    "k33_cycle400": lambda: _from_unitig_case("k33_cycle400", lambda strs, k: [twice_round(U.circular_seq(400, 33, 34), k), U.rc(twice_round(U.circular_seq(400, 33, 34), k))]),
    "k63_linear": lambda: _from_unitig_case("k63_linear", lambda strs, k: special_reads(strs, k, 90)),
    "k31_all_cycles": _cycles_case,
    "k21_cycle_and_tip": _cycle_and_tip_case,
}


def case(name: str):
    """-> (k, k-mers, counts, thr, unitig strings, reads), the caller's own"""
    return MAP_CASES[name]()
