"""The rule of kmx_unitig_walk_segs (include/kmx.h) restated in plain Python on top of unitig_map_ref and unitig_links_ref: the
joins between consecutive segments of a read, the walks, their steps, the reads per link and the counters.  With flat(), the
check of the rule's consequences, spell(), the mirror image of a result, the GAF text the facade must write, and the cases the
tests share.  Not a test."""
import functools
import random

import numpy as np

import unitig_clean_ref as UC
import unitig_links_ref as L
import unitig_map_ref as R
import unitigs_ref as U

WALK_FIELDS = (("pos", "<u8"), ("n_span", "<u8"), ("n_mapped", "<u8"), ("n_covered", "<u8"), ("first_seg", "<u8"), ("first_step", "<u8"),
               ("n_segs", "<u4"), ("n_steps", "<u4"), ("off_first", "<u4"), ("off_last", "<u4"), ("n_inside", "<u4"), ("n_across", "<u4"),
               ("indel", "<i4"), ("reserved", "<u4"))
WALK_DTYPE = np.dtype(list(WALK_FIELDS))
STAT_FIELDS = ("n_walks", "n_steps", "n_edge", "n_inside", "n_across", "n_unlinked", "n_breaks", "reserved")
PARTS = ("walks", "walk_offsets", "steps", "link_hits", "stats")


def join(k, mu, rows, loff, A, B, max_gap, max_indel):
    """the join A -> B of two consecutive segments of one read: (kind, d, link index) or (None, counter name, None)"""
    mA = mu[A["o"] >> 1]
    endA = A["off"] + A["n_windows"] - 1
    g = B["pos"] - A["pos"] - A["n_windows"]
    row = rows[A["o"]]
    e = loff[A["o"]] + row.index(B["o"]) if B["o"] in row else None
    if g == 0:
        if endA == mA - 1 and B["off"] == 0 and e is not None:
            return "edge", 0, e
        return None, "n_unlinked", None
    if 1 <= g <= max_gap:
        d = (B["off"] - endA - 1) - g
        if B["o"] == A["o"] and B["off"] > endA and abs(d) <= max_indel:
            return "inside", d, None
        d = (mA - 1 - endA) + B["off"] - g
        if e is not None and abs(d) <= max_indel:
            return "across", d, e
    return None, "n_breaks", None


def walk_segs(k, strs, segs, seg_offsets, rows, max_gap, max_indel):
    """-> (walks as dicts, walk_offsets, steps, link_hits, stats as a dict)"""
    mu = [len(s) - k + 1 for s in strs]
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    walks, walk_offsets, steps, hits = [], [], [], [0] * loff[-1]
    st = dict.fromkeys(STAT_FIELDS, 0)
    for r in range(len(seg_offsets) - 1):
        walk_offsets.append(len(walks))
        lo, hi = int(seg_offsets[r]), int(seg_offsets[r + 1])
        for i in range(lo, hi):
            B = segs[i]
            kind, d, e = (None, None, None) if i == lo else join(k, mu, rows, loff, segs[i - 1], B, max_gap, max_indel)
            if kind is None:
                if d is not None:
                    st[d] += 1
                walks.append({"pos": B["pos"], "n_span": 0, "n_mapped": 0, "n_covered": 0, "first_seg": i, "first_step": len(steps), "n_segs": 0, "n_steps": 1,
                              "off_first": B["off"], "off_last": 0, "n_inside": 0, "n_across": 0, "indel": 0, "reserved": 0})
                steps.append(B["o"])
            else:
                g = B["pos"] - segs[i - 1]["pos"] - segs[i - 1]["n_windows"]
                w = walks[-1]
                w["n_covered"] -= max(0, k - 1 - g)
                w["indel"] += d
                st["n_" + kind] += 1
                if kind != "inside":
                    hits[e] += 1
                    steps.append(B["o"])
                    w["n_steps"] += 1
                if kind != "edge":
                    w["n_" + kind] += 1
            w = walks[-1]
            w["n_segs"] += 1
            w["n_mapped"] += B["n_windows"]
            w["n_covered"] += B["n_windows"] + k - 1
            w["n_span"] = B["pos"] + B["n_windows"] - w["pos"]
            w["off_last"] = B["off"] + B["n_windows"] - 1
    walk_offsets.append(len(walks))
    st["n_walks"], st["n_steps"] = len(walks), len(steps)
    return walks, walk_offsets, steps, hits, st


def flat(walks, walk_offsets, steps, hits, st):
    """what the library returns: (WALK_DTYPE, uint64 [n_seqs + 1], uint32 steps, uint64 [n_links], uint64 [8] stats)"""
    w = np.zeros(len(walks), dtype=WALK_DTYPE)
    for i, g in enumerate(walks):
        for f, v in g.items():
            w[f][i] = v
    return (w, np.array(walk_offsets, dtype=np.uint64), np.array(steps, dtype=np.uint32), np.array(hits, dtype=np.uint64),
            np.array([st[f] for f in STAT_FIELDS], dtype=np.uint64))


def spell(strs, steps, k):
    """the steps' oriented strings, concatenated with k - 1 bytes of overlap"""
    out = R.oriented(strs, steps[0])
    for o in steps[1:]:
        out += R.oriented(strs, o)[k - 1:]
    return out


def path_of(k, strs, w, steps):
    """(path as text, path length, path start, path end) of a walk, the GAF columns"""
    mine = steps[w["first_step"]:w["first_step"] + w["n_steps"]]
    ms = [len(strs[o >> 1]) - k + 1 for o in mine]
    return "".join(f"{'<' if o & 1 else '>'}u{o >> 1}" for o in mine), sum(ms) + k - 1, w["off_first"], sum(ms[:-1]) + w["off_last"] + k


def gaf(k, strs, reads, walks, walk_offsets, steps, first_read=0):
    """the GAF text of KModel::write_walks_gaf: one line per walk"""
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    out = []
    for r, read in enumerate(reads):
        for w in walks[walk_offsets[r]:walk_offsets[r + 1]]:
            q0 = w["pos"] - int(starts[r])
            q1 = q0 + w["n_span"] + k - 1
            path, plen, p0, p1 = path_of(k, strs, w, steps)
            out.append(f"{first_read + r}\t{len(read)}\t{q0}\t{q1}\t+\t{path}\t{plen}\t{p0}\t{p1}\t{w['n_covered']}\t{max(q1 - q0, p1 - p0)}\t255\t"
                       f"id:i:{w['indel']}\tbg:i:{w['n_inside'] + w['n_across']}\n")
    return "".join(out)


def check(k, strs, reads, segs, seg_offsets, walks, walk_offsets, steps, st):
    """the consequences of the rule and what a walk's record promises, asserted on an output (of the restatement or the library)"""
    text = "".join(reads)
    assert st["n_unlinked"] == 0, "consequence (a): two neighbouring mapped windows are joined by an edge of the graph"
    assert len(walk_offsets) == len(reads) + 1 and walk_offsets[0] == 0 and walk_offsets[-1] == len(walks) == st["n_walks"]
    assert st["n_steps"] == len(steps) == sum(w["n_steps"] for w in walks)
    assert st["n_edge"] + st["n_inside"] + st["n_across"] + st["n_breaks"] + st["n_unlinked"] + sum(1 for a, b in zip(seg_offsets, seg_offsets[1:]) if b > a) == len(segs)
    nxt_seg = nxt_step = 0
    for r in range(len(reads)):
        mine = walks[walk_offsets[r]:walk_offsets[r + 1]]
        assert nxt_seg == seg_offsets[r], "walks do not partition the segments of a read in order"
        for w in mine:
            assert w["first_seg"] == nxt_seg and w["first_step"] == nxt_step and w["n_segs"] >= 1 and w["n_steps"] >= 1 and w["reserved"] == 0
            nxt_seg += w["n_segs"]
            nxt_step += w["n_steps"]
            ss = segs[w["first_seg"]:w["first_seg"] + w["n_segs"]]
            last = ss[-1]
            assert w["pos"] == ss[0]["pos"] and w["off_first"] == ss[0]["off"] and w["off_last"] == last["off"] + last["n_windows"] - 1
            assert w["n_span"] == last["pos"] + last["n_windows"] - w["pos"] and w["n_mapped"] == sum(s["n_windows"] for s in ss) <= w["n_span"]
            assert w["n_steps"] + w["n_inside"] == w["n_segs"] and w["n_covered"] <= w["n_span"] + k - 1
            path, plen, p0, p1 = path_of(k, strs, w, steps)
            if w["n_inside"] + w["n_across"] == 0:                  # consequence (b)
                n = w["n_span"] + k - 1
                assert w["indel"] == 0 and w["n_mapped"] == w["n_span"] and w["n_covered"] == n
                assert spell(strs, steps[w["first_step"]:w["first_step"] + w["n_steps"]], k)[p0:p0 + n] == text[w["pos"]:w["pos"] + n].upper(), "consequence (b)"
            if w["indel"] == 0:
                assert p1 - p0 == w["n_span"] + k - 1, "a walk without net indel: the path's span is the read's"
            assert 0 <= p0 < p1 <= plen
        assert nxt_seg == seg_offsets[r + 1]
    assert nxt_seg == len(segs) and nxt_step == len(steps)


def mirrored(k, strs, rows, walks, steps, hits, read_len):
    """the result for the reverse complement of ONE read (at flat position 0) from the read's own: (walks, steps, link_hits)"""
    mu = [len(s) - k + 1 for s in strs]
    loff = [0]
    for row in rows:
        loff.append(loff[-1] + len(row))
    out_w, out_s = [], []
    for w in reversed(walks):
        mine = steps[w["first_step"]:w["first_step"] + w["n_steps"]]
        v = dict(w)
        v.update(pos=read_len - k + 1 - (w["pos"] + w["n_span"]), first_step=len(out_s), off_first=mu[mine[-1] >> 1] - 1 - w["off_last"], off_last=mu[mine[0] >> 1] - 1 - w["off_first"])
        out_w.append(v)
        out_s += [o ^ 1 for o in reversed(mine)]
    n_segs = sum(w["n_segs"] for w in walks)
    at = 0
    for v in out_w:
        v["first_seg"] = at
        at += v["n_segs"]
    assert at == n_segs
    out_h = [0] * len(hits)
    for a, row in enumerate(rows):
        for j, b in enumerate(row):
            out_h[loff[b ^ 1] + rows[b ^ 1].index(a ^ 1)] = hits[loff[a] + j]
    return out_w, out_s, out_h


# ---- the cases: name -> (k, k-mers, counts, thr, unitig strings, reads, rows), computed once; the caller must not change them
def edited_reads(genome, n, length, seed):
    """reads cut from the genome with one lost base, one surplus base, one substitution, or two lost bases and the read
    reverse-complemented, in turn; the edit lies at least 2 k = 42 bases from either end"""
    r = random.Random(seed)
    out = []
    for i in range(n):
        a = r.randrange(len(genome) - length - 2)
        s = genome[a:a + length + 2]
        p = r.randrange(42, length - 42)
        if i % 4 == 0:
            s = s[:p] + s[p + 1:]
        elif i % 4 == 1:
            s = s[:p] + r.choice("ACGT") + s[p:]
        elif i % 4 == 2:
            s = s[:p] + r.choice([c for c in "ACGT" if c != s[p]]) + s[p + 1:]
        else:
            s = U.rc(s[:p] + s[p + 2:])
        out.append(s[:length])
    return out


def _every_kind_case():
    """k = 21: the noisy reads of the map cases, all 400 of them, plus 40 edited reads of 150 bases, on the uncleaned thr = 2 graph"""
    genome = U.rand_seq(2000, 70)
    noisy = U.noisy_reads(genome, 400, 100, 0.01, 71)
    km, cnt = U.listing_of(U.count_kmers(noisy, 21))
    strs, _ = U.unitigs(km, cnt, 21, 2)
    return 21, km, cnt, 2, strs, noisy + edited_reads(genome, 40, 150, 73)


NEW_CASE = "k21_every_kind"
WALK_CASES = sorted(R.MAP_CASES) + [NEW_CASE]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == NEW_CASE:
        k, km, cnt, thr, strs, reads = _every_kind_case()
    else:
        k, km, cnt, thr, strs, reads = R.case(name)
    if name == "k21_noisy_clean":
        res = UC.clean(km, cnt, k, thr)
        assert res["strs"] == strs
        rows = res["rows"]
    else:
        rows = L.links(km, cnt, k, thr, strs)
    return k, km, cnt, thr, strs, reads, rows


@functools.lru_cache(maxsize=None)
def mapped(name):
    """-> (segments as dicts, seg_offsets) of the case's reads, by the map's restatement"""
    k, km, cnt, thr, strs, reads, rows = case(name)
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    return segs, so


def params_of(k):
    """the three parameter pairs every case runs at"""
    return ((0, 0), (k, 0), (2 * k, 1))


@functools.lru_cache(maxsize=None)
def walked(name, max_gap, max_indel):
    k, km, cnt, thr, strs, reads, rows = case(name)
    segs, so = mapped(name)
    return walk_segs(k, strs, segs, so, rows, max_gap, max_indel)
