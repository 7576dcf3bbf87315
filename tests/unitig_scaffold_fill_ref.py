"""kmx_unitig_scaffold_fill restated in plain Python, straight from the rule in include/kmx.h: every scaffold is spelled step by
step as a Python string; a link's entry is looked up in a dict, its path is a list.  Built on unitig_scaffold_ref and
unitig_pair_paths_ref.  check() tests consequences (a) to (d); flat() gives what the library returns; fasta() and fill_tsv() the
texts of the facade's writers; the rest builds the cases the CPU and GPU tests share."""
import functools
import random

import numpy as np

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pair_paths_ref as Q
import unitig_pairs_ref as P
import unitig_scaffold_ref as S
import unitig_walk_ref as W
import unitigs_ref as U

SCAFFOLD_FILL_DTYPE = np.dtype([(f, "<u8") for f in ("n_bases", "n_gap_bases", "n_fill_bases", "n_path_links", "n_adjacent_links", "n_n_links", "n_pieces", "first_piece")])
FILL_STEP_DTYPE = np.dtype([("o", "<u4"), ("kind", "<u4"), ("entry", "<u4"), ("n_pieces", "<u4"), ("off", "<u8"), ("n_front", "<u8")])
STAT_FIELDS = ("n_head", "n_path", "n_adjacent", "n_n", "n_no_entry", "n_mirror", "n_removed", "n_filled")
HEAD, N, ADJACENT, PATH = range(4)
KINDS = ("HEAD", "N", "ADJACENT", "PATH")
NO_ENTRY = 0xFFFFFFFF


def link_of(k, nu, index, precs, psteps, kinds, p, q):
    """-> (entry or NO_ENTRY, through the mirror, the kind, the path) of the link p -> q"""
    e, mirror = index.get((p, q)), False
    if e is None:
        e, mirror = index.get((q ^ 1, p ^ 1)), True
    if e is None:
        return NO_ENTRY, False, N, []
    verdict, t, fs = precs[e][:3]
    if verdict == Q.ADJACENT and kinds & 2:
        return e, mirror, ADJACENT, []
    if verdict != Q.PATH or not kinds & 1 or not 1 <= t <= Q.MAX_STEPS or fs + t > len(psteps):
        return e, mirror, N, []
    path = list(psteps[fs:fs + t])
    if any(v >= 2 * nu for v in path):
        return e, mirror, N, []
    return e, mirror, PATH, ([v ^ 1 for v in reversed(path)] if mirror else path)


def fill(k, strs, srecs, steps, plinks, precs, psteps, kinds):
    """strs: the unitig strings; srecs: (first_step, n_steps with the circular bit) per scaffold; steps: (o, n_gap, ...) per step;
    plinks: tuples whose first two fields are a and b; precs: tuples in the order of PAIR_PATH_DTYPE; psteps: a list -> a dict:
    fstrs, frecs (dicts), fsteps [(o, kind, entry, n_pieces, off, n_front)], pieces, stats"""
    nu = len(strs)
    index = {(e[0], e[1]): i for i, e in enumerate(plinks)}
    st = dict.fromkeys(STAT_FIELDS, 0)
    fstrs, frecs, fsteps, pieces = [], [], [None] * nu, []
    tail = lambda o: S.oriented(strs[o >> 1], o & 1)[k - 1:]
    for first, n in srecs:
        n &= S.CIRCULAR - 1
        r = dict.fromkeys(SCAFFOLD_FILL_DTYPE.names, 0)
        r["first_piece"] = len(pieces)
        parts, at = [], 0
        for j in range(n):
            o, n_gap = steps[first + j][:2]
            whole = S.oriented(strs[o >> 1], o & 1)
            if j == 0:
                entry, mirror, kind, path = NO_ENTRY, False, HEAD, []
            else:
                entry, mirror, kind, path = link_of(k, nu, index, precs, psteps, kinds, steps[first + j - 1][0], o)
                st["n_no_entry"] += entry == NO_ENTRY
                st["n_mirror"] += mirror
            st["n_" + KINDS[kind].lower()] += 1
            if kind == HEAD:
                front, own, off = "", whole, at
            elif kind == N:
                front, own, off = "N" * n_gap, whole, at + n_gap
                r["n_gap_bases"] += n_gap
                r["n_n_links"] += 1
            else:
                front, own = "".join(tail(v) for v in path), whole[k - 1:]
                off = at + len(front) - (k - 1)
                r["n_path_links" if kind == PATH else "n_adjacent_links"] += 1
                r["n_fill_bases"] += len(front)
                r["n_pieces"] += len(path)
                pieces += path
                st["n_removed"] += n_gap
                st["n_filled"] += len(front)
            fsteps[first + j] = (o, kind, entry, len(path), off, len(front))
            parts += [front, own]
            at += len(front) + len(own)
        r["n_bases"] = at
        fstrs.append("".join(parts))
        frecs.append(r)
    return {"fstrs": fstrs, "frecs": frecs, "fsteps": fsteps, "pieces": pieces, "stats": st}


def flat(res):
    """the result as the library lays it out -> (uint8 bases, uint64 foffsets, SCAFFOLD_FILL_DTYPE, FILL_STEP_DTYPE, uint32 pieces, stats)"""
    fseq = np.frombuffer("".join(res["fstrs"]).encode(), dtype=np.uint8)
    foffs = np.cumsum([0] + [len(s) for s in res["fstrs"]], dtype=np.uint64).astype(np.uint64)
    frec = np.zeros(len(res["frecs"]), dtype=SCAFFOLD_FILL_DTYPE)
    for i, r in enumerate(res["frecs"]):
        for f in SCAFFOLD_FILL_DTYPE.names:
            frec[i][f] = r[f]
    fsteps = np.array(res["fsteps"], dtype=FILL_STEP_DTYPE) if res["fsteps"] else np.zeros(0, dtype=FILL_STEP_DTYPE)
    return fseq, foffs, frec, fsteps, np.array(res["pieces"], dtype=np.uint32), dict(res["stats"])


def mirrored_input(plinks, precs, psteps, which):
    """the entries `which` replaced by their mirrors, with their records and steps (consequence (b) of the pair-path contract),
    where the mirror's key is not in the list already -> (plinks, precs, psteps), ascending, first_step counted anew"""
    keys = {(e[0], e[1]) for e in plinks}
    items = []
    for i, (e, r) in enumerate(zip(plinks, precs)):
        own = list(psteps[r[2]:r[2] + r[1]]) if r[0] == Q.PATH and 1 <= r[1] <= Q.MAX_STEPS and r[2] + r[1] <= len(psteps) else None
        if i in which and (e[1] ^ 1, e[0] ^ 1) not in keys and (own is not None or r[0] != Q.PATH):
            e, own = Q.mirrored(e), ([v ^ 1 for v in reversed(own)] if own is not None else None)
        items.append((tuple(e), tuple(r), own))
    items.sort(key=lambda x: (x[0][0], x[0][1]))
    out_l, out_r, out_s = [], [], []
    for e, r, own in items:
        out_l.append(e)
        if own is None:
            out_r.append(r)                                       # (a PATH record that names no steps of its own stays as it is)
        else:
            out_r.append((r[0], r[1], len(out_s)) + tuple(r[3:]))
            out_s += own
    return out_l, out_r, out_s


def check(k, strs, srecs, steps, plinks, precs, psteps, kinds, res, sstrs=None, true_overlaps=False):
    """consequences (a) to (d) of include/kmx.h, and that the pieces and the counts add up.  sstrs: the scaffold call's strings
    on the same input; true_overlaps: every filled link runs along edges that are k - 1 overlaps"""
    nu = len(strs)
    assert len(res["fsteps"]) == nu and len(res["fstrs"]) == len(srecs)
    st = res["stats"]
    assert st["n_head"] == len(srecs) and st["n_head"] + st["n_path"] + st["n_adjacent"] + st["n_n"] == nu
    assert sum(r["n_pieces"] for r in res["frecs"]) == len(res["pieces"]) and sum(r["n_fill_bases"] for r in res["frecs"]) == st["n_filled"]
    zero = fill(k, strs, srecs, steps, plinks, precs, psteps, 0)
    if sstrs is not None:                                         # (a)
        assert zero["fstrs"] == list(sstrs), "consequence (a): kinds = 0"
        if st["n_path"] + st["n_adjacent"] == 0:
            assert res["fstrs"] == list(sstrs), "consequence (a): nothing to fill"
    assert zero["stats"]["n_path"] == zero["stats"]["n_adjacent"] == 0 and not zero["pieces"]
    for s, ((first, n), r, text) in enumerate(zip(srecs, res["frecs"], res["fstrs"])):
        n &= S.CIRCULAR - 1
        lens = [len(strs[steps[first + j][0] >> 1]) for j in range(n)]
        filled = r["n_path_links"] + r["n_adjacent_links"]
        assert r["n_bases"] == len(text) == sum(lens) - (k - 1) * filled + r["n_gap_bases"] + r["n_fill_bases"], "consequence (d)"
        assert filled + r["n_n_links"] == n - 1
        at = 0
        for j in range(n):
            o, kind, entry, npc, off, n_front = res["fsteps"][first + j]
            assert o == steps[first + j][0] and (kind == HEAD) == (j == 0)
            own = S.oriented(strs[o >> 1], o & 1)
            skip = k - 1 if kind in (ADJACENT, PATH) else 0
            assert off + skip == at + n_front and text[off + skip:off + len(own)] == own[skip:]
            if kind == N:
                assert text[at:at + n_front] == "N" * n_front == "N" * steps[first + j][1]
            if true_overlaps:
                assert text[off:off + len(own)] == own, "consequence (b)"
            at = off + len(own)
        assert at == len(text)
    for which in (set(range(len(plinks))), set(range(0, len(plinks), 2))):   # (c)
        ml, mr, ms = mirrored_input(plinks, precs, psteps, which)
        assert fill(k, strs, srecs, steps, ml, mr, ms, kinds)["fstrs"] == res["fstrs"], "consequence (c)"


# ---- the text files of the facade and the driver
def fasta(res, srecs):
    return "".join(f">s{s} n_bases={r['n_bases']} n_steps={n & (S.CIRCULAR - 1)} n_gap_bases={r['n_gap_bases']} n_fill_bases={r['n_fill_bases']} circular={n >> 31}\n{t}\n"
                   for s, (t, r, (_, n)) in enumerate(zip(res["fstrs"], res["frecs"], srecs)))


def fill_tsv(res, srecs):
    """scaffolds.fill.tsv: scaffold, step, unitig, strand, kind, entry, off, the bytes in front, the path"""
    out = []
    for s, ((first, n), r) in enumerate(zip(srecs, res["frecs"])):
        at = r["first_piece"]
        for j in range(n & (S.CIRCULAR - 1)):
            o, kind, entry, npc, off, n_front = res["fsteps"][first + j]
            out.append(f"s{s}\t{j}\tu{o >> 1}\t{'-' if o & 1 else '+'}\t{KINDS[kind]}\t{'*' if entry == NO_ENTRY else entry}\t{off}\t{n_front}\t{Q.fmt_steps(res['pieces'][at:at + npc])}\n")
            at += npc
    return "".join(out)


def srecs_of(scf):
    """(first_step, n_steps with the circular bit) of what unitig_scaffold_ref.scaffold returned"""
    return [(r["first_step"], r["n_steps"] | (S.CIRCULAR if r["circular"] else 0)) for r in scf["srecs"]]


# ---- the acceptance case: a repeat of k + 4 bases (5 windows) once in each of two pieces, A x B and C x D; error-free FR pairs of
# 400-base fragments from every start of both.  The graph has the edges A -> x, C -> x, x -> B, x -> D
ACCEPT_FLANK = 500


@functools.lru_cache(maxsize=None)
def acceptance():
    """-> a dict: k, pieces (the two genome strings), strs, rows, reads, plinks (unitig_pairs_ref's list), min_pairs, par (the
    scaffold parameters), path_par"""
    k = P.K
    x = U.rand_seq(k + 4, 501)
    fl = [list(U.rand_seq(ACCEPT_FLANK, 502 + i)) for i in range(4)]
    fl[0][-1], fl[2][-1], fl[1][0], fl[3][0] = "A", "C", "G", "T"        # the repeat ends where the flanks differ
    fl = ["".join(f) for f in fl]
    pieces = [fl[0] + x + fl[1], fl[2] + x + fl[3]]
    reads = []
    for g in pieces:
        reads += P.fragments(g, range(len(g) - P.FRAG + 1))
    km, cnt = U.listing_of(U.count_kmers(reads, k))
    strs, _ = U.unitigs(km, cnt, k, 1)
    rows = L.links(km, cnt, k, 1, strs)
    segs, so, _, _ = R.map_reads(km, k, strs, reads)
    walks, wo, steps, _, _ = W.walk_segs(k, strs, segs, so, rows, k, 0)
    mu = [len(s) - k + 1 for s in strs]
    plinks = [tuple(int(v) for v in e) for e in P.pair_walks(k, mu, walks, wo, steps, rows, *P.READ_PARAMS)[1]]
    rep = [u for u in range(len(strs)) if len(strs[u]) == k + 4]
    assert len(strs) == 5 and len(rep) == 1, "choose other seeds"
    on_x = [e[2] for e in plinks if rep[0] in (e[0] >> 1, e[1] >> 1)]
    across = [e[2] for e in plinks if rep[0] not in (e[0] >> 1, e[1] >> 1)]
    assert len(across) == 2 and max(on_x) < min(across)
    min_pairs = max(on_x) + 1
    return dict(k=k, pieces=pieces, strs=strs, rows=rows, reads=reads, plinks=plinks, rep=rep[0], min_pairs=min_pairs,
                par=dict(min_pairs=min_pairs, ratio=0, inner=221, min_n=10, max_n=1000), path_par=dict(min_pairs=min_pairs, inner=221, tol=k, max_steps=8, max_visits=4096))


def through_restatements(k, strs, rows, plinks, par, path_par, kinds=3):
    """scaffold -> pair_paths -> fill, all restated -> (the scaffold result, the path result, the fill result)"""
    scf = S.scaffold(k, strs, None, plinks, **par)
    pth = Q.pair_paths([len(s) - k + 1 for s in strs], rows, plinks, **path_par)
    return scf, pth, fill(k, strs, srecs_of(scf), scf["steps"], plinks, pth["recs"], pth["psteps"], kinds)


# ---- crafted input: lists, records and steps written by hand, so no graph is needed
def rand_strs(lens, seed):
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=sum(lens), dtype=np.uint8)].tobytes().decode()
    at = np.cumsum([0] + list(lens))
    return [b[at[i]:at[i + 1]] for i in range(len(lens))]


class Craft:
    """a unitig set of the given lengths and scaffolds over it.  scaffold() takes the oriented unitigs of its steps and one link
    spec per later step: None (no entry) or a dict: verdict (Q.PATH by default), via ("F", "M" or "both": the entry as it stands,
    its mirror, or both with a decoy behind the mirror), path (the oriented unitigs between the two steps, as the scaffold reads
    them), bad ("t0", "t17", "beyond", "big": a PATH record the rule refuses).  Every unitig that no scaffold names becomes a
    scaffold of one step in build()."""

    def __init__(self, k, lens, seed=1):
        self.k, self.strs = k, rand_strs(lens, seed)
        self.scaffolds, self.entries, self.used = [], {}, set()
        self.r = random.Random(seed)

    def scaffold(self, steps, links=(), circular=False, gaps=None):
        assert len(links) == max(len(steps) - 1, 0) and not self.used & {o >> 1 for o in steps} and len({o >> 1 for o in steps}) == len(steps)
        self.used |= {o >> 1 for o in steps}
        gaps = list(gaps) if gaps is not None else [self.r.randrange(0, 40) for _ in steps]
        if not circular:
            gaps[0] = 0
        self.scaffolds.append((list(steps), circular, gaps))
        for (p, q), spec in zip(zip(steps, steps[1:]), links):
            if spec is None:
                continue
            verdict, via, path, bad = spec.get("verdict", Q.PATH), spec.get("via", "F"), list(spec.get("path", [])), spec.get("bad")
            if via in ("F", "both"):
                self.entry(p, q, verdict, path, bad)
            if via == "M":
                self.entry(q ^ 1, p ^ 1, verdict, [v ^ 1 for v in reversed(path)], bad)
            if via == "both":
                self.entry(q ^ 1, p ^ 1, Q.PATH, [(v ^ 1) for v in path[:1]] * 2, None)   # a decoy: the entry as it stands wins

    def entry(self, a, b, verdict, stored, bad=None):
        assert (a, b) not in self.entries
        self.entries[(a, b)] = (verdict, stored, bad)

    def build(self):
        nu, k = len(self.strs), self.k
        for u in range(nu):
            if u not in self.used:
                self.scaffold([2 * u + (u % 3 == 0)])
        self.scaffolds.sort(key=lambda s: min(o >> 1 for o in s[0]))
        srecs, steps = [], []
        for sc, circular, gaps in self.scaffolds:
            srecs.append((len(steps), len(sc) | (S.CIRCULAR if circular else 0)))
            steps += [(o, g, g - 3) for o, g in zip(sc, gaps)]
        plinks, precs, psteps, late = [], [], [], []
        for (a, b), (verdict, stored, bad) in sorted(self.entries.items()):
            plinks.append((a, b, 5, 250, 50, 50))
            if verdict != Q.PATH:
                precs.append((verdict, 0, len(psteps) if verdict == Q.ADJACENT else 0, 0, int(verdict in (Q.ADJACENT, Q.AMBIGUOUS)), 1))
                continue
            if bad == "big":
                stored = stored[:-1] + [2 * nu + 3]
            w = sum(len(self.strs[v >> 1]) - k + 1 for v in stored if v < 2 * nu)
            if bad == "t0":
                precs.append((Q.PATH, 0, len(psteps), 0, 1, 1))
            elif bad == "t17":
                precs.append((Q.PATH, 17, 0, w, 1, 1))
            elif bad == "beyond":
                late.append((len(precs), len(stored)))
                precs.append(None)
            else:
                precs.append((Q.PATH, len(stored), len(psteps), w, 1, len(stored) + 1))
                psteps += stored
        for i, t in late:
            precs[i] = (Q.PATH, t, len(psteps) - t + 1, 0, 1, 1)
        return dict(k=k, strs=self.strs, srecs=srecs, steps=steps, plinks=plinks, precs=precs, psteps=psteps)


def craft_arrays(c):
    """the crafted input as the library takes it -> (ubuf, uoffsets, SCAFFOLD_DTYPE srec, STEP_DTYPE steps, PAIR_LINK_DTYPE plinks,
    PAIR_PATH_DTYPE precs, uint32 psteps)"""
    ubuf = np.frombuffer("".join(c["strs"]).encode(), dtype=np.uint8)
    uoffs = np.cumsum([0] + [len(s) for s in c["strs"]], dtype=np.uint64).astype(np.uint64)
    srec = np.zeros(len(c["srecs"]), dtype=S.SCAFFOLD_DTYPE)
    srec["first_step"], srec["n_steps"] = [f for f, _ in c["srecs"]], [n for _, n in c["srecs"]]
    steps = np.array(c["steps"], dtype=S.STEP_DTYPE) if c["steps"] else np.zeros(0, dtype=S.STEP_DTYPE)
    precs = np.array(c["precs"], dtype=Q.PAIR_PATH_DTYPE).reshape(-1) if c["precs"] else np.zeros(0, dtype=Q.PAIR_PATH_DTYPE)
    return ubuf, uoffs, srec, steps, S.plinks_array(c["plinks"]), precs, np.array(c["psteps"], dtype=np.uint32)


def fill_of(c, kinds=3):
    return fill(c["k"], c["strs"], c["srecs"], c["steps"], c["plinks"], c["precs"], c["psteps"], kinds)


@functools.lru_cache(maxsize=None)
def mixed(seed=7, nu=60, k=21):
    """tens of unitigs with every feature of the rule: paths of 1 and of 16 steps, unitigs of exactly k bytes, a unitig on 5 paths
    that is also a step, entries through the mirror with reverse pieces, both entries present, the four PATH records the rule
    refuses, ADJACENT links, other verdicts, a cycle, a scaffold of one step"""
    r = random.Random(seed)
    lens = [k if u % 4 == 0 else k + r.choice((1, 2, 7, 30, 90)) for u in range(nu)]
    c = Craft(k, lens, seed)
    hub = 2 * 9 + 1                                               # on 5 paths, and a step of the first scaffold
    rnd = lambda n: [r.randrange(2 * nu) for _ in range(n)]
    c.scaffold([0, hub, 5, 6, 11, 12, 17], [dict(path=[hub ^ 1]), dict(path=[hub] + rnd(15)), dict(via="M", path=[hub, 8 * 2 + 1, 16 * 2]), dict(via="both", path=rnd(3) + [hub]),
                                           dict(verdict=Q.ADJACENT), dict(verdict=Q.ADJACENT, via="M")])
    c.scaffold([40, 43, 44, 49, 50, 55, 56, 59 * 2], [dict(path=rnd(2), bad="t0"), dict(path=rnd(2), bad="t17"), dict(path=rnd(2), bad="beyond"), dict(path=rnd(2), bad="big"), None,
                                                     dict(verdict=Q.AMBIGUOUS), dict(via="M", path=[hub, 2 * 4, 2 * 8 + 1])])
    c.scaffold([2 * 30, 2 * 31 + 1, 2 * 32], [dict(path=[2 * 4 + 1]), dict(via="M", path=[2 * 8])], circular=True)
    c.entry(2 * 32, 2 * 30, Q.PATH, [hub])                       # the closing link of the cycle has a path: never spelled
    c.entry(2 * 40, 2 * 41, Q.PATH, rnd(4))                      # an entry no link asks for
    return c.build()


def alignments(lead, k=21):
    """the first unitig `lead` bytes longer than k: every destination alignment of the piece and the step behind it; a forward and
    a reverse piece, each longer than 16 bytes, and a piece of one byte"""
    c = Craft(k, [k + lead, k + 40, k + 37, k, k + 5, k + 3], 100 + lead)
    c.scaffold([0, 8, 10], [dict(path=[2, 5, 6]), dict(via="M", path=[3, 7, 4])])
    return c.build()


def tile_of_small_pieces(k=21):
    """more than a tile of one-byte pieces: 260 links of 16 one-byte pieces each (4160 piece bytes), U = 257 + 9"""
    nu = 261 + 5
    c = Craft(k, [k + 2] * 261 + [k] * 5, 3)
    small = [2 * (261 + i) + (i & 1) for i in range(5)]
    c.scaffold([2 * u + (u % 5 == 0) for u in range(261)], [dict(via="FM"[i % 2], path=[small[(i + j) % 5] for j in range(16)]) for i in range(260)])
    assert nu == len(c.strs)
    return c.build()


def long_pieces(k=21):
    """pieces that straddle the 4096-byte tile, and one longer than a tile, forward and reverse"""
    c = Craft(k, [k + 3, k + 4085, k + 9000, k + 10, k + 2, k + 1], 4)
    c.scaffold([0, 6, 8, 10], [dict(path=[2, 3, 4]), dict(via="M", path=[5, 2, 4]), dict(path=[3])])
    return c.build()


def chain(nu, k=21, seed=9):
    """one scaffold of nu steps, every link filled in turn by a path of 1 or 2 steps, an ADJACENT entry or none: U at a block edge"""
    r = random.Random(seed)
    c = Craft(k, [k + r.choice((0, 1, 5, 17)) for _ in range(nu)], seed)
    order = list(range(nu))
    r.shuffle(order)
    steps = [2 * u + r.randrange(2) for u in order]
    specs = []
    for i in range(nu - 1):
        specs.append((dict(via="FM"[i % 2], path=[r.randrange(2 * nu)]), dict(path=[r.randrange(2 * nu), r.randrange(2 * nu)]), dict(verdict=Q.ADJACENT, via="M"), None)[i % 4])
    c.scaffold(steps, specs)
    return c.build()


def padded(c, n):
    """the crafted input with entries no link asks for (both ends on one unitig: IGNORED records) until the list holds n"""
    have = {(e[0], e[1]) for e in c["plinks"]}
    extra = [(2 * u + d, 2 * u + 1 - d) for d in (0, 1) for u in range(len(c["strs"]))]
    items = list(zip(c["plinks"], c["precs"])) + [((a, b, 1, 10, 10, 10), (Q.IGNORED, 0, 0, 0, 0, 0)) for a, b in extra if (a, b) not in have][:max(n - len(c["plinks"]), 0)]
    assert len(items) == n
    items.sort(key=lambda x: (x[0][0], x[0][1]))
    return dict(c, plinks=[e for e, _ in items], precs=[r for _, r in items])
