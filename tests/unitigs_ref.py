"""The unitig rule of kmx_unitigs (include/kmx.h) restated in plain Python over a dict of strings, independent of the
library, with the checks of its output and the cases the tests and tests/golden/make_unitigs_golden.py share.  Not a test."""
import random

import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
UNITIG_DTYPE = np.dtype([("n_kmers", "<u8"), ("sum_count", "<u8"), ("min_count", "<u4"), ("max_count", "<u4"), ("first_node", "<u8"),
                         ("circular", "u1"), ("n_pred", "u1"), ("n_succ", "u1"), ("first_fwd", "u1"), ("reserved", "u1", (4,))])


def rc(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def canon(s: str) -> str:
    r = rc(s)
    return s if s <= r else r                                  # A < C < G < T as bytes and as codes: the numeric minimum


def count_kmers(seqs, k: int) -> dict:
    """{canonical k-mer: windows} over a list of str; windows with anything but ACGT are skipped"""
    out = {}
    for s in seqs:
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if set(w) <= set("ACGT"):
                c = canon(w)
                out[c] = out.get(c, 0) + 1
    return out


def listing_of(counts: dict):
    """the dict as a listing: (k-mers ascending, counts)"""
    km = sorted(counts)
    return km, [counts[x] for x in km]


class Graph:
    def __init__(self, kmers, counts, k: int, thr: int):
        self.k = k
        self.idx = {x: i for i, (x, c) in enumerate(zip(kmers, counts)) if c >= thr}
        self.count = {x: c for x, c in zip(kmers, counts)}
        self._out, self._in = {}, {}

    def succ(self, x):
        return [x[1:] + c for c in "ACGT" if canon(x[1:] + c) in self.idx]

    def pred(self, x):
        return [c + x[:-1] for c in "ACGT" if canon(c + x[:-1]) in self.idx]

    def link_out(self, x):
        if x not in self._out:
            self._out[x] = self._link_out(x)
        return self._out[x]

    def link_in(self, y):
        if y not in self._in:
            self._in[y] = self._link_in(y)
        return self._in[y]

    def _link_out(self, x):
        s = self.succ(x)
        if len(s) != 1 or len(self.pred(s[0])) != 1 or canon(s[0]) == canon(x):
            return None
        return s[0]

    def _link_in(self, y):
        p = self.pred(y)
        if len(p) != 1 or len(self.succ(p[0])) != 1 or canon(p[0]) == canon(y):
            return None
        return p[0]


def unitigs(kmers, counts, k: int, thr: int):
    """-> (list of str, list of dict records) in the rule's order; kmers: canonical strings, ascending"""
    g = Graph(kmers, counts, k, thr)
    seen, found = set(), []
    for x in kmers:
        if x not in g.idx or x in seen:
            continue
        back, y, circular = [], x, False
        while True:                                            # back to the first k-mer, or once round
            p = g.link_in(y)
            if p is None:
                break
            if p == x:
                circular = True
                break
            back.append(p)
            y = p
        path = back[::-1] + [x]
        if circular:
            nodes = [x]
            while g.link_out(nodes[-1]) != x:
                nodes.append(g.link_out(nodes[-1]))
            start = min((canon(z) for z in nodes), key=lambda z: g.idx[z])
            rep = [start]
            while g.link_out(rep[-1]) != start:
                rep.append(g.link_out(rep[-1]))
        else:
            while g.link_out(path[-1]) is not None:
                path.append(g.link_out(path[-1]))
            mirror = [rc(z) for z in reversed(path)]
            if len(path) == 1:
                rep = [canon(path[0])]
            else:
                rep = path if g.idx[canon(path[0])] < g.idx[canon(mirror[0])] else mirror
        for z in rep:
            assert canon(z) not in seen
            seen.add(canon(z))
        found.append((rep, circular))
    found.sort(key=lambda t: g.idx[canon(t[0][0])])
    strs, recs = [], []
    for rep, circular in found:
        cs = [g.count[canon(z)] for z in rep]
        strs.append(rep[0] + "".join(z[-1] for z in rep[1:]))
        recs.append({"n_kmers": len(rep), "sum_count": sum(cs), "min_count": min(cs), "max_count": max(cs),
                     "first_node": g.idx[canon(rep[0])], "circular": int(circular), "n_pred": len(g.pred(rep[0])),
                     "n_succ": len(g.succ(rep[-1])), "first_fwd": int(rep[0] == canon(rep[0]))})
    return strs, recs


def check(kmers, counts, k: int, thr: int, strs, recs):
    """the properties the rule promises, asserted on an output (of the restatement or of the library)"""
    g = Graph(kmers, counts, k, thr)
    owner = {}
    ends = []
    for u, (s, r) in enumerate(zip(strs, recs)):
        ks = [s[p:p + k] for p in range(len(s) - k + 1)]
        assert len(ks) == r["n_kmers"] >= 1 and len(s) == r["n_kmers"] + k - 1
        for z in ks:
            assert canon(z) in g.idx, "a k-mer that is no node"
            assert canon(z) not in owner, "a node twice, or in both orientations"
            owner[canon(z)] = u
        for a, b in zip(ks, ks[1:]):
            assert g.link_out(a) == b and g.link_in(b) == a, "consecutive k-mers are not linked"
            assert g.link_out(rc(b)) == rc(a), "links are not symmetric under reverse complement"
        closes = len(ks) >= 2 and g.link_out(ks[-1]) == ks[0]
        assert r["circular"] == int(closes)
        if not closes:                                         # maximal: no link leaves either end
            assert g.link_in(ks[0]) is None and g.link_out(ks[-1]) is None
            if len(ks) == 1:
                assert ks[0] == canon(ks[0])
            else:
                assert g.idx[canon(ks[0])] < g.idx[canon(ks[-1])]
        else:
            assert ks[0] == canon(ks[0]) and g.idx[ks[0]] == min(g.idx[canon(z)] for z in ks)
        cs = [g.count[canon(z)] for z in ks]
        assert (r["sum_count"], r["min_count"], r["max_count"]) == (sum(cs), min(cs), max(cs))
        assert r["first_node"] == g.idx[canon(ks[0])] and r["first_fwd"] == int(ks[0] == canon(ks[0]))
        assert r["n_pred"] == len(g.pred(ks[0])) and r["n_succ"] == len(g.succ(ks[-1]))
        ends.append(r["first_node"])
    assert set(owner) == set(g.idx), "not every node lies in a unitig"
    assert ends == sorted(ends) and len(set(ends)) == len(ends), "output order"


# ---- packed forms and flat outputs, for the tests that compare with the library
def pack(kmers, k: int) -> np.ndarray:
    """canonical strings -> packed k-mers ([n] for k <= 32, [n, 2] otherwise)"""
    v = [int("".join(str("ACGT".index(c)) for c in x), 4) for x in kmers]
    if k <= 32:
        return np.array(v, dtype=np.uint64).reshape(-1)
    return np.array([[x >> 64, x & (2 ** 64 - 1)] for x in v], dtype=np.uint64).reshape(-1, 2)


def unpack(km: np.ndarray, k: int):
    km = np.asarray(km, dtype=np.uint64)
    v = [int(x) for x in km] if km.ndim == 1 else [(int(h) << 64) | int(lo) for h, lo in km]
    return ["".join("ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in v]


def flat(strs, recs):
    """(uint8 bases, uint64 offsets, UNITIG_DTYPE records): what the library returns for this output"""
    buf = np.frombuffer("".join(strs).encode(), dtype=np.uint8).copy()
    off = np.zeros(len(strs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in strs], dtype=np.uint64)
    rec = np.zeros(len(recs), dtype=UNITIG_DTYPE)
    for i, r in enumerate(recs):
        for f, v in r.items():
            rec[f][i] = v
    return buf, off, rec


# ---- the cases, pinned by seed
def rand_seq(n: int, seed: int) -> str:
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(n))


def circular_seq(n: int, k: int, seed: int) -> str:
    s = rand_seq(n, seed)
    return s + s[:k - 1]


def noisy_reads(genome: str, n_reads: int, length: int, err: float, seed: int):
    r = random.Random(seed)
    out = []
    for _ in range(n_reads):
        p = r.randrange(len(genome) - length + 1)
        s = list(genome[p:p + length])
        for j in range(length):
            if r.random() < err:
                s[j] = r.choice([c for c in "ACGT" if c != s[j]])
        s = "".join(s)
        out.append(rc(s) if r.random() < 0.5 else s)
    return out


def small_k_case():
    s = rand_seq(200, 11)
    return [s[:100] + "AAAAAAAAA" + s[100:] + "ACGTACGTACG"]


def periodic(L: int, k: int, seed: int) -> str:
    """a random string of period L repeated to L + k - 1 bytes: a cycle of exactly L nodes, also for L < k (a draw whose L
    windows are not L distinct canonical k-mers -- a shorter period, a window that is another's reverse complement -- or have
    an edge besides the cycle's own, as happens at a small k, is drawn again)"""
    r = random.Random(seed)
    while True:
        p = "".join(r.choice("ACGT") for _ in range(L))
        s = (p * ((L + k - 1) // L + 1))[:L + k - 1]
        km, cnt = listing_of(count_kmers([s], k))
        g = Graph(km, cnt, k, 1)
        if len(km) == L and all(len(g.succ(x)) == 1 and len(g.pred(x)) == 1 for x in km):
            return s


PALETTE = (1, 2, 3, 5, 0xFFFFFFFF)


def dense(k: int, density: float, seed: int, counts=PALETTE):
    """-> (k-mers ascending, counts): every canonical k-mer kept with probability `density`, its count drawn from `counts`"""
    r = random.Random(seed)
    km, cnt = [], []
    for v in range(4 ** k):
        if r.random() < density:
            x = "".join("ACGT"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k))
            if x <= rc(x):
                km.append(x)
                cnt.append(r.choice(counts))
    return km, cnt


def top_run(k: int) -> str:
    """T..TA..A: its windows T^j A^(k-j), j <= k // 2, are canonical as they stand and lie at the top of a listing"""
    return "T" * (k // 2) + "A" * (k + 2)


def tangle(k: int, seed: int):
    """sequences whose graph has every local shape at a k where random subsets of the k-mers have no edges at all: a genome
    twice, substituted fragments of it in both orientations (bubbles and tips, single-copy), a palindromic junction (a hairpin
    edge), homopolymer runs (self-loops), the largest canonical k-mers, and isolated cycles, every other one twice"""
    r = random.Random(seed)

    def rs(n):
        return "".join(r.choice("ACGT") for _ in range(n))

    g = rs(400)
    seqs = [g, g]
    length = 2 * k + 20
    for j in range(30):
        p = r.randrange(len(g) - length + 1)
        s = list(g[p:p + length])
        for _ in range(2):
            q = r.randrange(length)
            s[q] = r.choice([c for c in "ACGT" if c != s[q]])
        s = "".join(s)
        seqs.append(rc(s) if j % 2 else s)
    h = rs(k + 8)
    seqs.append(h + rc(h))
    seqs.append(rs(k) + "C" * (k + 5) + rs(k))
    seqs.append(top_run(k))
    for j, L in enumerate((2, 3, 4, 5, 31, 32, 33, 64, 65)):
        c = periodic(L, k, 100 * seed + L)
        seqs += [c, c] if j % 2 else [c]
    return seqs


def all_cycles(k: int, lengths=range(2, 131)):
    """{L: periodic(L, k, 1000 + L)}: the cycles the tests run one by one, and k31_all_cycles in one listing"""
    return {L: periodic(L, k, 1000 + L) for L in lengths}


def cycle_and_tip():
    """a cycle of 40 nodes given twice and a single-copy tip that leaves it behind its third node: with the tip's k-mers (thr = 1)
    that node has two successors and nothing is circular; without them (thr = 2) the cycle closes"""
    k = 21
    c = periodic(40, k, 41)
    t0 = next(b for b in "ACGT" if b != c[3 + k - 1])
    return [c, c, c[3:3 + k - 1] + t0 + rand_seq(15, 42)]


def one_bucket():
    """-> (k, thr, k-mers, counts): 600 31-mers that share their first 20 bases (the windows of A^23 + 11 random bases that start
    with A^20, in families that share 8 of the 11, so that they branch), and behind them the run of top_run(31)"""
    k, r = 31, random.Random(43)
    roots = ["".join(r.choice("ACGT") for _ in range(8)) for _ in range(40)]
    got = {}
    while len(got) < 600:
        s = "A" * 23 + r.choice(roots) + "".join(r.choice("ACGT") for _ in range(3))
        for x, c in count_kmers([s], k).items():
            if x.startswith("A" * 20):
                got[x] = got.get(x, 0) + c
    both = {x: got[x] for x in sorted(got)[:600]}
    for x, c in count_kmers([top_run(k)], k).items():
        both[x] = both.get(x, 0) + c
    return (k, 1) + listing_of(both)


def equal_high_words(k: int, seed: int):
    """-> two canonical k-mers (k > 32), ascending, that share their first k - 32 bases: packed, their high words are equal"""
    r = random.Random(seed)
    head = "A" + "".join(r.choice("ACGT") for _ in range(k - 33))
    both = set()
    while len(both) < 2:
        x = head + "".join(r.choice("ACGT") for _ in range(32))
        if canon(x) == x:
            both.add(x)
    return sorted(both)


def _listing(k, thr, listing):
    return (k, thr) + tuple(listing)


CASES = {                                                      # name -> (k, thr, sequences) or (k, thr, k-mers, counts)
    "k5_loops_hairpins": lambda: (5, 1, small_k_case()),
    "k7_cycle30": lambda: (7, 1, [circular_seq(30, 7, 2)]),
    "k7_cycle40": lambda: (7, 1, [circular_seq(40, 7, 4)]),
    "k7_two_cycles_and_line": lambda: (7, 1, [circular_seq(30, 7, 2), circular_seq(40, 7, 4), rand_seq(60, 3)]),
    "k5_cycle2": lambda: (5, 1, ["ACACAC"]),                     # cycles of 2^j nodes: every pointer returns to its own node in round j
    "k7_cycle2": lambda: (7, 1, ["ACACACAC"]),
    "k7_cycle32": lambda: (7, 1, [circular_seq(32, 7, 3)]),
    "k9_cycle64": lambda: (9, 1, [circular_seq(64, 9, 2)]),
    "k7_cycle2_and_line": lambda: (7, 1, ["ACACACAC", rand_seq(60, 5)]),
    "k7_cycles_2_32_30_and_line": lambda: (7, 1, ["ACACACAC", circular_seq(32, 7, 3), circular_seq(30, 7, 2), rand_seq(60, 5)]),
    "k7_linear300": lambda: (7, 1, [rand_seq(300, 31)]),
    "k9_linear2000": lambda: (9, 1, [rand_seq(2000, 32)]),
    "k15_long_path": lambda: (15, 1, [rand_seq(6000, 33)]),
    "k33_cycle400": lambda: (33, 1, [circular_seq(400, 33, 34)]),
    "k63_linear": lambda: (63, 1, [rand_seq(500, 35)]),
    "reads_thr1": lambda: (21, 1, noisy_reads(rand_seq(5000, 36), 1000, 100, 0.01, 37)),
    "reads_thr3": lambda: (21, 3, noisy_reads(rand_seq(5000, 36), 1000, 100, 0.01, 37)),
    # every canonical k-mer, or a random subset: nodes of degree 3 and 4 on both sides, hairpins, self-loops, mirror pairs
    "k5_complete": lambda: _listing(5, 1, dense(5, 1.0, 50, (1,))),
    "k5_dense_thr3": lambda: _listing(5, 3, dense(5, 1.0, 51)),
    "k7_complete": lambda: _listing(7, 1, dense(7, 1.0, 52)),
    "k7_half_thr1": lambda: _listing(7, 1, dense(7, 0.5, 53)),
    "k7_half_thr3": lambda: _listing(7, 3, dense(7, 0.5, 53)),
    "k7_tenth": lambda: _listing(7, 0, dense(7, 0.1, 54, (0,) + PALETTE)),     # thr = 0: a count of 0 is a node
    "k9_dense": lambda: _listing(9, 0xFFFFFFFF, dense(9, 0.1, 55)),            # the largest thr: a fifth of the entries are nodes
    "k11_sparse": lambda: _listing(11, 2, dense(11, 0.02, 56)),
    **{f"tangle_k{k}_thr{thr}": (lambda k=k, thr=thr: (k, thr, tangle(k, k))) for k in (31, 33, 35, 47, 61, 63) for thr in (1, 2)},
    "k31_all_cycles": lambda: (31, 1, list(all_cycles(31).values()) + [rand_seq(700, 57)]),
    "cycle_only_above_thr": lambda: (21, 2, cycle_and_tip()),
    "cycle_only_above_thr_at1": lambda: (21, 1, cycle_and_tip()),
    "one_bucket": one_bucket,
}


def case(name: str):
    """-> (k, thr, k-mers, counts, strs, recs), the caller's own: a caller that asks twice keeps them itself"""
    c = CASES[name]()
    if len(c) == 3:
        k, thr, seqs = c
        km, cnt = listing_of(count_kmers(seqs, k))
    else:
        k, thr, km, cnt = c
    strs, recs = unitigs(km, cnt, k, thr)
    return k, thr, km, cnt, strs, recs
