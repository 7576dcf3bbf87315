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


CASES = {                                                      # name -> (k, thr, sequences)
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
}


def case(name: str):
    """-> (k, thr, k-mers, counts, strs, recs)"""
    k, thr, seqs = CASES[name]()
    km, cnt = listing_of(count_kmers(seqs, k))
    strs, recs = unitigs(km, cnt, k, thr)
    return k, thr, km, cnt, strs, recs
