"""Cost of lifting a unitig-level pair list to contig coordinates (kmx_unitig_pair_lift_dev) beside the calls it replaces, the
second mapping of the same pairs onto the contigs; prints one JSON line.

The input is tools/bench_unitig_scaffold.py's: paired reads (fragments of 400 +- 40 bases, mates of 150, 1 % substitutions) at
`--coverage`x over a genome of `--genome` bases, counted at k = 31 on the device, mapped, walked and paired on
count_unitig_graph(thr = 1) of that session, so that the contigs of kmx_unitig_contigs_dev (min_reads = 2, ratio = 4, the pairs per
edge added to the reads per edge) hold several unitigs.  The lift takes those unitig offsets, that place, those contig records and
that list at the pair call's max_dist.  First the check: on pairs made the same way over a genome of `--slice` bases, the device
form equals the plain-Python restatement of the rule (tests/unitig_pair_lift_ref.py) on the library's place and list, under both
fold kernels.  Then, warmed, the median of 5 calls with [min, max], run in turn on the same device buffers: the lift with the fold
inside the wavefront, the lift with the plain lane-per-item fold, and the three calls of the second mapping
(kmx_unitig_map_seqs_dev + kmx_unitig_walk_segs_dev + kmx_unitig_pair_walks_dev onto the contigs, inside a session that is begun
outside the timed span); the seconds per phase of one lift call of either fold under the profile; entries in and out and the
classes; and whether the lifted list equals the mapped one, with the number of keys that are in one list only or differ in their
record (with 1 % errors anchors can move, so it need not); and both folds once more on a crafted list of as many entries that all
lift onto one contig pair, the longest run there can be.  Not measured: the host form, the 10^8-base size, the host's second
parse of the input that the driver's switch also saves, other contig parameters, the kernels one by one.
usage: python tools/bench_unitig_pair_lift.py [--genome 3000000] [--coverage 10] [--slice 20000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_unitig_contigs import n50  # noqa: E402
from bench_unitig_map import med, timed  # noqa: E402
from bench_unitig_pairs import K, L, PARAMS, make_pairs  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import CONTIG_DTYPE, CONTIG_PLACE_DTYPE, PAIR_LIFT_DTYPE, PAIR_LINK_DTYPE  # noqa: E402

THR, MIN_READS, RATIO = 1, 2, 4
DEFAULT_FOLD = "wave"


class Mapped:
    """the buffers of one mapping of the reads onto a unitig set, allocated once: map(), walk() and pair() fill them again"""

    def __init__(self, m, d_b, d_o, n_reads, d_lo, d_lk):
        self.m, self.d_b, self.d_o, self.n_reads, self.d_lo, self.d_lk = m, d_b, d_o, n_reads, d_lo, d_lk
        self.n_links, self.n_pairs = int(d_lk.numel()), n_reads // 2
        self.d_segs = torch.zeros((n_reads * L, 24), dtype=torch.uint8, device="cuda")
        self.d_pairs = torch.zeros((self.n_pairs, 64), dtype=torch.uint8, device="cuda")
        self.d_pl = torch.zeros((self.n_pairs, 32), dtype=torch.uint8, device="cuda")
        self.d_hits = torch.zeros(max(self.n_links, 1), dtype=torch.int64, device="cuda")
        self.d_ph = torch.zeros(max(self.n_links, 1), dtype=torch.int64, device="cuda")
        self.d_so = self.d_wo = self.d_walks = self.d_steps = None

    def map(self):
        self.ns, self.d_so = self.m.seq_to_unitigs_dev(self.d_b, self.d_o, self.d_segs, self.d_so)

    def walk(self, hits=False):
        if self.d_walks is None:
            self.d_walks = torch.zeros((max(self.ns, 1), 80), dtype=torch.uint8, device="cuda")
            self.d_steps = torch.zeros(max(self.ns, 1), dtype=torch.int32, device="cuda")
        self.wst, self.d_wo = self.m.unitig_walks_dev(self.d_segs, self.ns, self.d_so, self.d_lo, self.d_lk, K, 1, self.d_walks, self.d_steps, self.d_wo, self.d_hits if hits else None)

    def pair(self, hits=False):
        self.pst, self.n_pl = self.m.unitig_pairs_dev(self.d_walks, self.wst["n_walks"], self.d_wo, self.d_steps, self.wst["n_steps"], self.d_lo, self.d_lk, PARAMS[1], PARAMS[0], PARAMS[2], PARAMS[3],
                                                      self.d_pairs, None, self.d_ph if hits else None, self.d_pl, 0)

    def all(self, hits=False):
        self.map()
        self.walk(hits)
        self.pair(hits)


def prepared(m, bases, n_reads):
    """count, graph at THR, map, walk and pair on the unitigs, the contigs from the reads and pairs per edge
    -> (listed, uoff, n_ubases, the unitig mapping, the contig call's output and counts, d_b, d_o)"""
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    listed = m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk = m.count_unitig_graph_dev(THR)
    m.count_unitig_map_begin_dev(ubuf, uoff)
    um = Mapped(m, d_b, d_o, n_reads, d_lo, d_lk)
    um.all(hits=True)
    m.unitig_map_end()
    ct, counts, cst = m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, (um.d_hits + um.d_ph)[:max(um.n_links, 1)], MIN_READS, RATIO, urec)
    torch.cuda.synchronize()
    return listed, ubuf, uoff, um, ct, counts, cst, d_b, d_o


def lists_differ(a, b):
    """two strictly ascending PAIR_LINK_DTYPE lists -> the keys that are in one only or carry different records"""
    ka, kb = (a["a"].astype(np.uint64) << 32) | a["b"], (b["a"].astype(np.uint64) << 32) | b["b"]
    both, ia, ib = np.intersect1d(ka, kb, return_indices=True)
    return len(ka) + len(kb) - len(both) - int(np.sum(a[ia] == b[ib]))


def one_run(m, n):
    """n entries that all lift onto one contig pair, the fold's worst case: unitig 2 i lies in contig 0 and unitig 2 i + 1 in contig
    1, every unitig one window, entry i goes from the one to the other -> seconds per fold kernel, median of 5, under the profile
    (the fold phase alone) and for the whole call"""
    k1 = K - 1
    uoff = torch.arange(2 * n + 1, dtype=torch.int64, device="cuda") * K
    place = np.zeros(2 * n, dtype=CONTIG_PLACE_DTYPE)
    place["oc"][1::2] = 2
    place["off"] = np.arange(2 * n) // 2
    crec = np.zeros(2, dtype=CONTIG_DTYPE)
    crec["n_kmers"] = n
    pl = np.zeros(n, dtype=PAIR_LINK_DTYPE)
    pl["a"], pl["b"] = 4 * np.arange(n), 4 * np.arange(n) + 2
    pl["n_pairs"], pl["sum_dist"], pl["min_dist"], pl["max_dist"] = 2, 20, 5, 15
    d_place = torch.from_numpy(place.view(np.int32).reshape(-1, 2)).cuda()
    d_crec = torch.from_numpy(crec.view(np.uint8).reshape(-1, 64)).cuda()
    d_pl = torch.from_numpy(pl.view(np.uint8).reshape(-1, 32)).cuda()
    out, n_out, st = m.unitig_pair_lift_dev(K, uoff, 2 * n * K + k1, d_place, d_crec, 2, d_pl, n, 2 ** 32 - 1)
    res = {"entries": n, "entries_out": n_out, "n_link": st["n_link"]}
    for which in ("wave", "plain"):
        m.unitig_pair_lift_fold(which)
        res[f"lift_{which}_s"] = med(timed(lambda: m.unitig_pair_lift_dev(K, uoff, 2 * n * K + k1, d_place, d_crec, 2, d_pl, n, 2 ** 32 - 1, out=out), reps=5, warm=1), 6)
        m.set_profile(1)
        ph = []
        for _ in range(5):
            m.unitig_pair_lift_dev(K, uoff, 2 * n * K + k1, d_place, d_crec, 2, d_pl, n, 2 ** 32 - 1, out=out)
            ph.append(m.unitig_pair_lift_phases()["fold"])
        m.set_profile(0)
        res[f"fold_{which}_s"] = med(ph, 6)[0]
    return res


def slice_check(a):
    """the device form under both folds against the restatement on the library's place and list of a small genome -> bool"""
    import unitig_pair_lift_ref as F
    sb, sn = make_pairs(a.slice, a.coverage, seed=6)
    m = KModel(1, 65535, a.nh, a.nb)
    _, ubuf, uoff, um, ct, (nc, _, _), _, _, _ = prepared(m, sb, sn)
    off = uoff.cpu().numpy()
    mu = [max(int(off[i + 1] - off[i]) - K + 1, 0) for i in range(len(off) - 1)]
    place = [tuple(int(x) for x in p) for p in ct[4].cpu().numpy().reshape(-1).view(CONTIG_PLACE_DTYPE)]
    cm = [int(x) for x in ct[2].cpu().numpy().reshape(-1).view(CONTIG_DTYPE)["n_kmers"][:nc]]
    plinks = [tuple(int(x) for x in e) for e in um.d_pl.cpu().numpy()[:um.n_pl].reshape(-1).view(PAIR_LINK_DTYPE)]
    want = F.flat(F.lift(mu, place, cm, plinks, PARAMS[1]))
    ok = True
    for fold in ("wave", "plain"):
        m.unitig_pair_lift_fold(fold)
        (d_rec, d_lout), n_out, st = m.unitig_pair_lift_dev(K, uoff, int(ubuf.numel()), ct[4], ct[2], nc, um.d_pl, um.n_pl, PARAMS[1])
        torch.cuda.synchronize()
        ok = ok and d_rec.cpu().numpy()[:um.n_pl].tobytes() == want[0].tobytes() and d_lout.cpu().numpy()[:n_out].tobytes() == want[1].tobytes() and n_out == want[2]
        ok = ok and [st[f] for f in F.STAT_FIELDS] == want[3]
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose lifted list is checked against the Python restatement")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_pairs(int(a.genome), a.coverage)
    res = {"metric": "unitig_pair_lift", "k": K, "thr": THR, "min_reads": MIN_READS, "ratio": RATIO, "max_dist": PARAMS[1], "genome_bases": int(a.genome), "coverage": a.coverage, "reads": n_reads,
           "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    res["listed"], ubuf, uoff, um, ct, (nc, ncb, ncl), cst, d_b, d_o = prepared(m, bases, n_reads)
    n_uni, n_ub, n_pl = int(uoff.numel() - 1), int(ubuf.numel()), um.n_pl
    d_cseq, d_coff, d_crec, d_place, d_cloff, d_clk = ct[0][:ncb], ct[1][:nc + 1], ct[2], ct[4], ct[5][:2 * nc + 1], ct[6][:ncl]
    l_out, n_out, lst = m.unitig_pair_lift_dev(K, uoff, n_ub, d_place, d_crec, nc, um.d_pl, n_pl, PARAMS[1])
    m.count_unitig_map_begin_dev(d_cseq, d_coff)                # the session of the second mapping stays open for the timing
    cm = Mapped(m, d_b, d_o, n_reads, d_cloff, d_clk)
    cm.all()
    torch.cuda.synchronize()
    lifted = l_out[1].cpu().numpy()[:n_out].reshape(-1).view(PAIR_LINK_DTYPE)
    mapped = cm.d_pl.cpu().numpy()[:cm.n_pl].reshape(-1).view(PAIR_LINK_DTYPE)
    rec = l_out[0].cpu().numpy()[:n_pl].reshape(-1).view(PAIR_LIFT_DTYPE)
    runs = np.bincount(rec["out"][rec["cls"] == 3]) if n_out else np.zeros(1, dtype=np.int64)
    differ = lists_differ(lifted, mapped)
    res.update(unitigs=n_uni, unitig_bases=n_ub, n50_unitigs=n50(np.diff(uoff.cpu().numpy())), contigs=nc, n_multi=cst["n_multi"], n50_contigs=n50(np.diff(d_coff.cpu().numpy())), entries_in=n_pl,
               entries_out=n_out, stats=lst, longest_run=int(runs.max()), mean_run=round(float(runs.mean()), 2), mapped_entries=cm.n_pl, mapped_stats=cm.pst, lifted_equals_mapped=differ == 0,
               differing_keys=differ)

    def lift_dev():
        m.unitig_pair_lift_dev(K, uoff, n_ub, d_place, d_crec, nc, um.d_pl, n_pl, PARAMS[1], out=l_out)

    def fold(which):
        def run():
            m.unitig_pair_lift_fold(which)
            lift_dev()
        return run

    t_w, t_p, t_m = [], [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y, z = timed(fold("wave"), reps=1, warm=0)[0], timed(fold("plain"), reps=1, warm=0)[0], timed(cm.all, reps=1, warm=0)[0]
        if it:
            t_w.append(x)
            t_p.append(y)
            t_m.append(z)
    res["lift_wave_s"], res["lift_plain_s"], res["remap_s"] = med(t_w, 6), med(t_p, 6), med(t_m, 6)
    t_1, t_2, t_3 = timed(cm.map, reps=5, warm=0), timed(cm.walk, reps=5, warm=0), timed(cm.pair, reps=5, warm=0)
    res["remap_calls_s"] = {"map_seqs": med(t_1, 6), "walk_segs": med(t_2, 6), "pair_walks": med(t_3, 6)}
    m.unitig_map_end()
    res["lift_over_remap"] = round(res["lift_wave_s"][0] / res["remap_s"][0], 6)
    m.set_profile(1)
    for which in ("wave", "plain"):
        ph = []
        for _ in range(5):
            fold(which)()
            ph.append(m.unitig_pair_lift_phases())
        res[f"phases_{which}_s"] = {f: med([p[f] for p in ph], 6)[0] for f in ph[0]}
    m.set_profile(0)
    res["one_run"] = one_run(m, n_pl)                            # as many entries as the list has, all on one contig pair
    m.unitig_pair_lift_fold(DEFAULT_FOLD)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
