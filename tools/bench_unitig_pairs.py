"""Cost of placing read pairs on the unitig graph (kmx_unitig_pair_walks_dev) beside the walk call that feeds it; prints one JSON
line.

The setup is tools/bench_unitig_walk.py's with paired reads: fragments of 400 +- 40 bases from a genome of `--genome` bases, both
mates 150 bases, mate 2 reverse-complemented, interleaved, 1 % substitutions, at `--coverage`x; counted at k = 31 on the device
and mapped on count_unitig_graph_clean(thr = 3) of that session.  First the check: on pairs made the same way over a genome of
`--slice` bases, the device form equals the plain-Python restatement of the rule (tests/unitig_pairs_ref.py).  Then, warmed, the
median of 5 calls with [min, max], run in turn on the same device buffers: kmx_unitig_walk_segs_dev (walks, steps, walk_offsets
and link_hits asked for, max_gap = k, max_indel = 1) and kmx_unitig_pair_walks_dev (records, hist, pair_hits and the list asked
for, merged into an empty list; min_mapped = 1, max_dist = 1000, bins of 10 bases), their ratio, the pairs per class and the
median fragment by the histogram.  Not measured: the host form, a merge into a list that already holds entries, and any size the
call does not name.
usage: python tools/bench_unitig_pairs.py [--genome 3000000] [--coverage 10] [--slice 20000]"""
import argparse
import ctypes as C
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
from bench_count import ACGT, COMP  # noqa: E402
from bench_unitig_map import chk, med, timed  # noqa: E402
from kmcex_amd import KModel, synth  # noqa: E402
from kmcex_amd.api import PairParams, PairStats, WalkParams, WalkStats  # noqa: E402

K, L, THR = 31, 150, 3
FRAG, FRAG_SD = 400, 40
PARAMS = (1, 1000, 10, 200)                                    # min_mapped, max_dist, bin_width, n_bins


def make_pairs(n_genome, coverage, seed=5):
    """(uint8 bases of the interleaved mates back to back, n_reads): every read L bases, so the offsets are i * L"""
    g = ACGT[synth.genome_bases(n_genome).astype(np.int64)]
    n_pairs = int(n_genome * coverage // (2 * L))
    rng = np.random.default_rng(seed)
    out = np.empty((2 * n_pairs, L), dtype=np.uint8)
    step = 1 << 19
    for a in range(0, n_pairs, step):
        b = min(n_pairs, a + step)
        frag = np.clip(np.rint(rng.normal(FRAG, FRAG_SD, size=b - a)).astype(np.int64), L, min(2 * FRAG, n_genome))
        start = (rng.random(b - a) * (n_genome - frag + 1)).astype(np.int64)
        r = out[2 * a:2 * b]
        r[0::2] = g[start[:, None] + np.arange(L)]
        r[1::2] = COMP[g[(start + frag - 1)[:, None] - np.arange(L)]]
        flat = r.reshape(-1)
        pos = np.nonzero(rng.random(flat.size, dtype=np.float32) < 0.01)[0]
        flat[pos] = ACGT[(np.searchsorted(ACGT, flat[pos]) + rng.integers(1, 4, size=pos.size)) % 4]
    return out.reshape(-1), 2 * n_pairs


def walked(m, d_b, d_o, n_reads, n_bases, d_lo, d_lk):
    """the reads mapped and walked on the device -> (d_segs, n_segs, d_so, d_walks, d_steps, d_wo, walk stats)"""
    d_segs = torch.zeros((n_bases, 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_segs = d_segs[:max(ns, 1)].clone()
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    st, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps)
    return d_segs, ns, d_so, d_walks, d_steps, d_wo, st


def slice_check(a):
    """the device form against the restatement on the pairs of a small genome, cleaned graph -> bool"""
    import unitig_clean_ref as UC
    import unitig_map_ref as R
    import unitig_pairs_ref as P
    import unitig_walk_ref as W
    import unitigs_ref as U
    sb, sn = make_pairs(a.slice, a.coverage, seed=6)
    reads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    res = UC.clean(km, cnt, K, THR)
    segs, so, _, _ = R.map_reads(km, K, res["strs"], reads)
    walks, wo, steps, _, _ = W.walk_segs(K, res["strs"], segs, so, res["rows"], K, 1)
    want = [x.tobytes() for x in P.flat(*P.pair_walks(K, [len(s) - K + 1 for s in res["strs"]], walks, wo, steps, res["rows"], *PARAMS))]
    m = KModel(1, 65535, a.nh, a.nb)
    m.count_begin(K)
    m.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_b = torch.from_numpy(sb).cuda()
    d_o = torch.arange(sn + 1, dtype=torch.int64, device="cuda") * L
    d_segs, ns, d_so, d_walks, d_steps, d_wo, wst = walked(m, d_b, d_o, sn, len(sb), d_lo, d_lk)
    n_pairs = sn // 2
    d_pairs = torch.zeros((n_pairs, 64), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(PARAMS[3], dtype=torch.int64, device="cuda")
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    d_pl = torch.zeros((n_pairs, 32), dtype=torch.uint8, device="cuda")
    st, n = m.unitig_pairs_dev(d_walks, wst["n_walks"], d_wo, d_steps, wst["n_steps"], d_lo, d_lk, PARAMS[1], PARAMS[0], PARAMS[2], PARAMS[3], d_pairs, d_hist, d_hits, d_pl, 0)
    torch.cuda.synchronize()
    got = [d_pairs.cpu().numpy().tobytes(), d_pl.cpu().numpy()[:n].tobytes(), d_hist.cpu().numpy().tobytes(), d_hits.cpu().numpy()[:d_lk.numel()].tobytes(),
           np.array([st[f] for f in P.STAT_FIELDS], dtype=np.uint64).tobytes()]
    m.unitig_map_end()
    return got == want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose pairs are checked against the Python restatement")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_pairs(int(a.genome), a.coverage)
    n_bases, n_pairs = n_reads * L, n_reads // 2
    res = {"metric": "unitig_pairs", "k": K, "thr": THR, "max_gap": K, "max_indel": 1, "min_mapped": PARAMS[0], "max_dist": PARAMS[1], "bin_width": PARAMS[2], "n_bins": PARAMS[3],
           "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L, "fragment": [FRAG, FRAG_SD], "reads": n_reads, "pairs": n_pairs, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
    res["listed"] = m.count_finish()
    ubuf, uoff, _, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    n_uni, n_links = int(uoff.numel() - 1), int(d_lk.numel())
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_segs, n_segs, d_so, d_walks, d_steps, d_wo, wst = walked(m, d_b, d_o, n_reads, n_bases, d_lo, d_lk)
    res.update(unitigs=n_uni, links=n_links, segments=n_segs, walks=wst["n_walks"], steps=wst["n_steps"])
    d_lh = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    d_pairs = torch.zeros((n_pairs, 64), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(PARAMS[3], dtype=torch.int64, device="cuda")
    d_ph = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    d_pl = torch.zeros((n_pairs, 32), dtype=torch.uint8, device="cuda")
    wpar, wstat, ppar, pstat, n_pl = WalkParams(K, 1), WalkStats(), PairParams(*PARAMS), PairStats(), C.c_uint64(0)

    def walk():
        chk(m.L.kmx_unitig_walk_segs_dev(m.h, d_segs.data_ptr(), n_segs, d_so.data_ptr(), n_reads, d_lo.data_ptr(), d_lk.data_ptr(), n_links, C.byref(wpar), d_walks.data_ptr(), n_segs,
                                         d_wo.data_ptr(), d_steps.data_ptr(), n_segs, d_lh.data_ptr(), C.byref(wstat)), "kmx_unitig_walk_segs_dev")

    def pair():
        n_pl.value = 0
        chk(m.L.kmx_unitig_pair_walks_dev(m.h, d_walks.data_ptr(), wst["n_walks"], d_wo.data_ptr(), n_reads, d_steps.data_ptr(), wst["n_steps"], d_lo.data_ptr(), d_lk.data_ptr(), n_links,
                                          C.byref(ppar), d_pairs.data_ptr(), d_hist.data_ptr(), d_ph.data_ptr(), d_pl.data_ptr(), n_pairs, C.byref(n_pl), C.byref(pstat)),
            "kmx_unitig_pair_walks_dev")

    pair()
    torch.cuda.synchronize()
    hist = d_hist.cpu().numpy().view(np.uint64)
    cum = np.cumsum(hist)
    res.update(stats=pstat.as_dict(), pair_links=int(n_pl.value), median_fragment_bin=int(np.searchsorted(cum, (int(cum[-1]) + 1) // 2)) * PARAMS[2] if cum[-1] else None)
    t_walk, t_pair = [], []
    for it in range(6):                                          # in turn, the first two warm
        x, y = timed(walk, reps=1, warm=0)[0], timed(pair, reps=1, warm=0)[0]
        if it:
            t_walk.append(x)
            t_pair.append(y)
    res["walk_dev_s"], res["pair_dev_s"] = med(t_walk, 5), med(t_pair, 5)
    res["pair_over_walk"] = round(res["pair_dev_s"][0] / res["walk_dev_s"][0], 4)
    res["pairs_per_s"] = round(n_pairs / res["pair_dev_s"][0])
    m.unitig_map_end()
    print(json.dumps(res), flush=True)
    s = res["stats"]
    sys.exit(0 if ok and s["n_none"] + s["n_single"] + s["n_same"] + s["n_inverted"] + s["n_link"] + s["n_far"] == n_pairs else 1)


if __name__ == "__main__":
    main()
