"""Cost of building scaffolds from the pair links (kmx_unitig_scaffold_dev) beside two yardsticks; prints one JSON line.

The setup is tools/bench_unitig_pairs.py's: paired reads (fragments of 400 +- 40 bases, mates of 150, 1 % substitutions) at
`--coverage`x over a genome of `--genome` bases, counted at k = 31 on the device, mapped, walked and paired on
count_unitig_graph_clean(thr = 3) of that session; the scaffold call takes those unitigs and the pair list of that run, with
inner = the floor of the mean d of the pairs on one unitig, min_n = 10 and max_n = 2 max_dist.  First the check: on pairs made
the same way over a genome of `--slice` bases, the device form equals the plain-Python restatement of the rule
(tests/unitig_scaffold_ref.py) on the library's unitigs and list.  Then, warmed, the median of 5 calls with [min, max], run in
turn on the same device buffers: kmx_unitig_scaffold_dev on exact room, kmx_unitig_contigs_dev on the same set (link hits of the
walks plus the pairs per edge) and a device copy of n_sbases bytes; the seconds per phase and the doubling rounds of one call
under the profile, the byte phase (the N fill of the whole string, then the tile emit) beside the copy, the scaffolds, those of
several unitigs, the N written, and the N50 of the unitigs against the scaffolds.  Not measured: the host form, the contig-level
run (pairs mapped onto the contigs), the other gap-fill form (a kernel over the gap words only) and any size the call does not
name.
usage: python tools/bench_unitig_scaffold.py [--genome 3000000] [--coverage 10] [--slice 20000] [--min-pairs 2] [--ratio 4]"""
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
from bench_unitig_pairs import K, L, PARAMS, THR, make_pairs, walked  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import PAIR_DTYPE, PAIR_LINK_DTYPE, KmxError  # noqa: E402

MIN_N = 10


def paired(m, bases, n_reads):
    """count, clean graph, map, walk and pair on the device -> (ubuf, uoff, urec, d_lo, d_lk, d_hits, d_plinks, n_plinks, inner)"""
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    listed = m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_segs = torch.zeros((n_reads * L, 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_segs = d_segs[:max(ns, 1)].clone()
    n_links, n_pairs = int(d_lk.numel()), n_reads // 2
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    wst, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps, None, d_hits)
    d_pairs = torch.zeros((n_pairs, 64), dtype=torch.uint8, device="cuda")
    d_ph = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    d_pl = torch.zeros((n_pairs, 32), dtype=torch.uint8, device="cuda")
    pst, n_pl = m.unitig_pairs_dev(d_walks, wst["n_walks"], d_wo, d_steps, wst["n_steps"], d_lo, d_lk, PARAMS[1], PARAMS[0], PARAMS[2], PARAMS[3], d_pairs, None, d_ph, d_pl, 0)
    m.unitig_map_end()
    torch.cuda.synchronize()
    rec = d_pairs.cpu().numpy().reshape(-1).view(PAIR_DTYPE)
    d = rec["d"][(rec["cls"] == 2) & (rec["frag"] >= 0)]
    inner = max(int(d.sum() // len(d)), 0) if len(d) else 0
    return listed, ubuf, uoff, urec, d_lo, d_lk, (d_hits + d_ph)[:n_links], d_pl, n_pl, inner, pst


def scaffold(m, a, ubuf, uoff, urec, d_pl, n_pl, inner, out=None):
    """the device call, on exact room after a sizing call when `out` is None -> (out, (n_scaffolds, n_sbases), stats)"""
    if out is None:
        try:
            return m.unitig_scaffold_dev(K, ubuf, uoff, d_pl, n_pl, inner, a.min_pairs, a.ratio, MIN_N, 2 * PARAMS[1], urec, capacity=0)
        except KmxError as e:
            if e.code != -5:
                raise
            return m.unitig_scaffold_dev(K, ubuf, uoff, d_pl, n_pl, inner, a.min_pairs, a.ratio, MIN_N, 2 * PARAMS[1], urec, capacity=e.needed)
    return m.unitig_scaffold_dev(K, ubuf, uoff, d_pl, n_pl, inner, a.min_pairs, a.ratio, MIN_N, 2 * PARAMS[1], urec, out=out)


def slice_check(a):
    """the device form against the restatement on the library's unitigs and list of a small genome -> bool"""
    import unitig_scaffold_ref as S
    sb, sn = make_pairs(a.slice, a.coverage, seed=6)
    m = KModel(1, 65535, a.nh, a.nb)
    _, ubuf, uoff, urec, _, _, _, d_pl, n_pl, inner, _ = paired(m, sb, sn)
    out, (ns, nsb), st = scaffold(m, a, ubuf, uoff, None, d_pl, n_pl, inner)
    torch.cuda.synchronize()
    off, buf = uoff.cpu().numpy(), ubuf.cpu().numpy().tobytes().decode()
    strs = [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    plinks = [tuple(int(x) for x in e) for e in d_pl.cpu().numpy()[:n_pl].reshape(-1).view(PAIR_LINK_DTYPE)]
    want = S.flat(S.scaffold(K, strs, None, plinks, a.min_pairs, a.ratio, inner, MIN_N, 2 * PARAMS[1]))
    got = (out[0].cpu().numpy()[:nsb], out[1].cpu().numpy()[:ns + 1], out[2].cpu().numpy()[:ns], out[3].cpu().numpy()[:len(strs)], out[4].cpu().numpy()[:len(strs)])
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and st == want[5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose scaffolds are checked against the Python restatement")
    ap.add_argument("--min-pairs", type=int, default=2, dest="min_pairs")
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_pairs(int(a.genome), a.coverage)
    res = {"metric": "unitig_scaffold", "k": K, "thr": THR, "min_pairs": a.min_pairs, "ratio": a.ratio, "min_n": MIN_N, "max_n": 2 * PARAMS[1], "max_dist": PARAMS[1], "genome_bases": int(a.genome),
           "coverage": a.coverage, "read_len": L, "reads": n_reads, "pairs": n_reads // 2, "gap_fill": "N over sseq[0, n_sbases), then the tile emit", "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    res["listed"], ubuf, uoff, urec, d_lo, d_lk, d_hits, d_pl, n_pl, inner, pst = paired(m, bases, n_reads)
    n_uni, n_ub = int(uoff.numel() - 1), int(ubuf.numel())
    out, (ns, nsb), st = scaffold(m, a, ubuf, uoff, urec, d_pl, n_pl, inner)
    torch.cuda.synchronize()
    ulen = np.diff(uoff.cpu().numpy())
    slen = np.diff(out[1].cpu().numpy()[:ns + 1])
    gaps = int(out[2].cpu().numpy()[:ns].reshape(-1).view(np.uint64).reshape(-1, 8)[:, 5].sum())
    res.update(unitigs=n_uni, unitig_bases=n_ub, links=int(d_lk.numel()), pair_links=n_pl, inner=inner, pair_stats=pst, scaffolds=ns, scaffold_bases=nsb, n_multi=st["n_multi"], gap_bases=gaps,
               stats=st, n50_unitigs=n50(ulen), n50_scaffolds=n50(slen), longest_scaffold=int(slen.max()) if ns else 0)
    c_out = m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, 2, 4, urec)[0]
    d_copy, d_src = torch.empty(nsb, dtype=torch.uint8, device="cuda"), out[0][:nsb]

    def scaffold_dev():
        scaffold(m, a, ubuf, uoff, urec, d_pl, n_pl, inner, out)

    def contigs_dev():
        m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, 2, 4, urec, out=c_out)

    def copy_dev():
        d_copy.copy_(d_src, non_blocking=True)                   # a device-to-device hipMemcpyAsync on the current stream

    t_s, t_c, t_m = [], [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y, z = timed(scaffold_dev, reps=1, warm=0)[0], timed(contigs_dev, reps=1, warm=0)[0], timed(copy_dev, reps=1, warm=0)[0]
        if it:
            t_s.append(x)
            t_c.append(y)
            t_m.append(z)
    res["scaffold_dev_s"], res["contigs_dev_s"], res["copy_s"] = med(t_s, 5), med(t_c, 5), med(t_m, 6)
    res["scaffold_over_contigs"] = round(res["scaffold_dev_s"][0] / res["contigs_dev_s"][0], 4)
    m.set_profile(1)
    scaffold_dev()
    ph = m.unitig_scaffold_phases()
    m.set_profile(0)
    res["phases_s"] = {f: round(v, 6) for f, v in ph.items() if f != "rounds"}
    res["rounds"] = ph["rounds"]
    res["bytes_phase_over_copy"] = round(ph["bytes"] / max(res["copy_s"][0], 1e-9), 3)
    res["bytes_phase_gb_s"] = round(nsb / max(ph["bytes"], 1e-9) / 1e9, 1)
    res["copy_gb_s"] = round(nsb / max(res["copy_s"][0], 1e-9) / 1e9, 1)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
