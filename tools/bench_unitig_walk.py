"""Cost of threading mapped reads through the unitig graph (kmx_unitig_walk_segs_dev) beside the map call that feeds it; prints
one JSON line.

The setup is tools/bench_unitig_map.py's: its read set (150-base reads, half reverse-complemented, 1 % substitutions, at
`--coverage`x over a genome of `--genome` bases), counted at k = 31 on the device, mapped on count_unitig_graph_clean(thr = 3) of
that session ("clean") and on its uncleaned thr = 3 graph ("raw").  First the check: on reads made the same way over a genome
of `--slice` bases, the device form equals the plain-Python restatement of the rule (tests/unitig_walk_ref.py) on the cleaned
graph.  Then per graph, warmed, the median of 5 calls with [min, max], run in turn on the same device buffers:
kmx_unitig_map_seqs_dev (segments, seg_offsets, records and hits asked for) and kmx_unitig_walk_segs_dev (walks, steps,
walk_offsets and link_hits asked for, max_gap = k, max_indel = 1), their ratio, segments, walks and steps per read, and the share
of reads that become exactly one walk at max_gap = 0 and at max_gap = k.  Not measured: the host form, and any size the call
does not name.
usage: python tools/bench_unitig_walk.py [--genome 3000000] [--coverage 10] [--slice 20000]"""
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
from bench_count import make_reads  # noqa: E402
from bench_unitig_map import chk, med, timed  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import WALK_DTYPE, WalkParams, WalkStats  # noqa: E402

K, L, THR = 31, 150, 3


def slice_check(a):
    """the device form against the restatement on the reads of a small genome, cleaned graph -> bool"""
    import unitig_clean_ref as UC
    import unitig_map_ref as R
    import unitig_links_ref as UL
    import unitig_walk_ref as W
    import unitigs_ref as U
    sb, sn = make_reads(a.slice, a.coverage, L, seed=6)
    reads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    res = UC.clean(km, cnt, K, THR)
    segs, so, _, _ = R.map_reads(km, K, res["strs"], reads)
    want = [x.tobytes() for x in W.flat(*W.walk_segs(K, res["strs"], segs, so, res["rows"], K, 1))]
    m = KModel(1, 65535, a.nh, a.nb)
    m.count_begin(K)
    m.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    ok = d_lo.cpu().numpy().tobytes() == UL.flat_links(res["rows"])[0].tobytes()
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_b = torch.from_numpy(sb).cuda()
    d_o = torch.arange(sn + 1, dtype=torch.int64, device="cuda") * L
    d_segs = torch.zeros((len(sb), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    st, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps, None, d_hits)
    torch.cuda.synchronize()
    got = [d_walks.cpu().numpy()[:st["n_walks"]].tobytes(), d_wo.cpu().numpy().tobytes(), d_steps.cpu().numpy()[:st["n_steps"]].tobytes(), d_hits.cpu().numpy()[:d_lk.numel()].tobytes(),
           np.array([st[f] for f in W.STAT_FIELDS], dtype=np.uint64).tobytes()]
    m.unitig_map_end()
    return ok and got == want


def one_graph(m, graph, d_b, d_o, n_reads, n_bases):
    """map and walk on one graph of the counted session -> dict"""
    ubuf, uoff, d_lo, d_lk = graph
    n_uni, n_links = int(uoff.numel() - 1), int(d_lk.numel())
    out = {"unitigs": n_uni, "links": n_links}
    chk(m.L.kmx_count_unitig_map_begin_dev(m.h, ubuf.data_ptr(), uoff.data_ptr(), n_uni, ubuf.numel()), "kmx_count_unitig_map_begin_dev")
    ns = C.c_uint64(0)
    d_so = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    d_rec = torch.zeros((n_reads, 64), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(max(n_uni, 1), dtype=torch.int64, device="cuda")
    chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, None, 0, C.byref(ns), d_so.data_ptr(), None, None), "the map's sizing call")
    n_segs = ns.value
    d_segs = torch.zeros((max(n_segs, 1), 24), dtype=torch.uint8, device="cuda")

    def map_dev():
        chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, d_segs.data_ptr(), n_segs, C.byref(ns), d_so.data_ptr(), d_rec.data_ptr(),
                                        d_hits.data_ptr()), "kmx_unitig_map_seqs_dev")
    d_wo = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    d_lh = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    st = WalkStats()

    def walk(par, d_walks=None, d_steps=None, cap=0, hits=None):
        chk(m.L.kmx_unitig_walk_segs_dev(m.h, d_segs.data_ptr(), n_segs, d_so.data_ptr(), n_reads, d_lo.data_ptr(), d_lk.data_ptr(), n_links, C.byref(par),
                                         d_walks.data_ptr() if d_walks is not None else None, cap, d_wo.data_ptr(), d_steps.data_ptr() if d_steps is not None else None, cap,
                                         hits.data_ptr() if hits is not None else None, C.byref(st)), "kmx_unitig_walk_segs_dev")
        return st.as_dict()

    def one_walk_share(max_gap, d_walks, d_steps):
        s = walk(WalkParams(max_gap, 1), d_walks, d_steps, n_segs)
        torch.cuda.synchronize()
        per_read = np.diff(d_wo.cpu().numpy())
        return s, round(float((per_read == 1).sum()) / max(n_reads, 1), 4)

    map_dev()
    d_walks = torch.zeros((max(n_segs, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(n_segs, 1), dtype=torch.int32, device="cuda")
    _, out["one_walk_share_gap0"] = one_walk_share(0, d_walks, d_steps)
    s, out["one_walk_share_gapk"] = one_walk_share(K, d_walks, d_steps)
    w = d_walks.cpu().numpy()[:s["n_walks"]].reshape(-1).view(WALK_DTYPE)
    out.update(segments=n_segs, segments_per_read=round(n_segs / n_reads, 3), walks_per_read=round(s["n_walks"] / n_reads, 3), steps_per_read=round(s["n_steps"] / n_reads, 3),
               stats=s, walks_with_indel=int((w["indel"] != 0).sum()))
    par = WalkParams(K, 1)
    t_map, t_walk = [], []
    for it in range(6):                                          # in turn, the first pair warms
        a, b = timed(map_dev, reps=1, warm=0)[0], timed(lambda: walk(par, d_walks, d_steps, n_segs, d_lh), reps=1, warm=0)[0]
        if it:
            t_map.append(a)
            t_walk.append(b)
    out["map_dev_s"], out["walk_dev_s"] = med(t_map, 5), med(t_walk, 5)
    out["walk_over_map"] = round(out["walk_dev_s"][0] / out["map_dev_s"][0], 4)
    out["walk_segments_per_s"] = round(n_segs / out["walk_dev_s"][0])
    out["walk_sizing_s"] = med(timed(lambda: walk(par)), 5)
    m.unitig_map_end()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reads are checked against the Python restatement")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_reads(int(a.genome), a.coverage, L)
    n_bases = n_reads * L
    res = {"metric": "unitig_walk", "k": K, "thr": THR, "max_gap": K, "max_indel": 1, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L, "reads": n_reads,
           "windows": n_bases, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
    res["listed"] = m.count_finish()
    ubuf, uoff, _, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    res["clean"] = one_graph(m, (ubuf, uoff, d_lo, d_lk), d_b, d_o, n_reads, n_bases)
    ubuf, uoff, _, d_lo, d_lk = m.count_unitig_graph_dev(THR)
    res["raw"] = one_graph(m, (ubuf, uoff, d_lo, d_lk), d_b, d_o, n_reads, n_bases)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok and res["clean"]["stats"]["n_unlinked"] == 0 and res["raw"]["stats"]["n_unlinked"] == 0 else 1)


if __name__ == "__main__":
    main()
