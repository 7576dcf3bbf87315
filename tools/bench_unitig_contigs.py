"""Cost of building contigs from the read-supported links (kmx_unitig_contigs_dev) beside two yardsticks; prints one JSON line.

The setup is tools/bench_unitig_walk.py's: its read set (150-base reads, half reverse-complemented, 1 % substitutions, at
`--coverage`x over a genome of `--genome` bases), counted at k = 31 on the device, mapped and walked (max_gap = k, max_indel = 1) on
count_unitig_graph_clean(thr = 3) of that session ("clean"), on its uncleaned thr = 3 graph ("raw") and on the uncleaned thr = 1
graph ("raw1"), whose many edges make the pruning do real work.  First the check: on reads made the same way over a genome of
`--slice` bases, the device form equals the plain-Python restatement of the rule (tests/unitig_contigs_ref.py) on the cleaned
graph, every array.  Then per graph, warmed, the median of 5 calls with [min, max], run in turn on the same device buffers:
kmx_unitig_contigs_dev at (`--min-reads`, `--ratio`); kmx_count_unitig_graph_dev at the graph's threshold, the same construction one
level down; and a device-to-device hipMemcpyAsync of n_ubases bytes, what the byte emit could at best approach.  It reports both
ratios, the seconds per phase under kmx_set_profile(m, 1) (one more call, not among the timed ones), contigs, multi-step
contigs, the N50 of unitigs and of contigs, and the stats.  Not measured: the host form, and any size the call does not name.
usage: python tools/bench_unitig_contigs.py [--genome 3000000] [--coverage 10] [--slice 20000] [--min-reads 2] [--ratio 4]"""
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

K, L = 31, 150


def n50(lens):
    lens = np.sort(np.asarray(lens, dtype=np.int64))[::-1]
    if not len(lens):
        return 0
    return int(lens[np.searchsorted(np.cumsum(lens), (int(lens.sum()) + 1) // 2)])


def slice_check(a):
    """the device form against the restatement on the reads of a small genome, cleaned thr = 3 graph -> bool"""
    import unitig_clean_ref as UC
    import unitig_contigs_ref as G
    import unitig_map_ref as R
    import unitig_walk_ref as W
    import unitigs_ref as U
    sb, sn = make_reads(a.slice, a.coverage, L, seed=6)
    reads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    res = UC.clean(km, cnt, K, 3)
    segs, so, _, _ = R.map_reads(km, K, res["strs"], reads)
    hits = W.walk_segs(K, res["strs"], segs, so, res["rows"], K, 1)[3]
    want = [np.ascontiguousarray(x).tobytes() for x in G.flat(G.contigs(K, res["strs"], res["recs"], res["rows"], hits, a.min_reads, a.ratio))]
    m = KModel(1, 65535, a.nh, a.nb)
    m.count_begin(K)
    m.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(3)
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_b = torch.from_numpy(sb).cuda()
    d_o = torch.arange(sn + 1, dtype=torch.int64, device="cuda") * L
    d_segs = torch.zeros((len(sb), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, None, None, None, d_hits)
    m.unitig_map_end()
    out, (nc, nb, nl), st = m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits[:d_lk.numel()], a.min_reads, a.ratio, urec)
    torch.cuda.synchronize()
    nu = uoff.numel() - 1
    h = [t.cpu().numpy() for t in out]
    got = [h[0][:nb].tobytes(), h[1][:nc + 1].tobytes(), h[2][:nc].tobytes(), h[3][:nu].tobytes(), h[4][:nu].tobytes(), h[5][:2 * nc + 1].tobytes(), h[6][:nl].tobytes(), h[7][:nl].tobytes(),
           np.array([st[f] for f in G.STAT_FIELDS], dtype=np.uint64).tobytes(), np.array([nc, nb, nl], dtype=np.uint64).tobytes()]
    return got == want


def one_graph(m, thr, graph, d_b, d_o, n_reads, n_bases, a):
    """link hits from the walks of the reads on one graph of the counted session, then the three timed calls -> dict"""
    ubuf, uoff, urec, d_lo, d_lk = graph
    n_uni, n_links, n_ub = int(uoff.numel() - 1), int(d_lk.numel()), int(ubuf.numel())
    out = {"thr": thr, "unitigs": n_uni, "links": n_links, "unitig_bases": n_ub}
    m.count_unitig_map_begin_dev(ubuf, uoff)
    nseg = C.c_uint64(0)
    d_so = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, None, 0, C.byref(nseg), d_so.data_ptr(), None, None), "the map's sizing call")
    d_segs = torch.zeros((max(nseg.value, 1), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_hits = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, None, None, None, d_hits)
    m.unitig_map_end()
    del d_segs
    d_hits = d_hits[:n_links]
    outs, (nc, nb, nl), st = m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, a.min_reads, a.ratio, urec)
    torch.cuda.synchronize()
    ulen = np.diff(uoff.cpu().numpy())
    clen = np.diff(outs[1].cpu().numpy()[:nc + 1])
    out.update(contigs=nc, contig_bases=nb, contig_links=nl, multi_step=st["n_multi"], stats=st, n50_unitigs=n50(ulen), n50_contigs=n50(clen), longest_contig=int(clen.max()) if nc else 0)
    # the graph call on exact room, as the cleaning and the map benches time it
    c3 = [C.c_uint64(0) for _ in range(3)]
    chk(m.L.kmx_count_unitig_graph_dev(m.h, thr, None, 0, None, None, 0, None, None, 0, C.byref(c3[0]), C.byref(c3[1]), C.byref(c3[2])), "the graph's sizing call")
    gu, gb, gl = (int(x.value) for x in c3)
    g_seq, g_off, g_rec = torch.zeros(max(gb, 1), dtype=torch.uint8, device="cuda"), torch.zeros(gu + 1, dtype=torch.int64, device="cuda"), torch.zeros((max(gu, 1), 40), dtype=torch.uint8, device="cuda")
    g_lo, g_lk = torch.zeros(2 * gu + 1, dtype=torch.int64, device="cuda"), torch.zeros(max(gl, 1), dtype=torch.int32, device="cuda")
    out["graph_call"] = {"unitigs": gu, "bases": gb, "links": gl}

    def graph_dev():
        chk(m.L.kmx_count_unitig_graph_dev(m.h, thr, g_seq.data_ptr(), gb, g_off.data_ptr(), g_rec.data_ptr(), gu, g_lo.data_ptr(), g_lk.data_ptr(), gl,
                                           C.byref(c3[0]), C.byref(c3[1]), C.byref(c3[2])), "kmx_count_unitig_graph_dev")

    def contigs_dev():
        m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, a.min_reads, a.ratio, urec, out=outs)

    d_copy = torch.empty_like(ubuf)

    def copy_dev():
        d_copy.copy_(ubuf, non_blocking=True)                   # a device-to-device hipMemcpyAsync on the current stream

    t_c, t_g, t_m = [], [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y, z = timed(contigs_dev, reps=1, warm=0)[0], timed(graph_dev, reps=1, warm=0)[0], timed(copy_dev, reps=1, warm=0)[0]
        if it:
            t_c.append(x)
            t_g.append(y)
            t_m.append(z)
    out["contigs_dev_s"], out["graph_dev_s"], out["copy_s"] = med(t_c, 5), med(t_g, 5), med(t_m, 6)
    out["contigs_over_graph"] = round(out["contigs_dev_s"][0] / out["graph_dev_s"][0], 4)
    m.set_profile(1)
    contigs_dev()
    ph = m.unitig_contigs_phases()
    m.set_profile(0)
    out["phases_s"] = {f: round(v, 6) for f, v in ph.items() if f != "rounds"}
    out["rounds"] = ph["rounds"]
    out["bytes_phase_over_copy"] = round(ph["bytes"] / max(out["copy_s"][0], 1e-9), 3)
    out["bytes_phase_gb_s"] = round(n_ub / max(ph["bytes"], 1e-9) / 1e9, 1)
    out["copy_gb_s"] = round(n_ub / max(out["copy_s"][0], 1e-9) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reads are checked against the Python restatement")
    ap.add_argument("--min-reads", type=int, default=2, dest="min_reads")
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_reads(int(a.genome), a.coverage, L)
    n_bases = n_reads * L
    res = {"metric": "unitig_contigs", "k": K, "min_reads": a.min_reads, "ratio": a.ratio, "max_gap": K, "max_indel": 1, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L,
           "reads": n_reads, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
    res["listed"] = m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(3)
    res["clean"] = one_graph(m, 3, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, n_reads, n_bases, a)
    ubuf, uoff, urec, d_lo, d_lk = m.count_unitig_graph_dev(3)
    res["raw"] = one_graph(m, 3, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, n_reads, n_bases, a)
    ubuf, uoff, urec, d_lo, d_lk = m.count_unitig_graph_dev(1)
    res["raw1"] = one_graph(m, 1, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, n_reads, n_bases, a)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
