"""Cost of the through hits (kmx_unitig_walk_through_dev) and of the resolution (kmx_unitig_resolve_dev) beside their yardsticks;
prints one JSON line.

The setup is tools/bench_unitig_contigs.py's: 150-base reads, half reverse-complemented, 1 % substitutions, at `--coverage`x over a
genome of `--genome` bases, counted at k = 31 on the device, mapped and walked (max_gap = k, max_indel = 1) on
count_unitig_graph_clean(thr = 3) of that session ("clean") and on the uncleaned thr = 1 graph ("raw1").  `--repeats N
--repeat-len L` plants N repeats in the genome before the reads are drawn: a random string of L bases, shorter than a read, written
at two random places.  First the check: on reads made the same way over a genome of `--slice` bases with 4 planted repeats, through
hits and every array of the resolution equal the plain-Python restatement (tests/unitig_resolve_ref.py) on the cleaned graph.
Then per graph, warmed, the median of 5 calls with [min, max], run in turn on the same device buffers: the through call beside
kmx_unitig_walk_segs_dev; the resolve call at (`--min-reads`, `--max-cross`) beside kmx_unitig_contigs_dev (on the unresolved graph,
at (2, 0)) and kmx_count_unitig_graph_dev; the byte phase of the resolve call (under kmx_set_profile(m, 1), one more call) beside a
device-to-device copy of the output bytes.  It reports how many repeats were planted and how many of them a resolved unitig lies
in, and contigs and N50 with and without the resolution.  Not measured: the host forms, and any size the call does not name.
usage: python tools/bench_unitig_resolve.py [--genome 3000000] [--coverage 10] [--repeats 200] [--repeat-len 60] [--slice 20000]"""
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
from bench_unitig_contigs import n50  # noqa: E402
from bench_unitig_map import chk, med, timed  # noqa: E402
from kmcex_amd import KModel, synth  # noqa: E402

K, L = 31, 150


def planted_reads(n_genome, coverage, n_repeats, repeat_len, seed=5):
    """bench_count.make_reads on a genome with planted repeats -> (uint8 bases back to back, n_reads, the repeat strings)"""
    g = ACGT[synth.genome_bases(n_genome).astype(np.int64)].copy()
    rng = np.random.default_rng(seed + 100)
    reps = []
    slots = rng.permutation(max(n_genome // (4 * L), 1))[:2 * n_repeats]      # two places per repeat, in slots of 4 reads' length: no two overlap
    for i in range(len(slots) // 2):
        s = ACGT[rng.integers(0, 4, size=repeat_len)]
        for slot in slots[2 * i:2 * i + 2]:
            at = int(slot) * 4 * L + L
            g[at:at + repeat_len] = s
        reps.append(s.tobytes().decode())
    n_reads = int(n_genome * coverage // L)
    rng = np.random.default_rng(seed)
    win = np.lib.stride_tricks.sliding_window_view(g, L)
    r = win[rng.integers(0, n_genome - L + 1, size=n_reads)].copy()
    r[1::2] = COMP[r[1::2, ::-1]]
    flat = r.reshape(-1)
    pos = np.nonzero(rng.random(flat.size, dtype=np.float32) < 0.01)[0]
    flat[pos] = ACGT[(np.searchsorted(ACGT, flat[pos]) + rng.integers(1, 4, size=pos.size)) % 4]
    return flat, n_reads, reps


def walked(m, graph, d_b, d_o, n_reads, n_bases):
    """inside a fresh session on the graph's unitigs: segments, walks, steps, link hits -> the device tensors and counts"""
    ubuf, uoff, urec, d_lo, d_lk = graph
    m.count_unitig_map_begin_dev(ubuf, uoff)
    nseg = C.c_uint64(0)
    d_so = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, None, 0, C.byref(nseg), d_so.data_ptr(), None, None), "the map's sizing call")
    d_segs = torch.zeros((max(nseg.value, 1), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    st, _ = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps, None, d_hits)
    return d_segs, ns, d_so, d_walks, d_steps, d_hits, st


def slice_check(a):
    """through hits and resolution, device forms, against the restatement on the reads of a small genome with 4 planted repeats -> bool"""
    import unitig_clean_ref as UC
    import unitig_map_ref as R
    import unitig_resolve_ref as X
    import unitig_walk_ref as W
    import unitigs_ref as U
    sb, sn, _ = planted_reads(a.slice, 3 * a.coverage, 4, a.repeat_len, seed=6)
    reads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    res = UC.clean(km, cnt, K, 3)
    segs, so, _, _ = R.map_reads(km, K, res["strs"], reads)
    walks, _, steps, hits, _ = W.walk_segs(K, res["strs"], segs, so, res["rows"], K, 1)
    t, tst = X.through(walks, steps, res["rows"], len(res["strs"]))
    want = X.flat(X.resolve(K, res["strs"], res["recs"], res["rows"], hits, t, a.min_reads, a.max_cross))
    m = KModel(1, 65535, a.nh, a.nb)
    m.count_begin(K)
    m.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(3)
    d_b = torch.from_numpy(sb).cuda()
    d_o = torch.arange(sn + 1, dtype=torch.int64, device="cuda") * L
    d_segs, ns, d_so, d_walks, d_steps, d_hits, wst = walked(m, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, sn, len(sb))
    m.unitig_map_end()
    d_t, st = m.unitig_through_dev(d_walks, wst["n_walks"], d_steps, wst["n_steps"], d_lo, d_lk)
    torch.cuda.synchronize()
    if d_t.cpu().numpy().view(np.uint64).tolist() != t or st != tst:
        return False, {}
    nl = d_lk.numel()
    out, (n, b), rst = m.unitig_resolve_dev(K, ubuf, uoff, d_lo, d_lk, d_t, a.min_reads, a.max_cross, urec, d_hits[:nl])
    torch.cuda.synchronize()
    nu = uoff.numel() - 1
    h = [x.cpu().numpy() for x in out]
    got = [h[0][:b], h[1][:n + 1], h[2][:n], h[3][:n], h[4][:nu], h[5][:2 * n + 1], h[6][:nl], h[7][:nl], h[8][:nl], np.array([rst[f] for f in X.RESOLVE_STAT_FIELDS], dtype=np.uint64),
           np.array([n, b], dtype=np.uint64)]
    return [x.tobytes() for x in got] == [np.ascontiguousarray(x).tobytes() for x in want], rst


def one_graph(m, thr, graph, d_b, d_o, n_reads, n_bases, reps, a):
    ubuf, uoff, urec, d_lo, d_lk = graph
    n_uni, n_links, n_ub = int(uoff.numel() - 1), int(d_lk.numel()), int(ubuf.numel())
    out = {"thr": thr, "unitigs": n_uni, "links": n_links, "unitig_bases": n_ub}
    d_segs, ns, d_so, d_walks, d_steps, d_hits, wst = walked(m, graph, d_b, d_o, n_reads, n_bases)
    out["walks"], out["steps"] = wst["n_walks"], wst["n_steps"]
    d_hits = d_hits[:n_links]
    d_scratch_hits = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")

    def walks_dev():
        m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps, None, d_scratch_hits)

    d_t, tst = m.unitig_through_dev(d_walks, wst["n_walks"], d_steps, wst["n_steps"], d_lo, d_lk)
    out["through_stats"] = tst
    d_scratch_t = torch.zeros_like(d_t)

    def through_dev():
        m.unitig_through_dev(d_walks, wst["n_walks"], d_steps, wst["n_steps"], d_lo, d_lk, d_scratch_t)

    t_w, t_t = [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y = timed(through_dev, reps=1, warm=0)[0], timed(walks_dev, reps=1, warm=0)[0]
        if it:
            t_t.append(x)
            t_w.append(y)
    m.unitig_map_end()
    out["through_dev_s"], out["walk_segs_dev_s"] = med(t_t, 6), med(t_w, 6)
    out["through_over_walks"] = round(out["through_dev_s"][0] / max(out["walk_segs_dev_s"][0], 1e-9), 4)
    del d_segs
    routs, (n, b), rst = m.unitig_resolve_dev(K, ubuf, uoff, d_lo, d_lk, d_t, a.min_reads, a.max_cross, urec, d_hits)
    torch.cuda.synchronize()
    out.update(resolve_stats=rst, unitigs_out=n, bases_out=b)
    place = routs[4].cpu().numpy()[:n_uni]
    ub, uo = ubuf.cpu().numpy(), uoff.cpu().numpy()
    split = [ub[uo[u]:uo[u + 1]].tobytes().decode() for u in np.nonzero(place[:, 1] > 1)[0]]
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    out["repeats_planted"] = len(reps)
    near = [x for x in split if K <= len(x) <= a.repeat_len + 16]     # a resolved unitig that lies in a planted repeat, up to 8 shared flank bases a side
    out["repeats_resolved"] = sum(1 for r in reps if any(x[8:-8] in r or rc(x)[8:-8] in r for x in near))
    couts, (nc, ncb, ncl), cst = m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, 2, 0, urec)
    c2, (nc2, ncb2, ncl2), cst2 = m.unitig_contigs_dev(K, routs[0][:b], routs[1][:n + 1], routs[5][:2 * n + 1], routs[6][:n_links], routs[8][:n_links], 2, 0, routs[2][:n])
    torch.cuda.synchronize()
    out["contigs_without"] = {"contigs": nc, "multi_step": cst["n_multi"], "n50": n50(np.diff(couts[1].cpu().numpy()[:nc + 1])), "longest": int(np.diff(couts[1].cpu().numpy()[:nc + 1]).max()) if nc else 0}
    out["contigs_with"] = {"contigs": nc2, "multi_step": cst2["n_multi"], "n50": n50(np.diff(c2[1].cpu().numpy()[:nc2 + 1])), "longest": int(np.diff(c2[1].cpu().numpy()[:nc2 + 1]).max()) if nc2 else 0}
    c3 = [C.c_uint64(0) for _ in range(3)]
    chk(m.L.kmx_count_unitig_graph_dev(m.h, thr, None, 0, None, None, 0, None, None, 0, C.byref(c3[0]), C.byref(c3[1]), C.byref(c3[2])), "the graph's sizing call")
    gu, gb, gl = (int(x.value) for x in c3)
    g_seq, g_off, g_rec = torch.zeros(max(gb, 1), dtype=torch.uint8, device="cuda"), torch.zeros(gu + 1, dtype=torch.int64, device="cuda"), torch.zeros((max(gu, 1), 40), dtype=torch.uint8, device="cuda")
    g_lo, g_lk = torch.zeros(2 * gu + 1, dtype=torch.int64, device="cuda"), torch.zeros(max(gl, 1), dtype=torch.int32, device="cuda")

    def graph_dev():
        chk(m.L.kmx_count_unitig_graph_dev(m.h, thr, g_seq.data_ptr(), gb, g_off.data_ptr(), g_rec.data_ptr(), gu, g_lo.data_ptr(), g_lk.data_ptr(), gl,
                                           C.byref(c3[0]), C.byref(c3[1]), C.byref(c3[2])), "kmx_count_unitig_graph_dev")

    def resolve_dev():
        m.unitig_resolve_dev(K, ubuf, uoff, d_lo, d_lk, d_t, a.min_reads, a.max_cross, urec, d_hits, out=routs)

    def contigs_dev():
        m.unitig_contigs_dev(K, ubuf, uoff, d_lo, d_lk, d_hits, 2, 0, urec, out=couts)

    d_src = routs[0][:b]
    d_copy = torch.empty_like(d_src)

    def copy_dev():
        d_copy.copy_(d_src, non_blocking=True)

    t_r, t_c, t_g, t_m = [], [], [], []
    for it in range(6):
        w, x, y, z = timed(resolve_dev, reps=1, warm=0)[0], timed(contigs_dev, reps=1, warm=0)[0], timed(graph_dev, reps=1, warm=0)[0], timed(copy_dev, reps=1, warm=0)[0]
        if it:
            t_r.append(w)
            t_c.append(x)
            t_g.append(y)
            t_m.append(z)
    out["resolve_dev_s"], out["contigs_dev_s"], out["graph_dev_s"], out["copy_s"] = med(t_r, 6), med(t_c, 6), med(t_g, 6), med(t_m, 6)
    out["resolve_over_contigs"] = round(out["resolve_dev_s"][0] / max(out["contigs_dev_s"][0], 1e-9), 4)
    out["resolve_over_graph"] = round(out["resolve_dev_s"][0] / max(out["graph_dev_s"][0], 1e-9), 4)
    m.set_profile(1)
    resolve_dev()
    ph = m.unitig_resolve_phases()
    m.set_profile(0)
    out["phases_s"] = {f: round(v, 6) for f, v in ph.items()}
    out["bytes_phase_over_copy"] = round(ph["bytes"] / max(out["copy_s"][0], 1e-9), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--repeat-len", type=int, default=60, dest="repeat_len")
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reads are checked against the Python restatement")
    ap.add_argument("--min-reads", type=int, default=2, dest="min_reads")
    ap.add_argument("--max-cross", type=int, default=0, dest="max_cross")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads, reps = planted_reads(int(a.genome), a.coverage, a.repeats, a.repeat_len)
    n_bases = n_reads * L
    res = {"metric": "unitig_resolve", "k": K, "min_reads": a.min_reads, "max_cross": a.max_cross, "max_gap": K, "max_indel": 1, "genome_bases": int(a.genome), "coverage": a.coverage,
           "read_len": L, "reads": n_reads, "repeats": len(reps), "repeat_len": a.repeat_len, "gen_s": round(time.perf_counter() - t0, 1)}
    ok, res["slice_resolve_stats"] = slice_check(a)
    res["slice_equals_reference"] = ok
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
    res["listed"] = m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(3)
    res["clean"] = one_graph(m, 3, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, n_reads, n_bases, reps, a)
    ubuf, uoff, urec, d_lo, d_lk = m.count_unitig_graph_dev(1)
    res["raw1"] = one_graph(m, 1, (ubuf, uoff, urec, d_lo, d_lk), d_b, d_o, n_reads, n_bases, reps, a)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
