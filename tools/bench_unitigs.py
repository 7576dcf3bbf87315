"""Throughput of the unitig construction on the device (kmx_count_unitigs_dev on a counted session); prints one JSON line.

Reads: tools/bench_count.py's own read set (150-base reads, half reverse-complemented, 1 % substitutions, at `--coverage`x over
a synth.genome_bases genome of `--genome` bases; by default 10x over 10^8 bases), counted at k = 31 on the device.  First the
checks: the device variant's bytes equal the host variant's on the whole input, and on reads made the same way over a genome
of `--slice` bases both equal the plain-Python restatement of the rule (tests/unitigs_ref.py).  Then, for thr = 1 and thr = 3, warmed,
the median of 5 calls with [min, max]: seconds, nodes/s and unitigs/s, the N50 of the unitigs, and (from one further call under
set_profile(1), where every phase waits for the stream) the seconds per phase -- adjacency, links, ranking with its round
count, emit.  Beside each of these, on the same listing and interleaved call by call with the above, kmx_count_unitig_graph_dev
(the same with the edges between unitigs): its seconds and nodes/s, n_links, and links_s, the seconds of its links phase under
set_profile(1); the slice check covers its link_offsets and links (tests/unitig_links_ref.py).  Yardsticks that are not the code under test: kmx_query_packed_dev's k-mers/s on the same 8 n neighbour k-mers
(the model answers the same 8 questions per node, inexactly), and the same session's kmx_count_finish time.
usage: python tools/bench_unitigs.py [--genome 100000000] [--coverage 10] [--slice 20000]"""
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
from kmcex_amd import KModel  # noqa: E402

K, L = 31, 150
MASK = (1 << (2 * K)) - 1


def med(xs):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], 4), [round(xs[0], 4), round(xs[-1], 4)]]


def revcomp_dev(y):
    """reverse complement of packed 31-mers held in int64 tensors (62 bits, so every value is non-negative)"""
    x = (~y) & MASK
    for s, msk in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        m = msk if msk < (1 << 63) else msk - (1 << 64)
        x = ((x >> s) & m) | ((x & m) << s)
    x = ((x >> 32) & 0xFFFFFFFF) | (x << 32)
    return (x >> (64 - 2 * K)) & MASK


def neighbours_dev(d_km, j):
    """the canonical form of neighbour j (0..3 successors, 4..7 predecessors) of every listed k-mer"""
    c = j & 3
    y = (((d_km << 2) | c) & MASK) if j < 4 else ((d_km >> 2) | (c << (2 * K - 2)))
    return torch.minimum(y, revcomp_dev(y))


def n50(lengths):
    s = np.sort(np.asarray(lengths, dtype=np.int64))[::-1]
    c = np.cumsum(s)
    return int(s[np.searchsorted(c, (c[-1] + 1) // 2)]) if len(s) else 0


def from_dev(got):
    buf, off, rec = got
    return buf.cpu().numpy().tobytes(), off.cpu().numpy().tobytes(), rec.cpu().numpy().tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=1e8)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reads are checked against the Python restatement")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_reads(int(a.genome), a.coverage, L)
    res = {"metric": "unitigs", "k": K, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L, "reads": n_reads,
           "gen_s": round(time.perf_counter() - t0, 1)}

    # check 1: the reference rule on the reads of a small genome of its own (the same generator)
    import unitigs_ref as U
    sb, sn = make_reads(a.slice, a.coverage, L, seed=6)
    sreads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    skm, scnt = U.listing_of(U.count_kmers(sreads, K))
    import unitig_links_ref as UL
    ok_ref = ok_links = True
    ms = KModel(1, 65535, a.nh, a.nb)
    ms.count_begin(K)
    ms.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    ms.count_finish()
    for thr in (1, 3):
        sstrs, srecs = U.unitigs(skm, scnt, K, thr)
        want = tuple(x.tobytes() for x in U.flat(sstrs, srecs))
        wantg = want + tuple(x.tobytes() for x in UL.flat_links(UL.links(skm, scnt, K, thr, sstrs)))
        ok_links = ok_links and tuple(np.asarray(x).tobytes() for x in ms.count_unitig_graph(thr)) == wantg
        ok_links = ok_links and tuple(x.cpu().numpy().tobytes() for x in ms.count_unitig_graph_dev(thr)) == wantg
        got = ms.count_unitigs(thr)
        ok_ref = ok_ref and tuple(np.asarray(x).tobytes() for x in got) == want and from_dev(ms.count_unitigs_dev(thr)) == want
    res["slice_equals_reference"] = ok_ref
    res["slice_links_equal_reference"] = ok_links
    del ms

    # the session
    d_b = torch.from_numpy(bases).cuda()
    d_o = (torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    torch.cuda.synchronize()
    t = time.perf_counter()
    n = m.count_finish()
    torch.cuda.synchronize()
    res["count_finish_s"] = round(time.perf_counter() - t, 3)
    res["listed"] = n
    del d_b, d_o
    torch.cuda.empty_cache()

    # check 2: device variant == host variant on the whole input
    ok_host = True
    nu, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    for thr in (1, 3):
        gg = m.count_unitig_graph_dev(thr)
        loff, lks = gg[3], gg[4]
        got = m.count_unitigs_dev(thr)
        ok_host = ok_host and from_dev(gg[:3]) == from_dev(got)
        host = m.count_unitigs(thr)
        ok_host = ok_host and from_dev(got) == tuple(np.asarray(x).tobytes() for x in host)
        buf, off, rec = got
        r = {"unitigs": int(off.numel() - 1), "bases": int(buf.numel())}
        lens = (off[1:] - off[:-1]).cpu().numpy()
        r["n50"] = n50(lens)
        r["nodes"] = int(lens.sum() - (K - 1) * len(lens))
        r["n_links"] = int(lks.numel())
        times, gtimes = [], []
        graph_args = (m.h, thr, gg[0].data_ptr(), gg[0].numel(), gg[1].data_ptr(), gg[2].data_ptr(), gg[2].shape[0], loff.data_ptr(), lks.data_ptr(), lks.numel(),
                      C.byref(nu), C.byref(nb), C.byref(nl))
        for it in range(6):                                        # the first call above warmed the buffers; one more, then 5
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = m.L.kmx_count_unitigs_dev(m.h, thr, buf.data_ptr(), buf.numel(), off.data_ptr(), rec.data_ptr(), rec.shape[0], C.byref(nu), C.byref(nb))
            torch.cuda.synchronize()
            if rc:
                raise SystemExit(f"kmx_count_unitigs_dev failed: {rc}")
            if it:
                times.append(time.perf_counter() - t)
            torch.cuda.synchronize()                               # the graph call in turn with its twin
            t = time.perf_counter()
            rc = m.L.kmx_count_unitig_graph_dev(*graph_args)
            torch.cuda.synchronize()
            if rc:
                raise SystemExit(f"kmx_count_unitig_graph_dev failed: {rc}")
            if it:
                gtimes.append(time.perf_counter() - t)
        r["seconds"] = med(times)
        r["graph_seconds"] = med(gtimes)
        r["graph_nodes_per_s"] = round(r["nodes"] / r["graph_seconds"][0])
        r["nodes_per_s"] = round(r["nodes"] / r["seconds"][0])
        r["unitigs_per_s"] = round(r["unitigs"] / r["seconds"][0])
        m.set_profile(1)
        m.L.kmx_count_unitigs_dev(m.h, thr, buf.data_ptr(), buf.numel(), off.data_ptr(), rec.data_ptr(), rec.shape[0], C.byref(nu), C.byref(nb))
        torch.cuda.synchronize()
        m.set_profile(0)
        m.kernel_times(reset=True)
        ph = m.unitigs_phases()
        r["phase_s"] = {p: round(ph[p], 4) for p in ("adjacency", "links", "ranking", "emit")}
        r["rounds"] = ph["rounds"]
        m.set_profile(1)
        m.L.kmx_count_unitig_graph_dev(*graph_args)
        torch.cuda.synchronize()
        m.set_profile(0)
        m.kernel_times(reset=True)
        gph = m.unitig_graph_phases()
        r["links_s"] = round(gph["unitig_links"], 4)
        r["graph_phase_s"] = {p: round(gph[p], 4) for p in ("adjacency", "links", "ranking", "emit", "unitig_links")}
        res[f"thr{thr}"] = r
        del got, buf, off, rec, host, gg, loff, lks, graph_args
        torch.cuda.empty_cache()
    res["dev_equals_host"] = ok_host

    # yardstick: the model's answers to the same 8 n neighbour k-mers
    km, _ = m.count_listing()
    d_km = torch.from_numpy(km.view(np.int64)).cuda()
    d_out = torch.empty(n, dtype=torch.int32, device="cuda")
    per = []
    for it in range(6):
        s = 0.0
        for j in range(8):
            q = neighbours_dev(d_km, j)
            torch.cuda.synchronize()
            t = time.perf_counter()
            m.kmer_to_occ_dev(q.data_ptr(), n, d_out.data_ptr())
            torch.cuda.synchronize()
            s += time.perf_counter() - t
            del q
        if it:
            per.append(s)
    res["query_packed_dev_8n_s"] = med(per)
    res["query_packed_dev_kmers_per_s"] = round(8 * n / res["query_packed_dev_8n_s"][0])
    res["adjacency_questions_per_s"] = round(8 * n / max(res["thr1"]["phase_s"]["adjacency"], 1e-9))
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok_ref and ok_links and ok_host else 1)


if __name__ == "__main__":
    main()
