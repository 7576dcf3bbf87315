"""Throughput of mapping reads onto the unitig graph on the device (kmx_unitig_map_seqs_dev and the host form); prints one JSON line.

Reads: tools/bench_count.py's own read set (150-base reads, half reverse-complemented, 1 % substitutions, at `--coverage`x over
a synth.genome_bases genome of `--genome` bases), counted at k = 31 on the device; the graph is count_unitig_graph_clean(thr = 3)
of that session and the map session reads its listing where it lies.  First the checks: on reads made the same way over a
genome of `--slice` bases, host and device variant equal the plain-Python restatement of the rule (tests/unitig_map_ref.py); on
the whole input the host variant's bytes equal the device variant's.  Then, warmed, the median of 5 calls with [min, max]: the
index build (kmx_count_unitig_map_begin_dev) in ms, windows/s of kmx_unitig_map_seqs_dev (segments, seg_offsets, records and
hits all asked for) and of the host form, segments per read and the share of mapped windows.  Beside them, in turn on the same
device buffers: kmx_query_seqs_dev (seq_to_occ_dev: the model's answer per window, the number to set the map kernel against)
and kmx_count_seqs_dev (the same window roll without a lookup; above 2^26 windows its time includes the sort and merge of
every full piece).  A window is one base position of the input, as in the other sequence benchmarks.
usage: python tools/bench_unitig_map.py [--genome 3000000] [--coverage 10] [--slice 20000]"""
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
from kmcex_amd.api import SEQ_MAP_DTYPE  # noqa: E402

K, L, THR = 31, 150, 3


def med(xs, digits=4):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], digits), [round(xs[0], digits), round(xs[-1], digits)]]


def timed(fn, reps=5, warm=1):
    out = []
    for it in range(warm + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warm:
            out.append(time.perf_counter() - t)
    return out


def chk(rc, what):
    if rc:
        raise SystemExit(f"{what} failed: {rc}")


def slice_check(a):
    """host and device variant against the restatement on the reads of a small genome -> bool"""
    import unitig_clean_ref as UC
    import unitig_map_ref as R
    import unitigs_ref as U
    sb, sn = make_reads(a.slice, a.coverage, L, seed=6)
    reads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    km, cnt = U.listing_of(U.count_kmers(reads, K))
    strs = UC.clean(km, cnt, K, THR)["strs"]
    want = [x.tobytes() for x in R.flat(*R.map_reads(km, K, strs, reads))]
    m = KModel(1, 65535, a.nh, a.nb)
    m.count_begin(K)
    m.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    m.count_finish()
    got = m.count_unitig_graph_clean(THR)
    ok = [got[0][int(got[1][i]):int(got[1][i + 1])].tobytes().decode() for i in range(len(got[2]))] == strs
    m.count_unitig_map_begin(got[0], got[1])
    hits = np.zeros(len(strs), dtype=np.uint64)
    segs, so, rec = m.seq_to_unitigs_flat(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L), hits=hits)
    ok = ok and [segs.tobytes(), so.tobytes(), rec.tobytes(), hits.tobytes()] == want
    d_b = torch.from_numpy(sb).cuda()
    d_o = torch.arange(sn + 1, dtype=torch.int64, device="cuda") * L
    d_segs = torch.zeros((len(sb), 24), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros((sn, 64), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(len(strs), dtype=torch.int64, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs, None, d_rec, d_hits)
    torch.cuda.synchronize()
    ok = ok and [d_segs.cpu().numpy()[:ns].tobytes(), d_so.cpu().numpy().tobytes(), d_rec.cpu().numpy().tobytes(), d_hits.cpu().numpy().tobytes()] == want
    m.unitig_map_end()
    return ok


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
    res = {"metric": "unitig_map", "k": K, "thr": THR, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L, "reads": n_reads, "windows": n_bases,
           "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok_ref = slice_check(a)

    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
    res["listed"] = m.count_finish()
    ubuf, uoff, urec, _, _, _, st = m.count_unitig_graph_clean_dev(THR)
    n_uni = int(uoff.numel() - 1)
    res["unitigs"], res["unitig_bases"], res["clean_rounds"] = n_uni, int(ubuf.numel()), st["rounds_run"]

    def begin():
        chk(m.L.kmx_count_unitig_map_begin_dev(m.h, ubuf.data_ptr(), uoff.data_ptr(), n_uni, ubuf.numel()), "kmx_count_unitig_map_begin_dev")
    res["index_build_ms"] = med([1e3 * t for t in timed(begin)], 2)

    ns = C.c_uint64(0)
    d_so = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    d_rec = torch.zeros((n_reads, 64), dtype=torch.uint8, device="cuda")
    d_hits = torch.zeros(max(n_uni, 1), dtype=torch.int64, device="cuda")
    chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, None, 0, C.byref(ns), d_so.data_ptr(), None, None), "the sizing call")
    n_segs = ns.value
    d_segs = torch.zeros((max(n_segs, 1), 24), dtype=torch.uint8, device="cuda")

    def map_dev():
        chk(m.L.kmx_unitig_map_seqs_dev(m.h, d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, d_segs.data_ptr(), n_segs, C.byref(ns), d_so.data_ptr(), d_rec.data_ptr(),
                                        d_hits.data_ptr()), "kmx_unitig_map_seqs_dev")
    d_hits.zero_()
    t_dev = timed(map_dev, reps=1, warm=0)                     # the first call with every output: it is also the one that is compared
    rec = d_rec.cpu().numpy().reshape(-1).view(SEQ_MAP_DTYPE)
    res["segments"] = n_segs
    res["segments_per_read"] = round(n_segs / max(n_reads, 1), 3)
    res["mapped_share"] = round(float(rec["n_mapped"].sum()) / max(float(rec["n_windows"].sum()), 1.0), 4)
    dev_bytes = [d_segs.cpu().numpy().tobytes(), d_so.cpu().numpy().tobytes(), d_rec.cpu().numpy().tobytes(), d_hits.cpu().numpy()[:n_uni].tobytes()]
    t_dev = timed(map_dev)
    res["map_dev_s"] = med(t_dev)
    res["map_dev_windows_per_s"] = round(n_bases / res["map_dev_s"][0])

    offs = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)
    h_segs, h_so, h_rec = np.zeros((n_segs, 24), np.uint8), np.zeros(n_reads + 1, np.uint64), np.zeros((n_reads, 64), np.uint8)
    h_hits = np.zeros(max(n_uni, 1), np.uint64)

    def map_host():
        h_hits[:] = 0
        chk(m.L.kmx_unitig_map_seqs(m.h, bases.ctypes.data, offs.ctypes.data, n_reads, h_segs.ctypes.data, n_segs, C.byref(ns), h_so.ctypes.data, h_rec.ctypes.data, h_hits.ctypes.data),
            "kmx_unitig_map_seqs")
    res["map_host_s"] = med(timed(map_host))
    res["map_host_windows_per_s"] = round(n_bases / res["map_host_s"][0])
    res["host_equals_dev"] = ok_host = [h_segs.tobytes(), h_so.tobytes(), h_rec.tobytes(), h_hits[:n_uni].tobytes()] == dev_bytes

    # beside it, in turn on the same buffers
    d_out = torch.empty(n_bases, dtype=torch.int32, device="cuda")
    res["seq_to_occ_dev_s"] = med(timed(lambda: m.seq_to_occ_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases, d_out.data_ptr())))
    res["seq_to_occ_dev_windows_per_s"] = round(n_bases / res["seq_to_occ_dev_s"][0])
    res["map_dev_over_seq_to_occ_dev"] = round(res["map_dev_s"][0] / res["seq_to_occ_dev_s"][0], 3)
    del d_out
    m.unitig_map_end()
    times = []
    for it in range(6):                                          # (a counting session drops the listing: this comes last)
        m.count_begin(K)
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_bases)
        torch.cuda.synchronize()
        if it:
            times.append(time.perf_counter() - t)
    res["count_seqs_dev_s"] = med(times)
    res["count_seqs_dev_windows_per_s"] = round(n_bases / res["count_seqs_dev_s"][0])
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok_ref and ok_host else 1)


if __name__ == "__main__":
    main()
