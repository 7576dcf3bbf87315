"""Throughput of k-mer counting on the device (kmx_count_*, kmx_build_from_reads); prints one JSON line.

Reads: `--read-len`-base pieces (half reverse-complemented, 1 % substitutions) at `--coverage`x over a synth.genome_bases
genome of `--genome` bases: by default 150-base reads at 10x over 10^8 bases, about 8e8 windows at k = 31.  Legs:
  dev_windows_per_s   kmx_count_seqs_dev with the bases already in HBM, counting only (begin .. the last piece merged)
  finish_s            kmx_count_finish, split into filter_s (flush of the last piece + filter + cap) and build_s (the model)
  host_windows_per_s  kmx_count_seqs from host memory (bases streamed through pinned slots), counting only
  reads_e2e_s         kmx_build_from_reads on the reads as a plain FASTQ on local disk (`--dir`), parse + count + build
plus the distinct and listed k-mers.  Checks (ci = 1, cs large enough for every count): the listing is strictly ascending,
its counts sum to the valid windows, and the three legs list the same k-mers.
usage: python tools/bench_count.py [--genome 100000000] [--coverage 10] [--k 31] [--dir /tmp] [--no-file]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kmcex_amd import KModel, synth  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
COMP[ACGT] = np.frombuffer(b"TGCA", dtype=np.uint8)


def make_reads(n_genome, coverage, L, seed=5):
    """(uint8 bases of the reads back to back, n_reads): every read L bases, so the offsets are i * L"""
    g = ACGT[synth.genome_bases(n_genome).astype(np.int64)]
    n_reads = int(n_genome * coverage // L)
    rng = np.random.default_rng(seed)
    out = np.empty((n_reads, L), dtype=np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(g, L)
    step = 1 << 20
    for a in range(0, n_reads, step):
        b = min(n_reads, a + step)
        r = win[rng.integers(0, n_genome - L + 1, size=b - a)]
        r[1::2] = COMP[r[1::2, ::-1]]
        flat = r.reshape(-1)
        pos = np.nonzero(rng.random(flat.size, dtype=np.float32) < 0.01)[0]
        flat[pos] = ACGT[(np.searchsorted(ACGT, flat[pos]) + rng.integers(1, 4, size=pos.size)) % 4]
        out[a:b] = r
    return out.reshape(-1), n_reads


def write_fastq(path, bases, n_reads, L):
    reads = bases.reshape(n_reads, L)
    step = 1 << 20
    rec = np.empty((step, 2 * L + 6), dtype=np.uint8)
    rec[:, 0], rec[:, 1] = ord("@"), ord("\n")
    rec[:, 2 + L], rec[:, 3 + L], rec[:, 4 + L] = ord("\n"), ord("+"), ord("\n")
    rec[:, 5 + L:5 + 2 * L] = ord("I")
    rec[:, 5 + 2 * L] = ord("\n")
    with open(path, "wb") as f:
        for a in range(0, n_reads, step):
            b = min(n_reads, a + step)
            rec[:b - a, 2:2 + L] = reads[a:b]
            rec[:b - a].tofile(f)


def check_listing(m, windows):
    km, cnt = m.count_listing()
    asc = bool(np.all(km[1:] > km[:-1])) if km.ndim == 1 else bool(np.all((km[1:, 0] > km[:-1, 0]) | ((km[1:, 0] == km[:-1, 0]) & (km[1:, 1] > km[:-1, 1]))))
    return asc, int(cnt.astype(np.int64).sum()) == windows, len(cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=1e8)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    ap.add_argument("--dir", default=tempfile.gettempdir(), help="local disk for the FASTQ of the end-to-end leg")
    ap.add_argument("--no-file", action="store_true", help="skip the FASTQ leg")
    a = ap.parse_args()
    k, L, ci, cs = a.k, a.read_len, 1, 65535
    t0 = time.perf_counter()
    bases, n_reads = make_reads(int(a.genome), a.coverage, L)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)
    windows = n_reads * (L - k + 1)
    res = {"metric": "kmer_count", "k": k, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L,
           "reads": n_reads, "windows": windows, "gen_s": round(time.perf_counter() - t0, 1)}

    # leg 1: bases in HBM
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.from_numpy(offsets.view(np.int64)).cuda()
    m = KModel(ci, cs, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(k)                                             # warm-up: one small session (rocPRIM, first launches)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), min(n_reads, 100000), min(n_reads, 100000) * L)
    m.count_finish()
    m.count_begin(k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    torch.cuda.synchronize()
    res["dev_count_s"] = round(time.perf_counter() - t, 3)
    res["dev_windows_per_s"] = round(windows / res["dev_count_s"])
    t = time.perf_counter()
    n_listed = m.count_finish()
    res["finish_s"] = round(time.perf_counter() - t, 3)
    ins, tot = C.c_double(), C.c_double()
    m.L.kmx_last_build_seconds(m.h, C.byref(ins), C.byref(tot))
    res["build_s"] = round(tot.value, 3)
    res["filter_s"] = round(res["finish_s"] - tot.value, 3)
    res["listed"] = n_listed
    asc, sums, _ = check_listing(m, windows)
    res["distinct"] = n_listed                                   # ci = 1 and cs above every count: nothing is filtered
    res["listing_ascending"], res["counts_sum_to_windows"] = asc, sums
    del d_b, d_o, m
    torch.cuda.empty_cache()

    # leg 2: host memory
    m = KModel(ci, cs, a.nh, a.nb)
    m.count_begin(k)
    t = time.perf_counter()
    m.count_seqs(bases, offsets)                                 # (returns once its last launch has run)
    res["host_count_s"] = round(time.perf_counter() - t, 3)
    res["host_windows_per_s"] = round(windows / res["host_count_s"])
    res["host_same_listing"] = m.count_finish() == n_listed
    del m

    # leg 3: a plain FASTQ on local disk, parse + count + build
    if not a.no_file:
        path = os.path.join(a.dir, f"kmx_bench_count_{os.getpid()}.fq")
        try:
            write_fastq(path, bases, n_reads, L)
            res["fastq_bytes"] = os.path.getsize(path)
            m = KModel(ci, cs, a.nh, a.nb)
            t = time.perf_counter()
            m.init_reads(path, k)
            res["reads_e2e_s"] = round(time.perf_counter() - t, 3)
            res["reads_same_listing"] = m.stats().n_total == n_listed
            del m
        finally:
            if os.path.exists(path):
                os.remove(path)
    print(json.dumps(res), flush=True)
    ok = res["listing_ascending"] and res["counts_sum_to_windows"] and res["host_same_listing"] and res.get("reads_same_listing", True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
