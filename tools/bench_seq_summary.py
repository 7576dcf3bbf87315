"""Throughput of the per-sequence summary (kmx_summarise_seqs) against what a caller had before it; prints one JSON line.

tools/bench_seq.py's input: the model of all k-mers of a random 10^8-base sequence, reads of `--read-len` bases of it with
1 % substitutions, about 10^8 windows.  Legs, in windows/s (median of `--reps`, min and max beside it):
  a  seq_summary_dev: bases and offsets in HBM, 64-byte records out            (kernel rate from HBM)
  b  seq_to_occ_dev on the same buffers: 4 bytes per base out                  (kernel rate from HBM)
  c  b, then a segment reduction of its output with torch on the device        (what a caller had in HBM)
  d  seq_summary_flat from host memory                                         (end-to-end rate from host memory)
  e  seq_to_occ_flat, then np.add / minimum / maximum.reduceat over its output (what a caller had from host memory)
  f  seq_to_occ_flat alone                                                     (end-to-end rate from host memory)
Every leg is warmed up, the device is synchronised around each timed call, a / b / c and d / e / f alternate in one loop.
Before anything is timed: a == the NumPy reduction of b's output, and d == a, on the timed inputs.
usage: python tools/bench_seq_summary.py [--reps 5] [--n-bases 100000000] [--windows 100000000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seq_summary_ref as S  # noqa: E402
from kmcex_amd import KModel, api, synth_torch  # noqa: E402

THR = (1, 3, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ci", type=int, default=1)
    ap.add_argument("--cs", type=int, default=1023)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    ap.add_argument("--n-bases", type=int, default=100_000_000)
    ap.add_argument("--windows", type=int, default=100_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, L = a.k, a.read_len
    assert k <= 32 and L >= k
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bases = torch.randint(0, 4, (a.n_bases,), dtype=torch.int64, device=dev, generator=g)
    n = a.n_bases - k + 1
    v = torch.zeros(n, dtype=torch.int64, device=dev)
    for j in range(k):
        v = (v << 2) | bases[j:j + n]
    v &= (1 << (2 * k)) - 1
    km = torch.unique(torch.minimum(v, synth_torch.revcomp(v, k)), sorted=True)
    del v
    cnt = synth_torch.d1_counts(km.numel(), a.ci, a.cs, 2, dev)
    m = KModel(a.ci, a.cs, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.build_dev(k, km.data_ptr(), cnt.data_ptr(), km.numel())
    del km, cnt

    # reads: L-base pieces of the sequence, 1 % substitutions (bench_seq.py's)
    wpr = L - k + 1
    n_reads = max(1, a.windows // wpr)
    g.manual_seed(23)
    starts = torch.randint(0, a.n_bases - L, (n_reads,), device=dev, generator=g)
    codes = bases[starts[:, None] + torch.arange(L, device=dev)[None, :]]
    del bases
    sub = torch.rand(codes.shape, device=dev, generator=g) < 0.01
    codes = torch.where(sub, (codes + torch.randint(1, 4, codes.shape, device=dev, generator=g)) % 4, codes)
    del sub
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    d_seq = lut[codes].reshape(-1).contiguous()
    del codes
    n_bases = d_seq.numel()
    n_win = n_reads * wpr
    d_off = (torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L).contiguous()
    d_out = torch.empty(n_bases, dtype=torch.int32, device=dev)
    d_rec = torch.empty(n_reads * 64, dtype=torch.uint8, device=dev)
    seq_id = torch.repeat_interleave(torch.arange(n_reads, device=dev), L)     # leg c's segment ids: made once, like a caller would
    torch.cuda.empty_cache()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def leg_a():
        m.seq_summary_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, THR, d_rec.data_ptr())

    def leg_b():
        m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_out.data_ptr())

    def leg_c():
        leg_b()
        ok = d_out >= 0
        val = torch.where(ok, d_out, 0).to(torch.int64)
        res = [torch.zeros(n_reads, dtype=torch.int64, device=dev).index_add_(0, seq_id, val)]
        res += [torch.zeros(n_reads, dtype=torch.int64, device=dev).index_add_(0, seq_id, (d_out >= t).to(torch.int64)) for t in THR]
        res.append(torch.full((n_reads,), 2**31 - 1, dtype=torch.int32, device=dev).scatter_reduce_(0, seq_id, torch.where(ok, d_out, 2**31 - 1), "amin"))
        res.append(torch.full((n_reads,), -1, dtype=torch.int32, device=dev).scatter_reduce_(0, seq_id, d_out, "amax"))
        return res

    # identity first: a == reduce(b), d == a
    leg_b()
    leg_a()
    torch.cuda.synchronize()
    h_seq = d_seq.cpu().numpy()
    h_off = d_off.cpu().numpy().view(np.uint64)
    rec_a = d_rec.cpu().numpy().view(api.SEQ_SUMMARY_DTYPE).copy()
    want = S.summarise(d_out.cpu().numpy(), h_off, k, THR)
    agree_a = S.same(rec_a, want)
    del want
    rec_d = m.seq_summary_flat(h_seq, h_off, THR)
    agree_d = S.same(rec_d, rec_a)
    if not (agree_a and agree_d):
        print(json.dumps({"tool": "bench_seq_summary", "error": "records differ", "a_equals_reduced_b": agree_a, "d_equals_a": agree_d}), flush=True)
        sys.exit(1)
    c_res = leg_c()
    agree_c = bool(np.array_equal(c_res[0].cpu().numpy().astype(np.uint64), rec_a["sum"]) and np.array_equal(c_res[4].cpu().numpy(), rec_a["min"])
                   and np.array_equal(c_res[5].cpu().numpy(), rec_a["max"]) and np.array_equal(c_res[1].cpu().numpy().astype(np.uint64), rec_a["n_ge"][:, 0]))
    del c_res

    seg = h_off[:-1].astype(np.int64)

    def leg_d():
        return m.seq_summary_flat(h_seq, h_off, THR)

    def leg_f():
        return m.seq_to_occ_flat(h_seq, h_off)

    def leg_e():
        occ = leg_f()
        ok = occ >= 0
        res = [np.add.reduceat(np.where(ok, occ, 0).astype(np.int64), seg), np.minimum.reduceat(np.where(ok, occ, 2**31 - 1), seg), np.maximum.reduceat(occ, seg)]
        res += [np.add.reduceat((occ >= t).astype(np.int64), seg) for t in THR]
        return res

    e_res = leg_e()
    agree_e = bool(np.array_equal(e_res[0].astype(np.uint64), rec_a["sum"]) and np.array_equal(e_res[1], rec_a["min"]) and np.array_equal(e_res[2], rec_a["max"])
                   and np.array_equal(e_res[5].astype(np.uint64), rec_a["n_ge"][:, 2]))
    del e_res
    for leg in (leg_a, leg_b, leg_c, leg_d, leg_f):
        timed(leg)
    t = {x: [] for x in "abcdef"}
    for _ in range(a.reps):
        for name, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
            t[name].append(timed(leg))
    for _ in range(a.reps):
        for name, leg in (("d", leg_d), ("e", leg_e), ("f", leg_f)):
            t[name].append(timed(leg))
    rate = {x: n_win / statistics.median(t[x]) for x in t}
    lo = {x: n_win / max(t[x]) for x in t}
    hi = {x: n_win / min(t[x]) for x in t}
    out = {"tool": "bench_seq_summary", "k": k, "model_bases": a.n_bases, "read_len": L, "n_reads": n_reads, "windows": n_win, "thr": list(THR),
           "reps": a.reps, "a_equals_reduced_b": agree_a, "d_equals_a": agree_d, "c_agrees": agree_c, "e_agrees": agree_e}
    names = {"a": "a_summary_dev", "b": "b_seq_dev", "c": "c_seq_dev_torch_reduce", "d": "d_summary_host", "e": "e_seq_host_numpy_reduce", "f": "f_seq_host"}
    for x in "abcdef":
        out[names[x] + "_wps"] = rate[x]
        out[names[x] + "_wps_min_max"] = [lo[x], hi[x]]
        out[x + "_s"] = t[x]
    out["a_over_b"] = rate["a"] / rate["b"]
    out["a_not_below_b_by_more_than_b_spread"] = bool(rate["a"] >= rate["b"] - (hi["b"] - lo["b"]))
    out["d_over_f"] = rate["d"] / rate["f"]
    out["d_faster_than_f_beyond_f_spread"] = bool(rate["d"] > rate["f"] + (hi["f"] - lo["f"]))
    out["d_over_a"] = rate["d"] / rate["a"]
    out["d_over_e"] = rate["d"] / rate["e"]
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
