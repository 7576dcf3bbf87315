"""Throughput of the sequence query (kmx_query_seqs) against today's ways of asking the same thing; prints one JSON line.

The model is bench.py's genome leg construction (all k-mers of a random 10^8-base sequence, built on the device); the
reads are `--read-len`-base pieces of that sequence with 1 % substitutions, about 10^8 windows in all.  Legs, in windows/s:
  a  seq_to_occ_dev: the bases on the device, windows built there (k_query_seq + k_query_ascii_at)
  b  the same windows pre-packed, through kmx_query_packed_dev (k_query): the baseline
  c  the host seq_to_occ_flat (bases streamed through pinned slots)
  d  kmx_query_strings over the extracted window strings (the workaround before kmx_query_seqs)
Every leg is warmed up, the device is synchronised around each timed call, a and b alternate in one loop, the median of
`--reps` runs is reported.  usage: python tools/bench_seq.py [--reps 5] [--n-bases 100000000] [--windows 100000000]"""
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
from kmcex_amd import KModel, synth_torch  # noqa: E402


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
    ap.add_argument("--skip-host", action="store_true", help="legs a and b only")
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

    # reads: L-base pieces of the sequence, 1 % substitutions
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
    n_bases = d_seq.numel()
    d_off = (torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L).contiguous()
    packed = torch.zeros((n_reads, wpr), dtype=torch.int64, device=dev)    # leg b's input: the valid windows, packed
    for j in range(k):
        packed = (packed << 2) | codes[:, j:j + wpr]
    del codes
    packed = packed.reshape(-1).contiguous()
    n_win = packed.numel()
    d_out = torch.empty(n_bases, dtype=torch.int32, device=dev)
    p_out = torch.empty(n_win, dtype=torch.int32, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    leg_a = lambda: m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_out.data_ptr())   # noqa: E731
    leg_b = lambda: m.kmer_to_occ_dev(packed.data_ptr(), n_win, p_out.data_ptr())                               # noqa: E731
    timed(leg_a)
    timed(leg_b)
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(timed(leg_a))
        tb.append(timed(leg_b))
    res_a = d_out.reshape(n_reads, L)[:, :wpr].reshape(-1)
    agree_ab = bool(torch.equal(res_a, p_out))
    tails_ok = bool((d_out.reshape(n_reads, L)[:, wpr:] == -1).all().item())
    out = {"tool": "bench_seq", "k": k, "model_bases": a.n_bases, "read_len": L, "n_reads": n_reads, "windows": n_win,
           "reps": a.reps, "a_seq_dev_wps": n_win / statistics.median(ta), "b_packed_dev_wps": n_win / statistics.median(tb),
           "a_over_b": statistics.median(tb) / statistics.median(ta), "a_s": ta, "b_s": tb, "agree_ab": agree_ab and tails_ok,
           "nonzero": float((p_out != 0).float().mean().item())}
    if not a.skip_host:
        h_seq = d_seq.cpu().numpy()
        h_off = d_off.cpu().numpy().view(np.uint64)
        ref = p_out.cpu().numpy()
        del packed, p_out, d_out
        torch.cuda.empty_cache()
        leg_c = lambda: m.seq_to_occ_flat(h_seq, h_off)                   # noqa: E731
        got_c = leg_c()
        tc = [timed(leg_c) for _ in range(a.reps)]
        rows = np.lib.stride_tricks.sliding_window_view(h_seq.reshape(n_reads, L), k, axis=1).reshape(-1, k)
        rows = np.ascontiguousarray(rows)                                     # the window strings a caller would have cut
        leg_d = lambda: m.kmer_to_occ_rows(rows, k, separate=True)            # noqa: E731
        got_d = leg_d()
        td = [timed(leg_d) for _ in range(a.reps)]
        out.update({"c_seq_host_wps": n_win / statistics.median(tc), "d_strings_host_wps": n_win / statistics.median(td),
                    "c_over_d": statistics.median(td) / statistics.median(tc), "c_s": tc, "d_s": td,
                    "agree_cd": bool(np.array_equal(got_c.reshape(n_reads, L)[:, :wpr].reshape(-1), ref) and np.array_equal(got_d, ref))})
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
