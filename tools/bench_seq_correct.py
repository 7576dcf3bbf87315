"""Throughput of the read correction (kmx_correct_seqs) against seq_to_occ on the same buffers; prints one JSON line.

tools/bench_seq.py's input: the model of all k-mers of a random 10^8-base sequence, reads of `--read-len` bases of it with
`--sub-rate` substitutions (default 1 %), about 10^8 windows.  Legs, in input windows/s (median of `--reps`, min and max):
  a  seq_correct_dev: bases and offsets in HBM, corrected bases and records out  (kernel rate from HBM)
  b  seq_to_occ_dev on the same buffers: 4 bytes per base out                    (kernel rate from HBM)
  d  seq_correct_flat from host memory                                           (end-to-end rate from host memory)
  f  seq_to_occ_flat from host memory                                            (end-to-end rate from host memory)
Every leg is warmed up, the device is synchronised around each timed call, a / b and d / f alternate in one loop.  Before
anything is timed: d == a (bases and records), and on a sample of 10^4 reads a == the reference rule
(tests/seq_correct_ref.py) over seq_to_occ_flat / kmer_to_occ_rows.  q = verification windows the rule asks per input window
on that sample (counted, not timed); the expectation for one candidate per wave pass is a = b / (1 + q * 64 / k).
usage: python tools/bench_seq_correct.py [--reps 5] [--sub-rate 0.01] [--min-support 1] [--skip-host]"""
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
import seq_correct_ref as S  # noqa: E402
from kmcex_amd import KModel, api, synth_torch  # noqa: E402


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
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--min-support", type=int, default=1)
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="legs a and b only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, L, thr, ms = a.k, a.read_len, a.ci, a.min_support
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

    wpr = L - k + 1
    n_reads = max(1, a.windows // wpr)
    g.manual_seed(23)
    starts = torch.randint(0, a.n_bases - L, (n_reads,), device=dev, generator=g)
    codes = bases[starts[:, None] + torch.arange(L, device=dev)[None, :]]
    del bases
    truth = codes.to(torch.uint8)
    sub = torch.rand(codes.shape, device=dev, generator=g) < a.sub_rate
    codes = torch.where(sub, (codes + torch.randint(1, 4, codes.shape, device=dev, generator=g)) % 4, codes)
    n_errors = int(sub.sum().item())
    del sub
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    d_seq = lut[codes].reshape(-1).contiguous()
    d_truth = lut[truth.to(torch.int64)].reshape(-1).contiguous()
    del codes, truth
    n_bases = d_seq.numel()
    n_win = n_reads * wpr
    d_off = (torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L).contiguous()
    d_occ = torch.empty(n_bases, dtype=torch.int32, device=dev)
    d_fix = torch.empty(n_bases, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(n_reads * 64, dtype=torch.uint8, device=dev)
    torch.cuda.empty_cache()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def leg_a():
        m.seq_correct_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, thr, ms, d_fix.data_ptr(), d_rec.data_ptr())

    def leg_b():
        m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_occ.data_ptr())

    # identity first
    leg_a()
    torch.cuda.synchronize()
    restored = int(((d_seq != d_truth) & (d_fix == d_truth)).sum().item())
    miscorrected = int(((d_fix != d_seq) & (d_fix != d_truth)).sum().item())
    del d_truth
    h_seq = d_seq.cpu().numpy()
    h_off = d_off.cpu().numpy().view(np.uint64)
    fix_a = d_fix.cpu().numpy()
    rec_a = d_rec.cpu().numpy().view(api.SEQ_CORRECTION_DTYPE).copy()
    ns = min(a.sample, n_reads)
    s_off = h_off[:ns + 1]
    s_buf = h_seq[:int(s_off[-1])]
    w_out, w_rec, nq = S.correct(m.seq_to_occ_flat(s_buf, s_off), s_buf, s_off, k, thr, ms, lambda rows: m.kmer_to_occ_rows(rows, k))
    agree_ref = bool(np.array_equal(w_out, fix_a[:len(w_out)]) and S.same(w_rec, rec_a[:ns]))
    q = nq / float(ns * wpr)
    agree_d = True
    if not a.skip_host:
        fix_d, rec_d = m.seq_correct_flat(h_seq, h_off, thr, ms)
        agree_d = bool(np.array_equal(fix_d, fix_a) and S.same(rec_d, rec_a))
        del fix_d, rec_d
    if not (agree_ref and agree_d):
        print(json.dumps({"tool": "bench_seq_correct", "error": "results differ", "a_equals_reference_on_sample": agree_ref, "d_equals_a": agree_d}), flush=True)
        sys.exit(1)

    legs = [("a", leg_a), ("b", leg_b)]
    host = [] if a.skip_host else [("d", lambda: m.seq_correct_flat(h_seq, h_off, thr, ms)), ("f", lambda: m.seq_to_occ_flat(h_seq, h_off))]
    for _, leg in legs + host:
        timed(leg)
    t = {x: [] for x, _ in legs + host}
    for _ in range(a.reps):
        for name, leg in legs:
            t[name].append(timed(leg))
    for _ in range(a.reps):
        for name, leg in host:
            t[name].append(timed(leg))
    rate = {x: n_win / statistics.median(t[x]) for x in t}
    lo = {x: n_win / max(t[x]) for x in t}
    hi = {x: n_win / min(t[x]) for x in t}
    out = {"tool": "bench_seq_correct", "k": k, "model_bases": a.n_bases, "read_len": L, "n_reads": n_reads, "windows": n_win, "sub_rate": a.sub_rate, "thr": thr,
           "min_support": ms, "reps": a.reps, "a_equals_reference_on_sample": agree_ref, "sample_reads": ns, "d_equals_a": agree_d if not a.skip_host else None,
           "q_verify_windows_per_window": q, "errors": n_errors, "restored": restored, "miscorrected": miscorrected,
           "tallies": {f: int(rec_a[f].sum()) for f in S.FIELDS}}
    names = {"a": "a_correct_dev", "b": "b_seq_dev", "d": "d_correct_host", "f": "f_seq_host"}
    for x in t:
        out[names[x] + "_wps"] = rate[x]
        out[names[x] + "_wps_min_max"] = [lo[x], hi[x]]
        out[x + "_s"] = t[x]
    out["a_over_b"] = rate["a"] / rate["b"]
    out["a_expected_over_b"] = 1.0 / (1.0 + q * 64.0 / k)
    out["a_below_expectation_by_more_than_b_spread"] = bool(rate["a"] < rate["b"] * out["a_expected_over_b"] - (hi["b"] - lo["b"]))
    if not a.skip_host:
        out["d_over_f"] = rate["d"] / rate["f"]
        out["d_over_a"] = rate["d"] / rate["a"]
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
