"""Throughput of the read editing (kmx_edit_seqs: substitutions and single-base indels) against the substitution corrector and
seq_to_occ on the same buffers; prints one JSON line.

tools/bench_seq_correct.py's model (all k-mers of a random `--n-bases` sequence); reads of `--read-len` true bases of it with
tests/seq_edit_reads.py's error draw (0.4 % substituted, 0.3 % lost, 0.3 % followed by a surplus base), about `--windows`
windows.  Legs, in input windows/s (median of `--reps`, min and max):
  a7 seq_edit_dev(ops = 7), a1 seq_edit_dev(ops = 1): bases and offsets in HBM, edit list and records out
  c  seq_correct_dev, b  seq_to_occ_dev on the same buffers
  d  seq_edit_flat, e  seq_correct_flat from host memory
Every leg is warmed up, the device is synchronised around each timed call, the device legs alternate in one loop, then the host
legs.  Before anything is timed: d == a7 (edits and records), apply_edits_dev == the host apply, and on a sample of `--sample`
reads a7 == the reference rule (tests/seq_edit_ref.py) over seq_to_occ_flat / kmer_to_occ_rows.  q = verification windows the
rule asks per input window on that sample (counted, not timed); the work count predicts a7 = b / (1 + q * 64 / k).  Of the
sample's reads with exactly one injected error, per kind: how many the edits restore to the truth and how many they change into
something else.
usage: python tools/bench_seq_edit.py [--reps 5] [--windows 100000000] [--skip-host]"""
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
import seq_edit_reads as ER  # noqa: E402
import seq_edit_ref as E  # noqa: E402
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
    ap.add_argument("--min-support", type=int, default=1)
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="device legs only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, L, thr, ms = a.k, a.read_len, a.ci, a.min_support
    assert k <= 32 and L >= 2 * k
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

    n_reads = max(1, a.windows // (L - k + 1))
    g.manual_seed(23)
    starts = torch.randint(0, a.n_bases - L, (n_reads,), device=dev, generator=g)
    truth = np.frombuffer(b"ACGT", dtype=np.uint8)[bases[starts[:, None] + torch.arange(L, device=dev)[None, :]].cpu().numpy()]   # [n_reads, L]
    del bases, starts
    rng = np.random.default_rng(23)
    u = rng.random(truth.shape)
    sub, lost = u < ER.SUB_RATE, (u >= ER.SUB_RATE) & (u < ER.SUB_RATE + ER.DROP_RATE)
    extra = (u >= ER.SUB_RATE + ER.DROP_RATE) & (u < ER.SUB_RATE + ER.DROP_RATE + ER.EXTRA_RATE)
    del u
    r = truth.copy()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    r[sub] = acgt[(np.searchsorted(acgt, r[sub]) + rng.integers(1, 4, size=int(sub.sum()))) % 4]
    pairs = np.stack([r, acgt[rng.integers(0, 4, size=r.shape)]], axis=2)
    keep = np.stack([~lost, extra], axis=2)
    h_seq = np.ascontiguousarray(pairs[keep])
    h_off = np.zeros(n_reads + 1, dtype=np.uint64)
    h_off[1:] = np.cumsum(keep.sum(axis=(1, 2)), dtype=np.uint64)
    n_err = {"sub": int(sub.sum()), "lost": int(lost.sum()), "surplus": int(extra.sum())}
    ns = min(a.sample, n_reads)
    one = (sub[:ns].sum(1) + lost[:ns].sum(1) + extra[:ns].sum(1)) == 1
    kind_of = np.where(sub[:ns].any(1), 0, np.where(lost[:ns].any(1), 1, 2))
    s_truth = truth[:ns].copy()
    del pairs, keep, r, sub, lost, extra, truth
    n_bases = len(h_seq)
    n_win = int((np.diff(h_off.astype(np.int64)) - k + 1).clip(min=0).sum())
    cap = n_bases // 3 + 1
    d_seq = torch.from_numpy(h_seq).to(dev)
    d_off = torch.from_numpy(h_off.view(np.int64)).to(dev)
    d_occ = torch.empty(n_bases, dtype=torch.int32, device=dev)
    d_fix = torch.empty(n_bases, dtype=torch.uint8, device=dev)
    d_ed = torch.empty(cap, dtype=torch.int64, device=dev)
    d_rec = torch.empty(n_reads * 80, dtype=torch.uint8, device=dev)
    torch.cuda.empty_cache()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def edit_dev(ops):
        return m.seq_edit_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, thr, ms, ops, d_ed.data_ptr(), cap, d_rec.data_ptr())

    # identity first
    n_ed = edit_dev(7)
    torch.cuda.synchronize()
    ed_a = d_ed.cpu().numpy().view(np.uint64)[:n_ed].copy()
    rec_a = d_rec.cpu().numpy().view(api.SEQ_EDITS_DTYPE).copy()
    d_out = torch.empty(n_bases + n_ed, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    m.apply_edits_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_ed.data_ptr(), n_ed, d_out.data_ptr(), n_bases + n_ed, d_oo.data_ptr())
    torch.cuda.synchronize()
    h_out, h_oo = api.apply_edits(h_seq, h_off, ed_a)
    agree_apply = bool(np.array_equal(d_out.cpu().numpy()[:len(h_out)], h_out) and np.array_equal(d_oo.cpu().numpy().view(np.uint64), h_oo))
    del d_out, d_oo
    s_off = h_off[:ns + 1]
    s_buf = h_seq[:int(s_off[-1])]
    w_ed, w_rec, nq = E.edit_seqs(m.seq_to_occ_flat(s_buf, s_off), s_buf, s_off, k, thr, ms, 7, lambda rows: m.kmer_to_occ_rows(rows, k))
    _, _, nq1 = E.edit_seqs(m.seq_to_occ_flat(s_buf, s_off), s_buf, s_off, k, thr, ms, 1, lambda rows: m.kmer_to_occ_rows(rows, k))
    agree_ref = bool(np.array_equal(w_ed, ed_a[:len(w_ed)]) and E.same(w_rec, rec_a[:ns]))
    s_win = int(w_rec["n_windows"].sum())
    q, q1 = nq / float(s_win), nq1 / float(s_win)
    fixed = [h_out[int(h_oo[i]):int(h_oo[i + 1])].tobytes() for i in range(ns)]
    reads = [s_buf[int(s_off[i]):int(s_off[i + 1])].tobytes() for i in range(ns)]
    truths = [s_truth[i].tobytes() for i in range(ns)]
    per_kind = {}
    for ki, name in enumerate(("sub", "lost", "surplus")):
        idx = np.nonzero(one & (kind_of == ki))[0]
        per_kind[name] = {"reads_with_only_this_error": len(idx), "restored": sum(fixed[i] == truths[i] for i in idx),
                          "miscorrected": sum(fixed[i] != truths[i] and fixed[i] != reads[i] for i in idx)}
    sample = {"reads": ns, "wrong_before": sum(x != t for x, t in zip(reads, truths)), "wrong_after": sum(x != t for x, t in zip(fixed, truths)),
              "right_made_wrong": sum(x == t and f != t for x, f, t in zip(reads, fixed, truths)), "single_error_reads": per_kind}
    agree_d = True
    if not a.skip_host:
        ed_d, rec_d = m.seq_edit_flat(h_seq, h_off, thr, ms, 7)
        agree_d = bool(np.array_equal(ed_d, ed_a) and E.same(rec_d, rec_a))
        del ed_d, rec_d
    if not (agree_ref and agree_d and agree_apply):
        print(json.dumps({"tool": "bench_seq_edit", "error": "results differ", "a7_equals_reference_on_sample": agree_ref, "d_equals_a7": agree_d, "apply_dev_equals_host": agree_apply}), flush=True)
        sys.exit(1)

    legs = [("a7", lambda: edit_dev(7)), ("a1", lambda: edit_dev(1)),
            ("c", lambda: m.seq_correct_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, thr, ms, d_fix.data_ptr(), d_rec.data_ptr())),
            ("b", lambda: m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_occ.data_ptr()))]
    host = [] if a.skip_host else [("d", lambda: m.seq_edit_flat(h_seq, h_off, thr, ms, 7)), ("e", lambda: m.seq_correct_flat(h_seq, h_off, thr, ms))]
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
    out = {"tool": "bench_seq_edit", "k": k, "model_bases": a.n_bases, "read_len": L, "n_reads": n_reads, "bases": n_bases, "windows": n_win, "thr": thr, "min_support": ms,
           "reps": a.reps, "errors": n_err, "a7_equals_reference_on_sample": agree_ref, "d_equals_a7": agree_d if not a.skip_host else None, "apply_dev_equals_host": agree_apply,
           "q_verify_windows_per_window": q, "q_verify_windows_per_window_ops1": q1, "sample": sample, "tallies": {f: int(rec_a[f].sum()) for f in E.FIELDS}}
    names = {"a7": "a7_edit_dev_ops7", "a1": "a1_edit_dev_ops1", "c": "c_correct_dev", "b": "b_seq_dev", "d": "d_edit_host", "e": "e_correct_host"}
    for x in t:
        out[names[x] + "_wps"] = rate[x]
        out[names[x] + "_wps_min_max"] = [n_win / max(t[x]), n_win / min(t[x])]
        out[x + "_s"] = t[x]
    out["a7_over_b"] = rate["a7"] / rate["b"]
    out["a7_expected_over_b"] = 1.0 / (1.0 + q * 64.0 / k)
    out["a7_more_than_a_tenth_below_expectation"] = bool(out["a7_over_b"] < 0.9 * out["a7_expected_over_b"])
    out["a1_over_c"] = rate["a1"] / rate["c"]
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
