"""Throughput of polishing reads to a fixed point on the device (kmx_polish_seqs_dev) against the loop it replaces: seq_edit_dev +
apply_edits_dev over the WHOLE batch, repeated until a pass returns an empty list; prints one JSON line.

tools/bench_seq_edit.py's workload: the model of all k-mers of a random `--n-bases` sequence; reads of `--read-len` true bases
of it with tests/seq_edit_reads.py's error draw (0.4 % substituted, 0.3 % lost, 0.3 % followed by a surplus base), about
`--windows` windows, in device buffers.  Legs, in INPUT windows/s (median of `--reps`, min and max):
  p8 polish_dev(max_passes)         l8 the loop of seq_edit_dev + apply_edits_dev until a pass is empty
  p1 polish_dev(max_passes = 1)     l1 one seq_edit_dev + apply_edits_dev
  hp seq_polish_flat                hl the same loop through seq_edit_flat + apply_edits (host memory)
Every leg is warmed up, the device is synchronised around each timed call, and the legs of a pair alternate in one loop.
Before anything is timed: p8 == l8 (reads and offsets, compared on the device) and, on a sample of `--sample` reads, the
records == the reference loop (tests/seq_polish_ref.py) over seq_edit_flat.  From the untimed loop: the reads and windows
each pass examines once reads retire, and the sample's reads that differ from their truth after each pass.  The work count
predicts p8 = l8 * (passes * all windows) / (sum of the active windows).
usage: python tools/bench_seq_polish.py [--reps 5] [--windows 100000000] [--skip-host]"""
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
import seq_polish_ref as P  # noqa: E402
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
    ap.add_argument("--max-passes", type=int, default=8)
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="device legs only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, L, thr, ms, mp = a.k, a.read_len, a.ci, a.min_support, a.max_passes
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
    ns = min(a.sample, n_reads)
    truths = [truth[i].tobytes() for i in range(ns)]
    del pairs, keep, r, sub, lost, extra, truth
    n_bases = len(h_seq)
    n_win = int((np.diff(h_off.astype(np.int64)) - k + 1).clip(min=0).sum())
    room = n_bases + n_bases // 16 + 64                            # of every buffer that holds edited reads
    cap = room // 3 + 1
    d_seq = torch.from_numpy(h_seq).to(dev)
    d_off = torch.from_numpy(h_off.view(np.int64)).to(dev)
    d_ed = torch.empty(cap, dtype=torch.int64, device=dev)
    d_rec = torch.empty(n_reads * 80, dtype=torch.uint8, device=dev)
    d_prec = torch.empty(n_reads * 96, dtype=torch.uint8, device=dev)
    d_x = [torch.empty(room, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_xo = [torch.empty(n_reads + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    d_out = torch.empty(room, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    torch.cuda.empty_cache()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def polish(passes):
        return m.seq_polish_dev(d_seq.data_ptr(), d_off.data_ptr(), n_reads, n_bases, thr, ms, 7, passes, d_out.data_ptr(), room, d_oo.data_ptr(), d_prec.data_ptr())

    def loop(passes, watch=None):
        """-> (index of the buffer that holds the result or -1 for the input, its length, passes run)"""
        seq, off, nb, cur = d_seq, d_off, n_bases, -1
        for p in range(1, passes + 1):
            n_ed = m.seq_edit_dev(seq.data_ptr(), off.data_ptr(), n_reads, nb, thr, ms, 7, d_ed.data_ptr(), cap, d_rec.data_ptr())
            if watch:
                watch(p, seq, off, nb, n_ed)
            if not n_ed:
                return cur, nb, p
            nxt = (cur + 1) % 2 if cur >= 0 else 0
            m.apply_edits_dev(seq.data_ptr(), off.data_ptr(), n_reads, nb, d_ed.data_ptr(), n_ed, d_x[nxt].data_ptr(), room, d_xo[nxt].data_ptr())
            seq, off, cur = d_x[nxt], d_xo[nxt], nxt
            torch.cuda.synchronize()
            nb = int(off[-1].item())
        return cur, nb, passes

    # ---- identity and the per-pass figures first (untimed)
    per_pass, wrong_after = [], []
    active = torch.ones(n_reads, dtype=torch.bool, device=dev)

    def watch(p, seq, off, nb, n_ed):
        nonlocal active
        torch.cuda.synchronize()
        lens = off[1:] - off[:-1]
        rec = d_rec.view(torch.int64).view(n_reads, 10)
        edited = (rec[:, 4] + rec[:, 5] + rec[:, 6]) > 0
        per_pass.append({"pass": p, "active_reads": int(active.sum().item()), "active_windows": int((lens - k + 1).clamp(min=0)[active].sum().item()),
                         "edited_reads": int(edited.sum().item()), "edits": int(n_ed)})
        assert not bool((edited & ~active).any().item()), "a retired read was edited"
        active = edited
        so = off[:ns + 1].cpu().numpy()
        sb = seq[:int(so[-1])].cpu().numpy()
        wrong_after.append(sum(sb[int(so[i]):int(so[i + 1])].tobytes() != truths[i] for i in range(ns)))

    cur, nb, l_passes = loop(mp, watch)
    # (pass p's figure is taken BEFORE its edits are applied: wrong_after[p] is the state after pass p - 1)
    wrong = {"before": wrong_after[0], "after_pass": wrong_after[1:]}
    p_passes = polish(mp)
    torch.cuda.synchronize()
    l_seq, l_off = (d_seq, d_off) if cur < 0 else (d_x[cur], d_xo[cur])
    agree_loop = bool(p_passes == l_passes and torch.equal(d_oo, l_off) and int(d_oo[-1].item()) == nb and torch.equal(d_out[:nb], l_seq[:nb]))
    s_off = h_off[:ns + 1]
    s_buf = h_seq[:int(s_off[-1])]
    ref = P.polish(lambda b, o: m.seq_edit_flat(b, o, thr, ms, 7), s_buf, s_off, mp)
    prec = d_prec.cpu().numpy().view(api.SEQ_POLISH_DTYPE)
    so = d_oo[:ns + 1].cpu().numpy().view(np.uint64)
    agree_ref = bool(E.same(prec[:ns], ref["records"]) and np.array_equal(so, ref["offsets"]) and np.array_equal(d_out[:int(so[-1])].cpu().numpy(), ref["bases"]))
    if len(wrong["after_pass"]) < l_passes:                        # the loop ended at max_passes with edits: the state after its last pass
        wrong["after_pass"].append(P.wrong([ref["bases"][int(so[i]):int(so[i + 1])].tobytes() for i in range(ns)], truths))
    tall = {f: int(prec[f].sum()) for f in P.FIELDS}
    tall["not_converged"] = int((prec["converged"] == 0).sum())
    agree_host = True
    if not a.skip_host:
        hb, ho, hr, hp = m.seq_polish_flat(h_seq, h_off, thr, ms, 7, mp)
        agree_host = bool(hp == p_passes and np.array_equal(ho, d_oo.cpu().numpy().view(np.uint64)) and E.same(hr, prec) and np.array_equal(hb, d_out[:len(hb)].cpu().numpy()))
        del hb, ho, hr
    if not (agree_loop and agree_ref and agree_host):
        print(json.dumps({"tool": "bench_seq_polish", "error": "results differ", "p8_equals_loop": agree_loop, "records_equal_reference_on_sample": agree_ref,
                          "host_equals_dev": agree_host}), flush=True)
        sys.exit(1)

    def host_loop():
        x, o = h_seq, h_off
        for _ in range(mp):
            ed, _ = m.seq_edit_flat(x, o, thr, ms, 7)
            if not len(ed):
                break
            x, o = api.apply_edits(x, o, ed)

    pairs_dev = [("p8", lambda: polish(mp)), ("l8", lambda: loop(mp)), ("p1", lambda: polish(1)), ("l1", lambda: loop(1))]
    pairs_host = [] if a.skip_host else [("hp", lambda: m.seq_polish_flat(h_seq, h_off, thr, ms, 7, mp)), ("hl", host_loop)]
    for _, leg in pairs_dev + pairs_host:
        timed(leg)
    t = {x: [] for x, _ in pairs_dev + pairs_host}
    for group in (pairs_dev[:2], pairs_dev[2:], pairs_host):
        for _ in range(a.reps):
            for name, leg in group:
                t[name].append(timed(leg))
    med = {x: statistics.median(t[x]) for x in t}
    spread = {x: max(t[x]) - min(t[x]) for x in t}
    sum_active = sum(p["active_windows"] for p in per_pass)
    out = {"tool": "bench_seq_polish", "k": k, "model_bases": a.n_bases, "read_len": L, "n_reads": n_reads, "bases": n_bases, "windows": n_win, "thr": thr, "min_support": ms,
           "max_passes": mp, "reps": a.reps, "passes_run": p_passes, "per_pass": per_pass, "sample_reads": ns, "sample_reads_wrong": wrong, "tallies": tall,
           "p8_equals_loop": agree_loop, "records_equal_reference_on_sample": agree_ref, "host_equals_dev": agree_host if not a.skip_host else None}
    names = {"p8": "p8_polish_dev", "l8": "l8_loop_dev", "p1": "p1_polish_dev_one_pass", "l1": "l1_edit_apply_dev", "hp": "hp_polish_host", "hl": "hl_loop_host"}
    for x in t:
        out[names[x] + "_wps"] = n_win / med[x]
        out[names[x] + "_wps_min_max"] = [n_win / max(t[x]), n_win / min(t[x])]
        out[x + "_s"] = t[x]
    out["p8_over_l8"] = med["l8"] / med["p8"]
    out["p8_over_l8_predicted_by_work_count"] = l_passes * n_win / float(sum_active)
    out["l8_spread_s"] = spread["l8"]
    out["p8_beats_l8_by_more_than_its_spread"] = bool(med["l8"] - med["p8"] > spread["l8"])
    out["p8_short_of_prediction_by_more_than_the_spread"] = bool(med["p8"] - med["l8"] / out["p8_over_l8_predicted_by_work_count"] > spread["l8"])
    out["p1_over_l1"] = med["l1"] / med["p1"]
    out["l1_spread_s"] = spread["l1"]
    out["p1_within_the_spread_of_l1"] = bool(abs(med["p1"] - med["l1"]) <= spread["l1"])
    if not a.skip_host:
        out["hp_over_hl"] = med["hl"] / med["hp"]
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
