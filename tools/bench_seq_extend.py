"""Throughput of the path extension (kmx_extend_seqs) against the same rule driven from the host; prints one JSON line.

Input: the model of all k-mers of a random 10^8-base sequence (k = 31), `--seeds` k-mers cut from it (10^6), thr = ci,
depth 2, max_ext 1000.  Legs, in appended bases/s (median of `--reps`, min and max):
  a  seq_extend_dev: seeds and offsets in HBM, rows and records out               (the feature, from HBM)
  d  seq_extend_flat from host memory                                            (the feature, end to end)
  i  the same rule with torch on the device: one kmx_query_packed_dev launch per step (and per lookahead level) over the
     compacted live walks -- what a caller could do before this entry point existed
  ii query_packed_dev's k-mers/s on the neighbours of genome k-mers, divided by the queries the rule asks per appended
     base: the rate of a walk whose every query hid its latency (a ceiling, not a leg)
Every leg is warmed up, the device is synchronised around each timed call, a and i alternate in one loop.  Before anything
is timed: d == a and i == a on the whole input (rows and records), and a == the reference rule (tests/seq_extend_ref.py)
over kmer_to_occ_rows on the first `--sample` seeds.
usage: python tools/bench_seq_extend.py [--reps 5] [--seeds 1000000] [--max-ext 1000] [--depth 2] [--skip-host]"""
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
import seq_extend_ref as X  # noqa: E402
from kmcex_amd import KModel, api, synth_torch  # noqa: E402


class HostDriven:
    """yardstick (i): the rule of include/kmx.h in torch over packed k-mers (k <= 31), every query through kmer_to_occ_dev"""

    def __init__(self, m, k, thr, max_ext, depth, dev):
        self.m, self.k, self.thr, self.max_ext, self.depth, self.dev = m, k, thr, max_ext, depth, dev
        self.mask, self.top = (1 << (2 * k)) - 1, 2 * (k - 1)
        self.four = torch.arange(4, dtype=torch.int64, device=dev)
        self.lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        self.asked = 0

    def ask(self, q):
        q = q.reshape(-1).contiguous()
        out = torch.empty(q.numel(), dtype=torch.int32, device=self.dev)
        self.m.kmer_to_occ_dev(q.data_ptr(), q.numel(), out.data_ptr())
        self.asked += q.numel()
        return out

    def children(self, x, fwd):
        if fwd:
            return ((x[:, None] << 2) | self.four[None, :]) & self.mask
        return (x[:, None] >> 2) | (self.four[None, :] << self.top)

    def sup(self, x, d, fwd):
        ch = self.children(x, fwd)
        solid = (self.ask(ch) >= self.thr).view(-1, 4)
        if d == 1:
            return solid.any(1)
        idx = solid.nonzero(as_tuple=True)
        ok = torch.zeros_like(solid)
        if idx[0].numel():
            ok[idx] = self.sup(ch[idx], d - 1, fwd)
        return ok.any(1)

    def run(self, seeds):
        """seeds: packed k-mers (int64) -> (ext uint8 [n, max_ext], dict of record fields), all on the device"""
        n, dev = seeds.numel(), self.dev
        ext = torch.zeros((n, self.max_ext), dtype=torch.uint8, device=dev)
        r = {f: torch.zeros(n, dtype=torch.int64, device=dev) for f in X.FIELDS}
        r["min_occ"] -= 1
        r["max_occ"] -= 1
        r["seed_occ"] = self.ask(seeds).to(torch.int64)
        live, cur, first = torch.arange(n, device=dev), seeds.clone(), seeds.clone()
        while live.numel():
            succ = self.children(cur, True)
            pred = (cur & ((1 << self.top) - 1))[:, None] | (self.four[None, :] << self.top)
            a = self.ask(torch.cat([succ, pred], 1)).view(-1, 8)
            S = a[:, :4] >= self.thr
            P = (a[:, 4:] >= self.thr) & (self.four[None, :] != (cur >> self.top)[:, None])
            looked = torch.zeros_like(live, dtype=torch.bool)
            if self.depth > 0:
                tie = S.sum(1) > 1
                looked = tie | P.any(1)
                idx = (S & tie[:, None]).nonzero(as_tuple=True)
                if idx[0].numel():
                    S[idx] = self.sup(succ[idx], self.depth, True)
                idx = P.nonzero(as_tuple=True)
                if idx[0].numel():
                    P[idx] = self.sup(pred[idx], self.depth, False)
            ns = S.sum(1)
            stop = torch.where(ns == 0, X.DEAD_END, torch.where(ns > 1, X.BRANCH, torch.where(P.any(1), X.JOIN, 0)))
            c = S.to(torch.uint8).argmax(1)
            nxt = succ.gather(1, c[:, None]).squeeze(1)
            stop = torch.where((stop == 0) & (nxt == first), X.CYCLE, stop)
            go = stop == 0
            ids = live[go]
            a_c = a[:, :4].gather(1, c[:, None]).squeeze(1)[go].to(torch.int64)
            ne = r["n_ext"][ids]
            ext[ids, ne] = self.lut[c[go]]
            r["min_occ"][ids] = torch.where(ne == 0, a_c, torch.minimum(r["min_occ"][ids], a_c))
            r["max_occ"][ids] = torch.where(ne == 0, a_c, torch.maximum(r["max_occ"][ids], a_c))
            r["sum_occ"][ids] += a_c
            r["n_lookahead"][ids] += looked[go].to(torch.int64)
            r["n_ext"][ids] = ne + 1
            stop[go] = torch.where(ne + 1 == self.max_ext, X.MAX_EXT, 0)
            done = stop != 0
            r["stop"][live[done]] = stop[done]
            keep = ~done
            live, cur, first = live[keep], nxt[keep], first[keep]
        return ext, r


def records_of(r):
    rec = np.zeros(r["n_ext"].numel(), dtype=api.SEQ_EXTENSION_DTYPE)
    for f in X.FIELDS:
        rec[f] = r[f].cpu().numpy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--ci", type=int, default=1)
    ap.add_argument("--cs", type=int, default=1023)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    ap.add_argument("--n-bases", type=int, default=100_000_000)
    ap.add_argument("--seeds", type=int, default=1_000_000)
    ap.add_argument("--max-ext", type=int, default=1000)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="no leg d")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    k, thr, max_ext, depth, n = a.k, a.ci, a.max_ext, a.depth, a.seeds
    assert k <= 31
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bases = torch.randint(0, 4, (a.n_bases,), dtype=torch.int64, device=dev, generator=g)
    nk = a.n_bases - k + 1
    v = torch.zeros(nk, dtype=torch.int64, device=dev)
    for j in range(k):
        v = (v << 2) | bases[j:j + nk]
    km = torch.unique(torch.minimum(v, synth_torch.revcomp(v, k)), sorted=True)
    cnt = synth_torch.d1_counts(km.numel(), a.ci, a.cs, 2, dev)
    m = KModel(a.ci, a.cs, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.build_dev(k, km.data_ptr(), cnt.data_ptr(), km.numel())
    del km, cnt
    g.manual_seed(29)
    starts = torch.randint(0, a.n_bases - k - max_ext, (n,), device=dev, generator=g)
    seeds = v[starts].contiguous()
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    d_seq = lut[bases[starts[:, None] + torch.arange(k, device=dev)[None, :]]].reshape(-1).contiguous()
    d_off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * k).contiguous()
    # yardstick (ii)'s queries: the 8 neighbours of genome k-mers, the mix of present and absent k-mers a walk asks about
    s = v[torch.randint(0, nk, (5_000_000,), device=dev, generator=g)]
    four = torch.arange(4, dtype=torch.int64, device=dev)
    q_nb = torch.cat([((s[:, None] << 2) | four[None, :]) & ((1 << (2 * k)) - 1), (s[:, None] & ((1 << (2 * k - 2)) - 1)) | (four[None, :] << (2 * k - 2))], 1).reshape(-1).contiguous()
    d_occ = torch.empty(q_nb.numel(), dtype=torch.int32, device=dev)
    del v, bases, s
    d_ext = torch.empty(n * max_ext, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    torch.cuda.empty_cache()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def leg_a():
        m.seq_extend_dev(d_seq.data_ptr(), d_off.data_ptr(), n, n * k, thr, max_ext, depth, d_ext.data_ptr(), d_rec.data_ptr())

    hd = HostDriven(m, k, thr, max_ext, depth, dev)

    # identity first
    leg_a()
    torch.cuda.synchronize()
    ext_a = d_ext.cpu().numpy().reshape(n, max_ext)
    rec_a = d_rec.cpu().numpy().view(api.SEQ_EXTENSION_DTYPE).copy()
    h_seq, h_off = d_seq.cpu().numpy(), d_off.cpu().numpy().view(np.uint64)
    ns = min(a.sample, n)
    w_ext, w_rec, nq = X.extend(h_seq[:ns * k], h_off[:ns + 1], k, thr, max_ext, depth, lambda rows: m.kmer_to_occ_rows(rows, k, separate=False))
    agree_ref = bool(np.array_equal(w_ext, ext_a[:ns]) and X.same(w_rec, rec_a[:ns]))
    ext_i, r_i = hd.run(seeds)
    agree_i = bool(np.array_equal(ext_i.cpu().numpy(), ext_a) and X.same(records_of(r_i), rec_a))
    appended = int(rec_a["n_ext"].sum())
    q_per_base = (hd.asked - n) / float(appended)                  # (without the n seed_occ queries)
    del ext_i, r_i
    agree_d = True
    if not a.skip_host:
        ext_d, rec_d = m.seq_extend_flat(h_seq, h_off, thr, max_ext, depth)
        agree_d = bool(np.array_equal(ext_d, ext_a) and X.same(rec_d, rec_a))
        del ext_d, rec_d
    if not (agree_ref and agree_i and agree_d):
        print(json.dumps({"tool": "bench_seq_extend", "error": "results differ", "a_equals_reference_on_sample": agree_ref, "i_equals_a": agree_i, "d_equals_a": agree_d}), flush=True)
        sys.exit(1)

    legs = [("a", leg_a), ("i", lambda: hd.run(seeds))]
    host = [] if a.skip_host else [("d", lambda: m.seq_extend_flat(h_seq, h_off, thr, max_ext, depth))]
    query = [("q", lambda: m.kmer_to_occ_dev(q_nb.data_ptr(), q_nb.numel(), d_occ.data_ptr()))]
    for _, leg in legs + host + query:
        timed(leg)
    t = {x: [] for x, _ in legs + host + query}
    for _ in range(a.reps):
        for name, leg in legs + query:
            t[name].append(timed(leg))
    for _ in range(a.reps):
        for name, leg in host:
            t[name].append(timed(leg))
    work = {x: (q_nb.numel() if x == "q" else appended) for x in t}
    rate = {x: work[x] / statistics.median(t[x]) for x in t}
    lo = {x: work[x] / max(t[x]) for x in t}
    hi = {x: work[x] / min(t[x]) for x in t}
    out = {"tool": "bench_seq_extend", "k": k, "model_bases": a.n_bases, "seeds": n, "thr": thr, "depth": depth, "max_ext": max_ext, "reps": a.reps,
           "a_equals_reference_on_sample": agree_ref, "sample_seeds": ns, "i_equals_a": agree_i, "d_equals_a": agree_d if not a.skip_host else None,
           "appended_bases": appended, "queries_per_appended_base": q_per_base, "sample_rows_asked_per_appended_base": (nq - ns) / float(max(int(w_rec["n_ext"].sum()), 1)),
           "tallies": X.tallies(rec_a)}
    names = {"a": "a_extend_dev_bases_per_s", "i": "i_host_driven_bases_per_s", "d": "d_extend_host_bases_per_s", "q": "query_packed_dev_kmers_per_s"}
    for x in t:
        out[names[x]] = rate[x]
        out[names[x] + "_min_max"] = [lo[x], hi[x]]
        out[x + "_s"] = t[x]
    out["ii_ceiling_bases_per_s"] = rate["q"] / q_per_base
    out["a_over_i"] = rate["a"] / rate["i"]
    out["a_beats_i_beyond_spreads"] = bool(lo["a"] > hi["i"])
    out["a_fraction_of_ii"] = rate["a"] / out["ii_ceiling_bases_per_s"]
    if not a.skip_host:
        out["d_over_a"] = rate["d"] / rate["a"]
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
