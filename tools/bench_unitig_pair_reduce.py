"""Cost and effect of dropping the pair links that skip a unitig (kmx_unitig_pair_reduce_dev) beside the scaffold call; prints one
JSON line.

The input is tools/bench_unitig_scaffold.py's: paired reads (fragments of 400 +- 40 bases, mates of 150, 1 % substitutions) at
`--coverage`x over a genome of `--genome` bases, counted at k = 31 on the device, mapped, walked and paired on
count_unitig_graph_clean(thr = 3) of that session.  The reduce call takes those unitig offsets and that list at the scaffolds'
min_pairs and inner (the floor of the mean d of the pairs on one unitig), tol = k and max_row = 64.  First the check: on pairs made
the same way over a genome of `--slice` bases, the device form equals the plain-Python restatement of the rule
(tests/unitig_pair_reduce_ref.py) on the library's unitigs and list.  Then, warmed, the median of 5 calls with [min, max], run in
turn on the same device buffers: kmx_unitig_pair_reduce_dev and kmx_unitig_scaffold_dev on the same (full) list, and their ratio;
the seconds per phase of one reduce call under the profile; the verdict counts and the rows enumerated; and, for the scaffolds of
the full and of the reduced list, the chain links, the scaffolds, the N written and the N50.  Not measured: the host form, the
10^8-base size, other tol and max_row, the kernels one by one.
usage: python tools/bench_unitig_pair_reduce.py [--genome 3000000] [--coverage 10] [--slice 20000] [--min-pairs 2] [--ratio 4]"""
import argparse
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
from bench_unitig_contigs import n50  # noqa: E402
from bench_unitig_map import med, timed  # noqa: E402
from bench_unitig_pairs import K, PARAMS, THR, make_pairs  # noqa: E402
from bench_unitig_scaffold import paired, scaffold  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import PAIR_LINK_DTYPE, PAIR_REDUCE_DTYPE  # noqa: E402

MAX_ROW = 64


def reduce(m, a, uoff, n_ub, d_pl, n_pl, inner, out=None):
    """kmx_unitig_pair_reduce_dev at the scaffolds' min_pairs and inner, tol = k -> (out, n_out, stats)"""
    return m.unitig_pair_reduce_dev(K, uoff, n_ub, d_pl, n_pl, inner, K, a.min_pairs, MAX_ROW, out=out)


def slice_check(a):
    """the device form against the restatement on the library's unitigs and list of a small genome -> bool"""
    import unitig_pair_reduce_ref as X
    sb, sn = make_pairs(a.slice, a.coverage, seed=6)
    m = KModel(1, 65535, a.nh, a.nb)
    _, ubuf, uoff, _, _, _, _, d_pl, n_pl, inner, _ = paired(m, sb, sn)
    (d_rec, d_lout, d_org), n_out, st = reduce(m, a, uoff, int(ubuf.numel()), d_pl, n_pl, inner)
    torch.cuda.synchronize()
    off = uoff.cpu().numpy()
    mu = [max(int(off[i + 1] - off[i]) - K + 1, 0) for i in range(len(off) - 1)]
    plinks = [tuple(int(x) for x in e) for e in d_pl.cpu().numpy()[:n_pl].reshape(-1).view(PAIR_LINK_DTYPE)]
    want = X.flat(X.reduce(mu, plinks, a.min_pairs, inner, K, MAX_ROW))
    got = (d_rec.cpu().numpy()[:n_pl], d_lout.cpu().numpy()[:n_out], d_org.cpu().numpy()[:n_out])
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want[:3])) and n_out == want[3] and [st[f] for f in X.STAT_FIELDS] == list(want[4])


def scaffold_summary(out, ns, st, ulen):
    slen = np.diff(out[1].cpu().numpy()[:ns + 1])
    gaps = int(out[2].cpu().numpy()[:ns].reshape(-1).view(np.uint64).reshape(-1, 8)[:, 5].sum())
    return {"entries": st["n_entries"], "kept": st["n_kept"], "chain_links": st["n_chain"], "scaffolds": ns, "n_multi": st["n_multi"], "gap_bases": gaps, "n50": n50(slen),
            "longest": int(slen.max()) if ns else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reduced list is checked against the Python restatement")
    ap.add_argument("--min-pairs", type=int, default=2, dest="min_pairs")
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_pairs(int(a.genome), a.coverage)
    res = {"metric": "unitig_pair_reduce", "k": K, "thr": THR, "min_pairs": a.min_pairs, "ratio": a.ratio, "tol": K, "max_row": MAX_ROW, "max_dist": PARAMS[1], "genome_bases": int(a.genome),
           "coverage": a.coverage, "reads": n_reads, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    res["listed"], ubuf, uoff, urec, _, _, _, d_pl, n_pl, inner, _ = paired(m, bases, n_reads)
    n_uni, n_ub = int(uoff.numel() - 1), int(ubuf.numel())
    r_out, n_out, rst = reduce(m, a, uoff, n_ub, d_pl, n_pl, inner)
    s_full, (ns_f, _), st_f = scaffold(m, a, ubuf, uoff, urec, d_pl, n_pl, inner)
    s_red, (ns_r, _), st_r = scaffold(m, a, ubuf, uoff, urec, r_out[1], n_out, inner)
    torch.cuda.synchronize()
    ulen = np.diff(uoff.cpu().numpy())
    rec = r_out[0].cpu().numpy()[:n_pl].reshape(-1).view(PAIR_REDUCE_DTYPE)
    tr = rec[rec["verdict"] == 3]
    res.update(unitigs=n_uni, unitig_bases=n_ub, n50_unitigs=n50(ulen), pair_links=n_pl, inner=inner, stats=rst, links_out=n_out, max_n_via=int(tr["n_via"].max()) if len(tr) else 0,
               exact_skips=int((tr["delta"] == 0).sum()), scaffolds_full=scaffold_summary(s_full, ns_f, st_f, ulen), scaffolds_reduced=scaffold_summary(s_red, ns_r, st_r, ulen))

    def reduce_dev():
        reduce(m, a, uoff, n_ub, d_pl, n_pl, inner, r_out)

    def scaffold_dev():
        scaffold(m, a, ubuf, uoff, urec, d_pl, n_pl, inner, s_full)

    t_r, t_s = [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y = timed(reduce_dev, reps=1, warm=0)[0], timed(scaffold_dev, reps=1, warm=0)[0]
        if it:
            t_r.append(x)
            t_s.append(y)
    res["reduce_dev_s"], res["scaffold_dev_s"] = med(t_r, 6), med(t_s, 6)
    res["reduce_over_scaffold"] = round(res["reduce_dev_s"][0] / res["scaffold_dev_s"][0], 4)
    m.set_profile(1)
    reduce_dev()
    ph = m.unitig_pair_reduce_phases()
    scaffold_dev()
    sph = m.unitig_scaffold_phases()
    m.set_profile(0)
    res["phases_s"] = {f: round(v, 6) for f, v in ph.items()}
    res["scaffold_verdict_phase_s"] = round(sph["verdicts"], 6)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
