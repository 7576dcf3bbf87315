"""Cost and effect of threading the pair links through the graph (kmx_unitig_pair_paths_dev) beside two yardsticks; prints one JSON
line.

The setup is tools/bench_unitig_pairs.py's, over a genome with planted repeats: `--repeats` segments of `--repeat-len` bases, each
copied once more elsewhere in a genome of `--genome` bases, so that every one lies in the genome twice; paired reads (fragments
of 400 +- 40 bases, mates of 150, 1 % substitutions) at `--coverage`x, counted at k = 31 on the device, mapped, walked and paired on
count_unitig_graph_clean(thr = 3) of that session.  A read of 150 bases cannot cross a repeat of 150, the fragments do.  The call
takes the offsets, the CSR and the pair list of that run, with inner = the floor of the mean d of the pairs on one unitig,
tol = k, max_steps = 8, max_visits = 4096 and min_pairs = `--min-pairs`.  First the check: on pairs made the same way over a
genome of `--slice` bases with 2 repeats, the device form equals the plain-Python restatement of the rule
(tests/unitig_pair_paths_ref.py) on the library's unitigs, CSR and list.  Then, warmed, the median of 5 calls with [min, max], run
in turn on the same device buffers: kmx_unitig_pair_paths_dev (its sums into scratch arrays), kmx_unitig_pair_walks_dev on the
batch and kmx_unitig_scaffold_dev on the list; the seconds per phase of one call under the profile, entries and prefixes visited
per second of the search phase, the verdict counts, what kmx_unitig_resolve_dev says with and without the pair evidence, and the
contig N50 of kmx_unitig_contigs_dev on both resolved graphs.  Not measured: the host form and any size the call does not name.
usage: python tools/bench_unitig_pair_paths.py [--genome 3000000] [--repeats 200] [--repeat-len 150] [--coverage 10] [--slice 20000]"""
import argparse
import json
import os
import sys
import time
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_unitig_contigs import n50  # noqa: E402
from bench_unitig_map import med, timed  # noqa: E402
from bench_unitig_pairs import K, L, PARAMS, THR, make_pairs  # noqa: E402
from kmcex_amd import KModel, synth  # noqa: E402
from kmcex_amd.api import PAIR_DTYPE, PAIR_LINK_DTYPE, PAIR_PATH_DTYPE  # noqa: E402

MAX_STEPS, MAX_VISITS = 8, 4096


def planted_pairs(n_genome, coverage, repeats, repeat_len, seed=5):
    """make_pairs over the synthetic genome with `repeats` segments copied once more: the genome falls into 2 * repeats slots, the
    segment a quarter into an even slot is written over the same place of the odd slot behind it"""
    codes = synth.genome_bases(n_genome).copy()
    slot = n_genome // (2 * max(repeats, 1))
    assert slot >= 4 * repeat_len + 1200, "the repeats do not fit the genome"
    for i in range(repeats):
        src, dst = 2 * i * slot + slot // 4, (2 * i + 1) * slot + slot // 4
        codes[dst:dst + repeat_len] = codes[src:src + repeat_len]
    with mock.patch.object(synth, "genome_bases", lambda n: codes):
        return make_pairs(n_genome, coverage, seed)


def paired(m, bases, n_reads):
    """count, clean graph, map, walk, through hits and pairs on the device; the session stays open -> a dict of what the calls left"""
    d_b = torch.from_numpy(bases).cuda()
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    listed = m.count_finish()
    ubuf, uoff, urec, d_lo, d_lk, _, _ = m.count_unitig_graph_clean_dev(THR)
    m.count_unitig_map_begin_dev(ubuf, uoff)
    d_segs = torch.zeros((n_reads * L, 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_b, d_o, d_segs)
    d_segs = d_segs[:max(ns, 1)].clone()
    n_links, n_pairs = int(d_lk.numel()), n_reads // 2
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    wst, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, K, 1, d_walks, d_steps, None, d_hits)
    d_through, _ = m.unitig_through_dev(d_walks, wst["n_walks"], d_steps, wst["n_steps"], d_lo, d_lk)
    d_pairs = torch.zeros((n_pairs, 64), dtype=torch.uint8, device="cuda")
    d_ph = torch.zeros(max(n_links, 1), dtype=torch.int64, device="cuda")
    d_pl = torch.zeros((n_pairs, 32), dtype=torch.uint8, device="cuda")
    pst, n_pl = m.unitig_pairs_dev(d_walks, wst["n_walks"], d_wo, d_steps, wst["n_steps"], d_lo, d_lk, PARAMS[1], PARAMS[0], PARAMS[2], PARAMS[3], d_pairs, None, d_ph, d_pl, 0)
    torch.cuda.synchronize()
    rec = d_pairs.cpu().numpy().reshape(-1).view(PAIR_DTYPE)
    d = rec["d"][(rec["cls"] == 2) & (rec["frag"] >= 0)]
    inner = max(int(d.sum() // len(d)), 0) if len(d) else 0
    return dict(listed=listed, ubuf=ubuf, uoff=uoff, urec=urec, lo=d_lo, lk=d_lk, hits=(d_hits + d_ph)[:max(n_links, 1)], through=d_through, pl=d_pl, n_pl=n_pl, inner=inner, pair_stats=pst,
                walks=d_walks, n_walks=wst["n_walks"], wo=d_wo, steps=d_steps, n_steps=wst["n_steps"], pairs=d_pairs)


def paths(m, a, s, d_through=None, d_hits=None, out=None):
    return m.unitig_pair_paths_dev(K, s["uoff"], s["lo"], s["lk"], s["pl"], s["n_pl"], s["inner"], K, a.min_pairs, MAX_STEPS, MAX_VISITS, d_through, d_hits, out=out)


def slice_check(a):
    """the device form against the restatement on the library's unitigs, CSR and list of a small genome -> bool"""
    import unitig_links_ref as LR
    import unitig_pair_paths_ref as Q
    sb, sn = planted_pairs(a.slice, a.coverage, 2, a.repeat_len, seed=6)
    m = KModel(1, 65535, a.nh, a.nb)
    s = paired(m, sb, sn)
    m.unitig_map_end()
    nu, nl = int(s["uoff"].numel() - 1), int(s["lk"].numel())
    d_t, d_h = torch.zeros(16 * nu, dtype=torch.int64, device="cuda"), torch.zeros(max(nl, 1), dtype=torch.int64, device="cuda")
    out, n_st, st = paths(m, a, s, d_t, d_h)
    torch.cuda.synchronize()
    off = s["uoff"].cpu().numpy()
    mu = [max(int(off[i + 1] - off[i]) - (K - 1), 0) for i in range(nu)]
    rows = LR.rows_of(s["lo"].cpu().numpy(), s["lk"].cpu().numpy().view(np.uint32))
    plinks = [tuple(int(x) for x in e) for e in s["pl"].cpu().numpy()[:s["n_pl"]].reshape(-1).view(PAIR_LINK_DTYPE)]
    want = Q.flat(Q.pair_paths(mu, rows, plinks, a.min_pairs, s["inner"], K, MAX_STEPS, MAX_VISITS))
    got = (out[0].cpu().numpy()[:len(plinks)], out[1].cpu().numpy()[:n_st], d_t.cpu().numpy(), d_h.cpu().numpy()[:nl])
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and st == want[4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--repeat-len", type=int, default=150, dest="repeat_len")
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose pair paths are checked against the Python restatement")
    ap.add_argument("--min-pairs", type=int, default=2, dest="min_pairs")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = planted_pairs(int(a.genome), a.coverage, a.repeats, a.repeat_len)
    res = {"metric": "unitig_pair_paths", "k": K, "thr": THR, "min_pairs": a.min_pairs, "tol": K, "max_steps": MAX_STEPS, "max_visits": MAX_VISITS, "max_dist": PARAMS[1], "genome_bases": int(a.genome),
           "repeats": a.repeats, "repeat_len": a.repeat_len, "coverage": a.coverage, "read_len": L, "reads": n_reads, "pairs": n_reads // 2, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    s = paired(m, bases, n_reads)
    nu, nl, n_pl = int(s["uoff"].numel() - 1), int(s["lk"].numel()), s["n_pl"]
    # the effect: resolve and contigs without and with the pair evidence
    d_t, d_h = s["through"].clone(), s["hits"].clone()
    out, n_st, st = paths(m, a, s, d_t, d_h)
    torch.cuda.synchronize()
    rec = out[0].cpu().numpy()[:n_pl].reshape(-1).view(PAIR_PATH_DTYPE)
    res.update(listed=s["listed"], unitigs=nu, unitig_bases=int(s["ubuf"].numel()), links=nl, pair_links=n_pl, inner=s["inner"], pair_stats=s["pair_stats"], stats=st, path_steps=n_st,
               prefixes_visited=int(rec["n_visited"].sum()), longest_path=int(rec["n_steps"].max()) if n_pl else 0)
    for name, t, h in (("without", s["through"], s["hits"]), ("with", d_t, d_h)):
        r, (rn, rb), rst = m.unitig_resolve_dev(K, s["ubuf"], s["uoff"], s["lo"], s["lk"], t, a.min_pairs, 0, s["urec"], h)
        c, (cn, cb, cl), cst = m.unitig_contigs_dev(K, r[0][:rb], r[1][:rn + 1], r[5][:2 * rn + 1], r[6], r[8], 2, 4, r[2][:rn])
        torch.cuda.synchronize()
        res["resolve_" + name] = {f: rst[f] for f in ("n_candidates", "n_resolved", "n_crossed", "n_unsupported", "n_ambiguous")}
        res["contigs_" + name] = cn
        res["n50_contigs_" + name] = n50(np.diff(c[1].cpu().numpy()[:cn + 1]))
    res["n50_unitigs"] = n50(np.diff(s["uoff"].cpu().numpy()))
    # the cost, in turn on the same buffers
    s_t, s_h = torch.zeros_like(d_t), torch.zeros_like(d_h)
    d_pl2 = torch.zeros_like(s["pl"])
    sc_out = None
    try:
        sc_out = m.unitig_scaffold_dev(K, s["ubuf"], s["uoff"], s["pl"], n_pl, s["inner"], a.min_pairs, 4, 10, 2 * PARAMS[1], s["urec"])[0]
    except Exception as e:                                       # (sized at what always suffices: not expected)
        res["scaffold_error"] = str(e)

    def paths_dev():
        paths(m, a, s, s_t, s_h, out)

    def pairs_dev():
        m.unitig_pairs_dev(s["walks"], s["n_walks"], s["wo"], s["steps"], s["n_steps"], s["lo"], s["lk"], PARAMS[1], PARAMS[0], PARAMS[2], PARAMS[3], s["pairs"], None, None, d_pl2, 0)

    def scaffold_dev():
        m.unitig_scaffold_dev(K, s["ubuf"], s["uoff"], s["pl"], n_pl, s["inner"], a.min_pairs, 4, 10, 2 * PARAMS[1], s["urec"], out=sc_out)

    t_p, t_w, t_s = [], [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y = timed(paths_dev, reps=1, warm=0)[0], timed(pairs_dev, reps=1, warm=0)[0]
        z = timed(scaffold_dev, reps=1, warm=0)[0] if sc_out is not None else 0.0
        if it:
            t_p.append(x)
            t_w.append(y)
            t_s.append(z)
    res["pair_paths_dev_s"], res["pair_walks_dev_s"], res["scaffold_dev_s"] = med(t_p, 6), med(t_w, 6), med(t_s, 6)
    m.set_profile(1)
    paths_dev()
    ph = m.unitig_pair_paths_phases()
    m.set_profile(0)
    m.unitig_map_end()
    res["phases_s"] = {f: round(v, 6) for f, v in ph.items()}
    res["entries_per_s"] = round(n_pl / max(ph["search"], 1e-9))
    res["prefixes_per_s"] = round(res["prefixes_visited"] / max(ph["search"], 1e-9))
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
