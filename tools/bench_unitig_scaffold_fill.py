"""Cost and effect of filling the scaffolds' gaps along the graph (kmx_unitig_scaffold_fill_dev) beside two yardsticks; prints one
JSON line.

The input is tools/bench_unitig_scaffold.py's over the genome of tools/bench_unitig_pair_paths.py: `--repeats` segments of
`--repeat-len` bases, each copied once more elsewhere in a genome of `--genome` bases; paired reads (fragments of 400 +- 40 bases,
mates of 150, 1 % substitutions) at `--coverage`x, counted at k = 31 on the device, mapped, walked and paired on
count_unitig_graph_clean(thr = 3) of that session.  kmx_unitig_scaffold_dev runs on those unitigs and that list (inner = the floor of
the mean d of the pairs on one unitig, min_n = 10, max_n = 2 max_dist), kmx_unitig_pair_paths_dev on the same list and the graph's
CSR (tol = k, max_steps = 8, max_visits = 4096, the scaffolds' min_pairs), and the fill call takes what both left on the device.
First the check: on pairs made the same way over a genome of `--slice` bases with 2 repeats, the device form equals the plain-Python
restatement of the rule (tests/unitig_scaffold_fill_ref.py) on the library's unitigs, scaffolds, list and paths.  Then, warmed, the
median of 5 calls with [min, max], run in turn on the same device buffers: kmx_unitig_scaffold_fill_dev on exact room,
kmx_unitig_scaffold_dev and a device copy of n_fbases bytes; the seconds per phase of one call under the profile, the byte phase
(the N fill, the step emit, the gather emit of the pieces) beside the copy, the links per kind, the N removed and the bases filled,
and the N50 of the unitigs, the scaffolds and the filled scaffolds.  Not measured: the host form, the contig-level run, kinds 1 and
2 on their own, and any size the call does not name.
usage: python tools/bench_unitig_scaffold_fill.py [--genome 3000000] [--repeats 200] [--repeat-len 150] [--coverage 10] [--slice 20000]"""
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
from bench_unitig_pair_paths import MAX_STEPS, MAX_VISITS, paired, planted_pairs  # noqa: E402
from bench_unitig_pairs import K, PARAMS, THR  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import PAIR_LINK_DTYPE, PAIR_PATH_DTYPE, SCAFFOLD_DTYPE, SCAFFOLD_STEP_DTYPE, KmxError  # noqa: E402

MIN_N = 10


def scaffold(m, a, s, out=None):
    """kmx_unitig_scaffold_dev, on exact room after a sizing call when `out` is None -> (out, (n_scaffolds, n_sbases), stats)"""
    args = (K, s["ubuf"], s["uoff"], s["pl"], s["n_pl"], s["inner"], a.min_pairs, a.ratio, MIN_N, 2 * PARAMS[1], s["urec"])
    if out is not None:
        return m.unitig_scaffold_dev(*args, out=out)
    try:
        return m.unitig_scaffold_dev(*args, capacity=0)
    except KmxError as e:
        if e.code != -5:
            raise
        return m.unitig_scaffold_dev(*args, capacity=e.needed)


def fill(m, a, s, sc, ns, pp, n_pst, out=None):
    """kmx_unitig_scaffold_fill_dev on what the scaffold and the pair-path call left, on exact room after a sizing call when `out` is
    None -> (out, (n_fbases, n_pieces), stats)"""
    args = (K, s["ubuf"], s["uoff"], sc[2], ns, sc[3], s["pl"], s["n_pl"], pp[0], pp[1], n_pst, a.kinds)
    if out is not None:
        return m.unitig_scaffold_fill_dev(*args, out=out)
    try:
        return m.unitig_scaffold_fill_dev(*args, capacity=0, piece_capacity=max(n_pst, 1))
    except KmxError as e:
        if e.code != -5:
            raise
        return m.unitig_scaffold_fill_dev(*args, capacity=e.needed, piece_capacity=max(e.needed_pieces, 1))


def chain(m, a, s):
    """scaffold, pair paths, fill -> (the scaffold call's result, the path call's, the fill call's)"""
    sc = scaffold(m, a, s)
    pp = m.unitig_pair_paths_dev(K, s["uoff"], s["lo"], s["lk"], s["pl"], s["n_pl"], s["inner"], K, a.min_pairs, MAX_STEPS, MAX_VISITS)
    return sc, pp, fill(m, a, s, sc[0], sc[1][0], pp[0], pp[1])


def slice_check(a):
    """the device form against the restatement on the library's unitigs, scaffolds, list and paths of a small genome -> bool"""
    import unitig_scaffold_fill_ref as F
    sb, sn = planted_pairs(a.slice, a.coverage, 2, a.repeat_len, seed=6)
    m = KModel(1, 65535, a.nh, a.nb)
    s = paired(m, sb, sn)
    m.unitig_map_end()
    (sc, (ns, nsb), _), (pp, n_pst, _), (out, (nf, npc), st) = chain(m, a, s)
    torch.cuda.synchronize()
    off, buf = s["uoff"].cpu().numpy(), s["ubuf"].cpu().numpy().tobytes().decode()
    nu = len(off) - 1
    strs = [buf[int(off[i]):int(off[i + 1])] for i in range(nu)]
    plinks = [tuple(int(x) for x in e) for e in s["pl"].cpu().numpy()[:s["n_pl"]].reshape(-1).view(PAIR_LINK_DTYPE)]
    srec = sc[2].cpu().numpy()[:ns].reshape(-1).view(SCAFFOLD_DTYPE)
    steps = [tuple(int(x) for x in e) for e in sc[3].cpu().numpy()[:nu].reshape(-1).view(SCAFFOLD_STEP_DTYPE)]
    precs = [tuple(int(x) for x in e) for e in pp[0].cpu().numpy()[:len(plinks)].reshape(-1).view(PAIR_PATH_DTYPE)]
    psteps = [int(x) for x in pp[1].cpu().numpy()[:n_pst].view(np.uint32)]
    want = F.flat(F.fill(K, strs, [(int(r["first_step"]), int(r["n_steps"])) for r in srec], steps, plinks, precs, psteps, a.kinds))
    got = (out[0].cpu().numpy()[:nf], out[1].cpu().numpy()[:ns + 1], out[2].cpu().numpy()[:ns], out[3].cpu().numpy()[:nu], out[4].cpu().numpy()[:npc])
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and st == want[5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=3e6)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--repeat-len", type=int, default=150, dest="repeat_len")
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose filled scaffolds are checked against the Python restatement")
    ap.add_argument("--min-pairs", type=int, default=2, dest="min_pairs")
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--kinds", type=int, default=3)
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = planted_pairs(int(a.genome), a.coverage, a.repeats, a.repeat_len)
    res = {"metric": "unitig_scaffold_fill", "k": K, "thr": THR, "min_pairs": a.min_pairs, "ratio": a.ratio, "kinds": a.kinds, "tol": K, "max_steps": MAX_STEPS, "max_visits": MAX_VISITS, "min_n": MIN_N,
           "max_n": 2 * PARAMS[1], "genome_bases": int(a.genome), "repeats": a.repeats, "repeat_len": a.repeat_len, "coverage": a.coverage, "reads": n_reads, "gen_s": round(time.perf_counter() - t0, 1)}
    res["slice_equals_reference"] = ok = slice_check(a)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    s = paired(m, bases, n_reads)
    m.unitig_map_end()
    (sc, (ns, nsb), sst), (pp, n_pst, pst), (out, (nf, npc), st) = chain(m, a, s)
    torch.cuda.synchronize()
    nu = int(s["uoff"].numel() - 1)
    ulen, slen, flen = np.diff(s["uoff"].cpu().numpy()), np.diff(sc[1].cpu().numpy()[:ns + 1]), np.diff(out[1].cpu().numpy()[:ns + 1])
    frec = out[2].cpu().numpy()[:ns].reshape(-1).view(np.uint64).reshape(-1, 8)
    res.update(listed=s["listed"], unitigs=nu, unitig_bases=int(s["ubuf"].numel()), pair_links=s["n_pl"], inner=s["inner"], scaffolds=ns, scaffold_bases=nsb, scaffold_gap_bases=int(slen.sum() - ulen.sum()),
               path_stats=pst, path_steps=n_pst, filled_bases=nf, pieces=npc, stats=st, gap_bases_left=int(frec[:, 1].sum()), n50_unitigs=n50(ulen), n50_scaffolds=n50(slen), n50_filled=n50(flen))
    d_copy, d_src = torch.empty(max(nf, 1), dtype=torch.uint8, device="cuda"), out[0][:max(nf, 1)]

    def fill_dev():
        fill(m, a, s, sc, ns, pp, n_pst, out)

    def scaffold_dev():
        scaffold(m, a, s, sc)

    def copy_dev():
        d_copy.copy_(d_src, non_blocking=True)                   # a device-to-device hipMemcpyAsync on the current stream

    t_f, t_s, t_m = [], [], []
    for it in range(6):                                          # in turn, the first round warms
        x, y, z = timed(fill_dev, reps=1, warm=0)[0], timed(scaffold_dev, reps=1, warm=0)[0], timed(copy_dev, reps=1, warm=0)[0]
        if it:
            t_f.append(x)
            t_s.append(y)
            t_m.append(z)
    res["fill_dev_s"], res["scaffold_dev_s"], res["copy_s"] = med(t_f, 5), med(t_s, 5), med(t_m, 6)
    res["fill_over_scaffold"] = round(res["fill_dev_s"][0] / res["scaffold_dev_s"][0], 4)
    m.set_profile(1)
    fill_dev()
    ph = m.unitig_scaffold_fill_phases()
    m.set_profile(0)
    res["phases_s"] = {f: round(v, 6) for f, v in ph.items()}
    res["bytes_phase_over_copy"] = round(ph["bytes"] / max(res["copy_s"][0], 1e-9), 3)
    res["bytes_phase_gb_s"] = round(nf / max(ph["bytes"], 1e-9) / 1e9, 1)
    res["copy_gb_s"] = round(nf / max(res["copy_s"][0], 1e-9) / 1e9, 1)
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
