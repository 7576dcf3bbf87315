"""Cost of cleaning the unitig graph on the device (kmx_count_unitig_graph_clean_dev on a counted session); prints one JSON line.

Reads: tools/bench_count.py's own read set, as tools/bench_unitigs.py takes it (150-base reads, half reverse-complemented, 1 %
substitutions, at `--coverage`x over a synth.genome_bases genome of `--genome` bases), counted at k = 31 on the device.  First
the check: on reads made the same way over a genome of `--slice` bases the host and the device variant equal the plain-Python
restatement of the rule (tests/unitig_clean_ref.py) at thr = 1 and thr = 3.  Then, for thr = 1 and thr = 3 with ops = 7, caps
2 k and at most 16 rounds, warmed, the median of 5 calls with [min, max]: the seconds of the cleaning call and, interleaved with
it call by call on the same listing in the same process, of kmx_count_unitig_graph_dev; their ratio clean / (rounds_run x graph);
rounds run, what each round removed (from max_rounds = 1, 2, ... prefixes, outside the timing), unitigs and N50 before and
after; and from one further call under set_profile(1) the six phase figures summed over the rounds.
usage: python tools/bench_unitig_clean.py [--genome 100000000] [--coverage 10] [--slice 20000]"""
import argparse
import ctypes as C
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
from bench_count import make_reads  # noqa: E402
from bench_unitigs import med, n50  # noqa: E402
from kmcex_amd import KModel  # noqa: E402
from kmcex_amd.api import UNITIG_CLEAN_PHASES, CleanParams, CleanStats  # noqa: E402

K, L = 31, 150
FIELDS = [f for f, _ in CleanStats._fields_]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=1e8)
    ap.add_argument("--coverage", type=float, default=10)
    ap.add_argument("--slice", type=int, default=20000, help="genome bases whose reads are checked against the Python restatement")
    ap.add_argument("--nh", type=int, default=7)
    ap.add_argument("--nb", type=int, default=5)
    a = ap.parse_args()
    t0 = time.perf_counter()
    bases, n_reads = make_reads(int(a.genome), a.coverage, L)
    res = {"metric": "unitig_clean", "k": K, "genome_bases": int(a.genome), "coverage": a.coverage, "read_len": L, "reads": n_reads,
           "ops": 7, "max_tip": 2 * K, "max_bubble": 2 * K, "max_rounds": 16, "gen_s": round(time.perf_counter() - t0, 1)}

    # the check: the rule's restatement on the reads of a small genome of its own (the same generator)
    import unitig_clean_ref as CL
    import unitigs_ref as U
    sb, sn = make_reads(a.slice, a.coverage, L, seed=6)
    sreads = [sb[i * L:(i + 1) * L].tobytes().decode() for i in range(sn)]
    skm, scnt = U.listing_of(U.count_kmers(sreads, K))
    ms = KModel(1, 65535, a.nh, a.nb)
    ms.count_begin(K)
    ms.count_seqs(sb, np.arange(sn + 1, dtype=np.uint64) * np.uint64(L))
    ms.count_finish()
    ok_ref = True
    for thr in (1, 3):
        want = CL.clean(skm, scnt, K, thr)
        flat = tuple(x.tobytes() for x in CL.flat(want))
        got = ms.count_unitig_graph_clean(thr)
        ok_ref = ok_ref and tuple(np.asarray(x).tobytes() for x in got[:6]) == flat and got[6] == want["stats"]
        dev = ms.count_unitig_graph_clean_dev(thr)
        ok_ref = ok_ref and tuple(x.cpu().numpy().tobytes() for x in dev[:6]) == flat and dev[6] == want["stats"]
    res["slice_equals_reference"] = ok_ref
    del ms

    # the session
    d_b = torch.from_numpy(bases).cuda()
    d_o = (torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * L)
    m = KModel(1, 65535, a.nh, a.nb)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.count_begin(K)
    m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L)
    torch.cuda.synchronize()
    n = m.count_finish()
    torch.cuda.synchronize()
    res["listed"] = n
    del d_b, d_o
    torch.cuda.empty_cache()

    nu, nb, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    st = CleanStats()
    P = CleanParams(7, 2 * K, 2 * K, 16)
    for thr in (1, 3):
        gg = m.count_unitig_graph_dev(thr)
        cc = m.count_unitig_graph_clean_dev(thr)
        stats = cc[6]
        lens0 = (gg[1][1:] - gg[1][:-1]).cpu().numpy()
        lens1 = (cc[1][1:] - cc[1][:-1]).cpu().numpy()
        r = {"rounds_run": stats["rounds_run"], "converged": stats["converged"], "stats": stats,
             "unitigs_before": int(len(lens0)), "n50_before": n50(lens0), "n_links_before": int(gg[4].numel()),
             "unitigs_after": int(len(lens1)), "n50_after": n50(lens1), "n_links_after": int(cc[4].numel()),
             "nodes_before": int(lens0.sum() - (K - 1) * len(lens0))}
        per_round, prev = [], dict.fromkeys(FIELDS, 0)
        for mr in range(1, stats["rounds_run"] + 1):               # what each round removed: the differences of the prefixes
            s = m.count_unitig_graph_clean_dev(thr, max_rounds=mr)[6]
            per_round.append({f: s[f] - prev[f] for f in ("n_tips", "n_islands", "n_bubbles", "n_kmers_removed")})
            prev = s
        r["per_round"] = per_round
        lk_g = gg[4] if gg[4].numel() else torch.empty(1, dtype=torch.int32, device=gg[0].device)      # (an empty tensor has no address to give)
        lk_c = cc[4] if cc[4].numel() else torch.empty(1, dtype=torch.int32, device=cc[0].device)
        graph_args = (m.h, thr, gg[0].data_ptr(), gg[0].numel(), gg[1].data_ptr(), gg[2].data_ptr(), gg[2].shape[0], gg[3].data_ptr(), lk_g.data_ptr(), gg[4].numel(),
                      C.byref(nu), C.byref(nb), C.byref(nl))
        clean_args = (m.h, thr, C.addressof(P), cc[0].data_ptr(), cc[0].numel(), cc[1].data_ptr(), cc[2].data_ptr(), cc[2].shape[0], cc[3].data_ptr(), lk_c.data_ptr(), cc[4].numel(),
                      C.byref(nu), C.byref(nb), C.byref(nl), cc[5].data_ptr(), C.addressof(st))
        ctimes, gtimes = [], []
        for it in range(6):                                        # the calls above warmed the buffers; one more, then 5
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = m.L.kmx_count_unitig_graph_clean_dev(*clean_args)
            torch.cuda.synchronize()
            if rc:
                raise SystemExit(f"kmx_count_unitig_graph_clean_dev failed: {rc}")
            if it:
                ctimes.append(time.perf_counter() - t)
            torch.cuda.synchronize()                               # the graph call in turn with the cleaning call
            t = time.perf_counter()
            rc = m.L.kmx_count_unitig_graph_dev(*graph_args)
            torch.cuda.synchronize()
            if rc:
                raise SystemExit(f"kmx_count_unitig_graph_dev failed: {rc}")
            if it:
                gtimes.append(time.perf_counter() - t)
        r["clean_seconds"] = med(ctimes)
        r["graph_seconds"] = med(gtimes)
        r["ratio_clean_over_rounds_x_graph"] = round(r["clean_seconds"][0] / (stats["rounds_run"] * r["graph_seconds"][0]), 3)
        m.set_profile(1)
        m.L.kmx_count_unitig_graph_clean_dev(*clean_args)
        torch.cuda.synchronize()
        m.set_profile(0)
        m.kernel_times(reset=True)
        ph = m.unitig_clean_phases()
        r["clean_phase_s"] = {p: round(ph[p], 4) for p in UNITIG_CLEAN_PHASES}
        r["doubling_rounds"] = ph["rounds"]
        res[f"thr{thr}"] = r
        del gg, cc, lk_g, lk_c, graph_args, clean_args
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    sys.exit(0 if ok_ref else 1)


if __name__ == "__main__":
    main()
