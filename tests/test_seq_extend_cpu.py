"""CPU side of the path extension (kmx_extend_seqs): the record's layout in the header and the NumPy dtype agree; the
reference rule (tests/seq_extend_ref.py) driven by the CPU oracle on hand-built sequences for every stop code; a tie caused
by a false positive of the model is broken by the lookahead; walks over the GENOME_CASES genomes follow the genome; the
fixture tests/golden/seq_extend_golden.json still describes the oracle's result; the facade compiles."""
import json
import os
import subprocess
import sys

import numpy as np

import count_reads as CR
import oracle_lib as O
import seq_correct_ref as SC
import seq_extend_ref as X
import seq_reads as R
from common import GENOME_CASES
from kmcex_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
K = 21
GCASE = {c[0]: c for c in GENOME_CASES}


def test_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmx.h"\nint main(void){ printf("%zu", sizeof(kmx_seq_extension));\n'
                   + "".join(f' printf(" %zu", offsetof(kmx_seq_extension, {f}));\n' for f in X.FIELDS)
                   + ' printf(" %d %d %d %d %d %d %d %d", KMX_EXT_DEAD_END, KMX_EXT_BRANCH, KMX_EXT_JOIN, KMX_EXT_CYCLE, KMX_EXT_MAX_EXT, KMX_EXT_BAD_SEED,'
                   + ' KMX_EXT_MAX_EXT_LIMIT, KMX_EXT_MAX_DEPTH);\n printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *rest = (int(x) for x in subprocess.check_output([str(exe)]).split())
    offs, codes = rest[:7], rest[7:]
    assert size == 32 == api.SEQ_EXTENSION_DTYPE.itemsize and X.DTYPE == api.SEQ_EXTENSION_DTYPE
    assert offs == [0, 4, 8, 12, 16, 20, 24] == [api.SEQ_EXTENSION_DTYPE.fields[f][1] for f in X.FIELDS]
    assert codes == [X.DEAD_END, X.BRANCH, X.JOIN, X.CYCLE, X.MAX_EXT, X.BAD_SEED, 65536, 3] and sorted(api.SEQ_EXTENSION_STOPS) == codes[:6]
    assert "kmx_extend_seqs" in api.ABI_SYMBOLS and "kmx_extend_seqs_dev" in api.ABI_SYMBOLS
    assert all(callable(getattr(api.KModel, f)) for f in ("seq_extend_flat", "seq_extend", "seq_extend_dev"))


def _model(seqs, k=K, ci=1):
    """a CPU oracle holding every k-mer of these sequences"""
    buf, off = R.flatten(seqs)
    km, cnt = CR.count(buf, off, k, ci, 1023)
    o = O.OracleModel(ci, 1023, 7, 5)
    o.build(k, km, cnt)
    return o


def _walk(o, seeds, max_ext, depth, k=K, thr=1):
    buf, off = R.flatten(seeds)
    ext, rec, _ = X.oracle_extend(o, buf, off, k, thr, max_ext, depth)
    return [ext[i, :int(rec["n_ext"][i])].tobytes() for i in range(len(seeds))], rec, ext


def _check_counts(o, seed, ext, r, k=K):
    """seed_occ, sum_occ, min_occ and max_occ of a record against the oracle's answers along seed + ext"""
    ask = SC.oracle_rows(o, k)
    path = np.frombuffer(seed[-k:] + ext, dtype=np.uint8)
    occ = ask(np.lib.stride_tricks.sliding_window_view(path, k))
    assert int(r["seed_occ"]) == int(occ[0])
    if len(ext):
        assert (int(r["sum_occ"]), int(r["min_occ"]), int(r["max_occ"])) == (int(occ[1:].sum()), int(occ[1:].min()), int(occ[1:].max()))
    else:
        assert (int(r["sum_occ"]), int(r["min_occ"]), int(r["max_occ"])) == (0, -1, -1)


def test_every_stop_code_on_hand_made_sequences():
    g = R.genome_ascii(3000, seed=5).tobytes()
    for depth in (2, 3):                                             # (at depth 0 a false positive of the model ends these walks early)
        # a linear path: the walk appends the rest of the sequence and finds nothing behind its end
        o = _model([g[:600]])
        (e,), rec, rows = _walk(o, [g[100:100 + K]], 2000, depth)
        assert (int(rec["stop"][0]), e) == (X.DEAD_END, g[100 + K:600]) and int(rec["n_ext"][0]) == 600 - 100 - K
        assert not rows[0, len(e):].any() and rows.shape == (1, 2000)
        _check_counts(o, g[100:100 + K], e, rec[0])
        # ... an N before the last k bytes of the seed changes nothing, max_ext cuts the walk
        (e2, e3), rec2, _ = _walk(o, [b"ACNNacgt" + g[100:100 + K], g[90:100 + K]], 50, depth)
        assert e2 == e3 == e[:50] and list(rec2["stop"]) == [X.MAX_EXT, X.MAX_EXT] and list(rec2["n_ext"]) == [50, 50]
        (e1,), rec1, _ = _walk(o, [g[100:100 + K]], 1, depth)
        assert e1 == e[:1] and int(rec1["stop"][0]) == X.MAX_EXT
        # two alleles behind the seed: BRANCH where they part; entering downstream of the variant: JOIN where they meet
        alt = bytearray(g[:600])
        alt[300] = ord("A") if g[300] != ord("A") else ord("C")
        o = _model([g[:600], bytes(alt)])
        (eb, ej), rec, _ = _walk(o, [g[200:200 + K], g[295:295 + K]], 2000, depth)
        assert (int(rec["stop"][0]), eb) == (X.BRANCH, g[200 + K:300])
        assert (int(rec["stop"][1]), ej) == (X.JOIN, g[295 + K:300 + K]) and int(rec["n_ext"][1]) == 5
        _check_counts(o, g[200:200 + K], eb, rec[0])
        # a circular sequence of n bases has n k-mers: the walk appends n - 1 bases, the n-th would close the circle
        n = 200
        c = g[1000:1000 + n]
        o = _model([c + c[:K - 1]])
        (ec,), rec, _ = _walk(o, [c[:K]], 2000, depth)
        assert (int(rec["stop"][0]), int(rec["n_ext"][0]), ec) == (X.CYCLE, n - 1, (c + c)[K:K + n - 1])
        (ec2,), rec, _ = _walk(o, [c[50:50 + K]], 2000, depth)                   # entered anywhere, it comes back to its seed
        assert (int(rec["stop"][0]), ec2) == (X.CYCLE, (c + c + c)[50 + K:50 + K + n - 1])
        # bad seeds: shorter than k, empty, an N, a lowercase byte, an IUPAC letter in the last k bytes
        o = _model([g[:600]])
        s = g[100:100 + K]
        bad = [s[:K - 1], b"", s[:3] + b"N" + s[4:], s[:K - 1] + bytes([s[K - 1] + 32]), b"R" + s[1:], g[50:100] + b"N"]
        ext, rec, rows = _walk(o, bad + [s], 40, depth)
        assert list(rec["stop"][:len(bad)]) == [X.BAD_SEED] * len(bad) and not rows[:len(bad)].any()
        for f, v in (("n_ext", 0), ("seed_occ", -1), ("min_occ", -1), ("max_occ", -1), ("n_lookahead", 0), ("sum_occ", 0)):
            assert (rec[f][:len(bad)] == v).all(), f
        assert ext[-1] == g[100 + K:140 + K]
        # a seed that is not in the model: seed_occ is the model's answer, the walk still looks at its successors
        stranger = (b"C" if s[:1] == b"A" else b"A") + s[1:]
        (es,), rec, _ = _walk(o, [stranger], 40, depth)
        _check_counts(o, stranger, es, rec[0])
        assert int(rec["seed_occ"][0]) < 1 and int(rec["stop"][0]) == X.JOIN and es == b""   # (s itself is the other predecessor)
        far = R.genome_ascii(100, seed=99).tobytes()[:K]
        (ef,), rec, _ = _walk(o, [far], 40, depth)
        assert (int(rec["seed_occ"][0]), int(rec["stop"][0]), ef) == (0, X.DEAD_END, b"")


def _genome_seeds(case, n, max_ext, seed=3):
    _, k, _, _, _, _, n_bases = case
    g = R.genome_ascii(n_bases)
    starts = np.random.default_rng(seed).integers(0, n_bases - max_ext - 2 * k, size=n)
    return g.tobytes(), starts.tolist(), [g[a:a + k].tobytes() for a in starts.tolist()]


def test_a_false_positive_tie_is_broken_by_the_lookahead():
    import make_seq_correct_golden as G
    case = GCASE["genome_k31_ci1"]
    k, ci = case[1], case[2]
    o = G.oracle_of(case)
    g, starts, seeds = _genome_seeds(case, 200, 100)
    e0, r0, _ = _walk(o, seeds, 100, 0, k, ci)
    e2, r2, _ = _walk(o, seeds, 100, 2, k, ci)
    found = [i for i in range(len(seeds)) if int(r0["stop"][i]) in (X.BRANCH, X.JOIN) and int(r2["n_ext"][i]) > int(r0["n_ext"][i])]
    print("stopped by a tie at depth 0 and running on at depth 2:", len(found), "of", len(seeds))
    assert len(found) >= 20
    for i in found:
        assert int(r2["n_lookahead"][i]) >= 1
        assert e2[i] == g[starts[i] + k:starts[i] + k + len(e2[i])] and e2[i][:len(e0[i])] == e0[i]


def test_walks_follow_the_genome():
    import make_seq_correct_golden as G
    for name, thr in (("genome_k31_ci1", 1), ("genome_k27_ci2", 2)):
        case = GCASE[name]
        k = case[1]
        o = G.oracle_of(case)
        g, starts, seeds = _genome_seeds(case, 200, 500)
        ext, rec, _ = _walk(o, seeds, 500, 2, k, thr)
        reached = int((rec["stop"] == X.MAX_EXT).sum())
        print(name, X.tallies(rec))
        assert 2 * reached >= len(seeds)
        if name == "genome_k31_ci1":                                 # the true successor is always solid: a false one can tie, never win
            assert all(e == g[a + k:a + k + len(e)] for e, a in zip(ext, starts))
            _check_counts(o, seeds[0], ext[0], rec[0], k)


def test_result_of_the_golden():
    import make_seq_extend_golden as G
    with open(os.path.join(ROOT, "tests", "golden", "seq_extend_golden.json")) as f:
        sg = json.load(f)
    assert sorted(sg["cases"]) == sorted(c[0] for c in GENOME_CASES) and sg["recipe"] == G.RECIPE
    for case in GENOME_CASES:
        assert G.entry(case, G.oracle_of(case)) == sg["cases"][case[0]], case[0]
    t = sg["cases"]["genome_k31_ci1"]["depth"]["2"]["tallies"]
    assert sum(t[n] for n in X.STOP_NAMES.values()) == sg["cases"]["genome_k31_ci1"]["n_seeds"] == 2008 and t["bad_seed"] >= 100


def test_left_is_the_walk_of_the_reverse_complement():
    """what left=True of the Python facade does on the host, stated on the reference rule: at k <= 32 both strands of a k-mer
    get one answer, so walking left from a k-mer retraces the genome backwards"""
    import make_seq_correct_golden as G
    case = GCASE["genome_k31_ci1"]
    k = case[1]
    o = G.oracle_of(case)
    g = R.genome_ascii(case[6]).tobytes()
    seeds = [g[a:a + 60] for a in (5000, 90000, 200000)]
    buf, off = R.flatten(seeds)
    ext, rec, _ = X.extend_left(buf, off, k, 1, 200, 2, SC.oracle_rows(o, k))
    for i, a in enumerate((5000, 90000, 200000)):
        n = int(rec["n_ext"][i])
        assert n >= 1 and X.revcomp(ext[i, :n].tobytes()) == g[a - n:a]


def test_facade_seq_extend_program_compiles(tmp_path):
    api.load_library()
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_extend.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", str(tmp_path / "facade_seq_extend")])
