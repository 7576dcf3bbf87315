"""kmx_edit_seqs / kmx_edit_seqs_dev / kmx_apply_edits_dev: substitutions and single-base insertions / deletions of reads found
on the device.  The edit list and the records must EQUAL, byte for byte, the reference rule (tests/seq_edit_ref.py) driven by the
CPU oracle and by the GPU's own seq_to_occ_flat / kmer_to_occ_rows, and the applied bases the NumPy apply: every output is an
integer or a byte and no decision depends on another, there is no tolerance."""
import functools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle_lib as O
import seq_edit_reads as ER
import seq_edit_ref as E
import seq_reads as R
from common import CASE, GENOME_CASES, SMALL
from kmcex_amd import KModel, api, synth
from test_gpu_alloc_failure import walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCASE = {c[0]: c for c in GENOME_CASES}
REC = api.SEQ_EDITS_DTYPE


def _genome_model(name, oracle=True):
    _, k, ci, cs, nh, nb, n_bases = GCASE[name]
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    o = None
    if oracle:
        o = O.OracleModel(ci, cs, nh, nb)
        o.build(k, km, cnt)
    return m, o, k, ci, n_bases


@functools.lru_cache(maxsize=None)
def _reads_case(name):
    """model, oracle, the recipe's 2000 reads and the oracle's per-base answers: computed once, shared, left unchanged"""
    m, o, k, ci, n_bases = _genome_model(name)
    reads, _ = ER.make_reads(n_bases, k, n_reads=2000)
    buf, offsets = R.flatten(reads)
    return m, o, k, ci, reads, buf, offsets, R.oracle_per_base(o, buf, offsets, k)


def _dev(m, buf, offsets, thr, ms, ops=7, n_bases=None, records=True, apply=True):
    """the device variants on fresh device copies, outputs pre-filled with 0xFF -> (edits, records, applied bases, offsets_out)"""
    import torch
    n_seqs, n = len(offsets) - 1, len(buf) if n_bases is None else n_bases
    cap = n // 3 + 1
    d_seq = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda") if len(buf) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda")
    d_ed = torch.full((cap * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    d_rec = torch.full((max(n_seqs, 1) * 80,), 0xFF, dtype=torch.uint8, device="cuda")
    n_ed = m.seq_edit_dev(d_seq.data_ptr(), d_off.data_ptr(), n_seqs, n, thr, ms, ops, d_ed.data_ptr(), cap, d_rec.data_ptr() if records else 0)
    torch.cuda.synchronize()
    edits, rec = d_ed.cpu().numpy().view(np.uint64)[:n_ed].copy(), d_rec.cpu().numpy()[:n_seqs * 80].view(REC)
    if not apply:
        return edits, rec
    d_out = torch.full((n + n_ed + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    d_oo = torch.full(((n_seqs + 1) * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    m.apply_edits_dev(d_seq.data_ptr(), d_off.data_ptr(), n_seqs, n, d_ed.data_ptr(), n_ed, d_out.data_ptr(), n + n_ed, d_oo.data_ptr())
    torch.cuda.synchronize()
    oo = d_oo.cpu().numpy().view(np.uint64)
    out = d_out.cpu().numpy()
    assert (out[int(oo[-1]):] == 0xFF).all()
    return edits, rec, out[:int(oo[-1])], oo


def _gpu_rule(m, buf, offsets, k, thr, ms, ops=7):
    """the reference rule over the GPU's own answers"""
    return E.edit_seqs(m.seq_to_occ_flat(buf, offsets), buf, offsets, k, thr, ms, ops, lambda rows: m.kmer_to_occ_rows(rows, k))[:2]


def _same(got, want):
    return got[0].dtype == np.uint64 and np.array_equal(got[0], want[0]) and E.same(got[1], want[1])


def _applied(got, buf, offsets, want_edits):
    w_out, w_off = E.apply_edits(buf, offsets, want_edits)
    return np.array_equal(got[2], w_out) and np.array_equal(got[3], w_off)


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "seq_edit_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("which", ["ci_ms1", "ci_ms4", "ci1_ms1"])
@pytest.mark.parametrize("name", [c[0] for c in GENOME_CASES])
def test_reads_match_the_oracle(name, which):
    m, o, k, ci, reads, buf, offsets, per_base = _reads_case(name)
    thr, ms = {"ci_ms1": (ci, 1), "ci_ms4": (ci, 4), "ci1_ms1": (ci + 1, 1)}[which]
    sg = _golden()["cases"][name]
    for ops in (7, 1, 6):
        w_ed, w_rec, _ = E.edit_seqs(per_base, buf, offsets, k, thr, ms, ops, E.S.oracle_rows(o, k))
        t = E.tallies(w_rec, w_ed)
        print(name, thr, ms, ops, t)
        if (thr, ms, ops) == (ci, 1, 7):                             # the data is not degenerate: judged on the ORACLE's result
            assert t["n_sub"] >= 400 and t["n_del"] >= 250 and t["n_ins"] >= 200 and t["n_ambiguous"] >= 1 and R.dirty_windows(buf, offsets, k) > 1000
            assert all(sg["tallies"][f] == v for f, v in t.items())
        else:
            assert t == sg["variants"][f"thr{thr}_ms{ms}_ops{ops}"]
        got = m.seq_edit_flat(buf, offsets, thr, ms, ops)
        assert got[1].dtype == REC and got[1].shape == (len(reads),)
        assert _same(got, (w_ed, w_rec)), (thr, ms, ops)
        dev = _dev(m, buf, offsets, thr, ms, ops)
        assert _same(dev, (w_ed, w_rec)) and _applied(dev, buf, offsets, w_ed), (thr, ms, ops)
        w_out, w_off = E.apply_edits(buf, offsets, w_ed)
        assert np.array_equal(np.diff(w_off), w_rec["out_len"])
        if ops == 1:                                                 # the substitution corrector
            c_out, c_rec = m.seq_correct_flat(buf, offsets, thr, ms)
            assert np.array_equal(w_out, c_out) and np.array_equal(w_rec["n_sub"], c_rec["n_corrected"]) and np.array_equal(w_rec["n_sites"], c_rec["n_sites"])
        if (thr, ms, ops) == (ci, 1, 7):
            assert _same(_gpu_rule(m, buf, offsets, k, thr, ms), (w_ed, w_rec))
            assert np.array_equal(_dev(m, buf, offsets, thr, ms, records=False, apply=False)[0], w_ed)   # d_rec == NULL
            fixed, rec, ed = m.seq_edit(reads, thr, ms)              # the list form
            assert b"".join(fixed) == w_out.tobytes() and [len(f) for f in fixed] == np.diff(w_off).tolist() and E.same(rec, w_rec) and np.array_equal(ed, w_ed)
            i = max((j for j in range(len(reads)) if w_rec["n_ins"][j] and w_rec["n_del"][j]), key=lambda j: len(reads[j]))
            one, r1, e1 = m.seq_edit(reads[i].decode("latin-1"), thr, ms)
            assert one == fixed[i] != reads[i] and r1.tobytes() == w_rec[i].tobytes() and len(e1) == int(w_rec[i]["n_sub"] + w_rec[i]["n_del"] + w_rec[i]["n_ins"])


def _with_indels(strs, rng, k):
    """joined k-mers of the model with single-base indels, substitutions and dirty bytes; plus the special reads"""
    reads, cur = [], []
    for i, s in enumerate(strs):
        s = s.copy()
        p = int(rng.integers(0, k))
        if i % 4 == 0:                                               # a substitution inside a known k-mer
            s[p] = R.ACGT[(int(np.searchsorted(R.ACGT, s[p])) + int(rng.integers(1, 4))) % 4]
        elif i % 4 == 1:                                             # a lost base
            s = np.delete(s, p)
        elif i % 4 == 2:                                             # a surplus base
            s = np.insert(s, p, R.ACGT[int(rng.integers(0, 4))])
        if i % 13 == 5:
            s[int(rng.integers(0, len(s)))] = ord("N") if i % 2 else ord("a")
        cur.append(s.tobytes())
        cur.append(R.ACGT[rng.integers(0, 4, size=int(rng.integers(0, 4)))].tobytes())
        if rng.random() < 0.1:
            reads.append(b"".join(cur))
            cur = []
    return reads + [b"".join(cur), b"", strs[0].tobytes()[:k - 1], strs[1].tobytes()]


@pytest.mark.parametrize("name", SMALL)
def test_every_k_matches_the_existing_paths(name):
    """k = 16 ... 64, one- and two-word k-mers: against the rule over the GPU's own answers, a fifth of the reads against the oracle"""
    _, k, ci, cs, nh, nb, n = CASE[name]
    km, cnt = synth.make_stream(n, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    rng = np.random.default_rng(k)
    reads = _with_indels(synth.to_ascii(km[rng.permutation(len(cnt))[:4000]], k), rng, k)
    buf, offsets = R.flatten(reads)
    for thr, ms, ops in ((ci, 1, 7), (ci + 2, 2, 6)):
        want = _gpu_rule(m, buf, offsets, k, thr, ms, ops)
        print(name, thr, ms, ops, E.tallies(want[1], want[0]))
        assert int(want[1]["n_sites"].sum()) >= 30 and R.dirty_windows(buf, offsets, k) > 100   # (about 400 reads: sites at their ends; with ops = 6 and min_support = 2 fewer are tried)
        assert _same(m.seq_edit_flat(buf, offsets, thr, ms, ops), want), (thr, ms, ops)
        dev = _dev(m, buf, offsets, thr, ms, ops)
        assert _same(dev, want) and _applied(dev, buf, offsets, want[0]), (thr, ms, ops)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    sbuf, soff = R.flatten([reads[i] for i in range(0, len(reads), 5)])
    w_ed, w_rec, _ = E.oracle_edit(o, sbuf, soff, k, ci, 1, 7)
    assert _same(m.seq_edit_flat(sbuf, soff, ci, 1, 7), (w_ed, w_rec))


@pytest.mark.parametrize("name", SMALL)
def test_every_k_finds_real_edits(name):
    """joined k-mers have one solid window each, so no candidate ever passes there.  Here the model holds both strands of every
    window of a small genome (at k > 32 the two strands of a k-mer hash apart), the reads are cut from it with substitutions,
    lost and surplus bases: edits of every kind pass through the one- and the two-word window packing"""
    _, k, ci, cs, nh, nb, _ = CASE[name]
    n_bases = 20000
    g = R.genome_ascii(n_bases)
    fwd = synth.from_strings([np.lib.stride_tricks.sliding_window_view(g, k).tobytes().decode()], k)
    km = synth.sort_unique(np.concatenate([fwd, synth.revcomp(fwd, k)]))
    cnt = synth.d1_counts(len(km), ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    reads, _ = ER.make_reads(n_bases, k, n_reads=300, long_read=3000)
    buf, offsets = R.flatten(reads)
    want = _gpu_rule(m, buf, offsets, k, ci, 1)
    t = E.tallies(want[1], want[0])
    print(name, t)
    # of about 230 / 170 / 170 injected; a model with 3 hash functions and one array answers many absent k-mers, and at
    # 32 < k < 64 the reference's canonical form through one 64-bit word finds few k-mers of either strand: sites only
    assert t["n_sites"] > 100 and (32 < k < 64 or (t["n_sub"] >= 15 and t["n_del"] >= 5 and t["n_ins"] >= 5))
    assert _same(m.seq_edit_flat(buf, offsets, ci, 1), want)
    dev = _dev(m, buf, offsets, ci, 1)
    assert _same(dev, want) and _applied(dev, buf, offsets, want[0])
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    sbuf, soff = R.flatten(reads[::5])
    w_ed, w_rec, _ = E.oracle_edit(o, sbuf, soff, k, ci, 1, 7)
    assert _same(m.seq_edit_flat(sbuf, soff, ci, 1), (w_ed, w_rec))


def _long_sequence(n_bases, n=3_000_000):
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(5)
    parts = []
    while sum(len(p) for p in parts) < n:
        p = ER.with_errors(g, rng)
        p[int(rng.integers(0, len(p) - 100)):][:50] = ord("n")
        parts.append(p)
    return np.concatenate(parts)[:n]


def test_small_chunks_give_the_same_result(monkeypatch):
    """KMX_SEQ_CHUNK_BASES (test hook): runs, sites and verification windows cross thousands of piece boundaries; one sequence of
    3 * 10^6 bases with indels and 2 * 10^4 reads; host and device variants give the bytes of the unhooked call"""
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    long_seq = _long_sequence(n_bases)
    reads, _ = ER.make_reads(n_bases, k, n_reads=20000, seed=31)
    for buf, offsets in [(long_seq, np.array([0, len(long_seq)], dtype=np.uint64)), R.flatten(reads)]:
        monkeypatch.delenv("KMX_SEQ_CHUNK_BASES", raising=False)
        plain = m.seq_edit_flat(buf, offsets, ci, 1)
        t = E.tallies(plain[1], plain[0])
        print(t)
        assert t["n_sub"] > 3000 and t["n_del"] > 2000 and t["n_ins"] > 2000 and np.all(plain[0][1:] > plain[0][:-1])
        dev = _dev(m, buf, offsets, ci, 1)
        assert _same(dev, plain) and _applied(dev, buf, offsets, plain[0])
        for chunk in ("4099", "65536"):
            monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
            assert _same(m.seq_edit_flat(buf, offsets, ci, 1), plain), chunk
            assert _same(_dev(m, buf, offsets, ci, 1, apply=False), plain), chunk


def test_empty_sequences_and_chunk_edges(monkeypatch):
    """empty sequences scattered between the reads, runs of them at multiples of the hooked chunk size, reads that end and
    start exactly on a chunk boundary with an indel in their last / first k bases, reads shorter than k at both ends"""
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    C = 4099
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(77)
    reads = [g[5:5 + k - 1].tobytes(), b"", g[40:40 + k - 3].tobytes()]
    total = sum(len(r) for r in reads)

    def add(r):
        nonlocal total
        reads.append(r)
        total += len(r)

    def read_of(ln):
        """ln bytes: a stretch of the genome with a lost base in its first k bases and a surplus one in its last k (or the other way round)"""
        if ln <= 2 * k + 2:
            a = int(rng.integers(0, n_bases - ln))
            return g[a:a + ln].tobytes()
        a = int(rng.integers(0, n_bases - ln - 1))
        r = g[a:a + ln].copy()                                                  # drop one, add one: ln bytes again
        lost, extra = int(rng.integers(1, k)), ln - 1 - int(rng.integers(1, k))
        if rng.random() < 0.5:
            lost, extra = extra, lost
        r = np.delete(r, lost)
        r = np.insert(r, min(extra, len(r)), R.ACGT[int(rng.integers(0, 4))])
        if rng.random() < 0.2:
            r[int(rng.integers(0, ln))] = ord("N")
        return r.tobytes()

    n_empty = 0
    for boundary in range(1, 40):
        while total + 400 < boundary * C:
            add(read_of(int(rng.integers(20, 300))))
            for _ in range(int(rng.integers(0, 40))):
                add(b"")
                n_empty += 1
        add(read_of(boundary * C - total))                                     # ends exactly on the chunk boundary,
        assert total == boundary * C
        for _ in range(1 + boundary % 5 * 700):                                # a run of empty sequences sits there,
            add(b"")
            n_empty += 1
        add(read_of(int(rng.integers(k, 500))))                                # and the next one starts on it
    reads += [g[900:900 + k - 1].tobytes(), b"", g[77:77 + 3].tobytes()]
    buf, offsets = R.flatten(reads)
    monkeypatch.delenv("KMX_SEQ_CHUNK_BASES", raising=False)
    want = _gpu_rule(m, buf, offsets, k, ci, 1)
    t = E.tallies(want[1], want[0])
    print(t)
    assert t["n_del"] > 150 and t["n_ins"] > 150 and n_empty > 10000
    assert _same(m.seq_edit_flat(buf, offsets, ci, 1), want)
    for chunk in (str(C), "65536"):
        monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
        assert _same(m.seq_edit_flat(buf, offsets, ci, 1), want), chunk
        dev = _dev(m, buf, offsets, ci, 1)
        assert _same(dev, want) and _applied(dev, buf, offsets, want[0]), chunk


def test_edges_and_errors():
    import ctypes
    import torch
    _, k, ci, cs, nh, nb, n_genome = GCASE["genome_k31_ci1"]
    m = KModel(ci, cs, nh, nb)
    buf = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    off1 = np.array([0, 160], dtype=np.uint64)
    ed = np.full(64, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rec = np.full(80, 0x5A, dtype=np.uint8).view(REC)
    n = ctypes.c_uint64(77)
    pn = ctypes.addressof(n)
    host = lambda o, n_seqs, thr, ms, ops: m.L.kmx_edit_seqs(m.h, buf.ctypes.data, o.ctypes.data, n_seqs, thr, ms, ops, ed.ctypes.data, 64, pn, rec.ctypes.data)
    devc = lambda thr, ms, ops: m.L.kmx_edit_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 160, thr, ms, ops, ed.ctypes.data, 64, pn, rec.ctypes.data)
    with pytest.raises(api.KmxError) as e:                                       # before the build
        m.seq_edit_flat(buf, off1, 1, 1)
    assert e.value.code == -4 and devc(1, 1, 7) == -4
    km, cnt = synth.genome_stream(n_genome, k, ci, cs)
    m.build_packed(k, km, cnt)
    # n_seqs = 0: nothing written, whatever else is passed
    assert m.L.kmx_edit_seqs(m.h, None, np.zeros(1, np.uint64).ctypes.data, 0, 1, 1, 7, None, 0, None, None) == 0
    assert m.L.kmx_edit_seqs_dev(m.h, None, None, 0, 0, 1, 1, 7, None, 0, None, None) == 0
    assert m.seq_edit([], 1)[0] == []
    # no bases: all-zero records, no edits
    e0, r0 = m.seq_edit_flat(buf, np.zeros(4, dtype=np.uint64), 1, 1)
    assert e0.shape == (0,) and E.same(r0, np.zeros(3, REC))
    d0 = _dev(m, buf[:0], np.zeros(4, dtype=np.uint64), 1, 1, apply=False)
    assert d0[0].shape == (0,) and E.same(d0[1], np.zeros(3, REC))
    m.set_profile(1)
    m.kernel_times(reset=True)
    for ops in (0, 8, -1):                                                       # ops outside 1 .. 7
        assert host(off1, 1, 1, 1, ops) == -1 and devc(1, 1, ops) == -1
    for ms in (0, 65, -1):                                                       # min_support outside [1, 64]
        assert host(off1, 1, 1, ms, 7) == -1 and devc(1, ms, 7) == -1
    for bad in ([1, 160], [0, 100, 90, 160], [0, 0, 160, 159]):                  # bad offsets on the host
        assert host(np.array(bad, dtype=np.uint64), len(bad) - 1, 1, 1, 7) == -1, bad
    assert m.L.kmx_edit_seqs(m.h, None, None, 1, 1, 1, 7, None, 0, None, None) == -1
    assert (ed == 0x5A5A5A5A5A5A5A5A).all() and (rec.view(np.uint8) == 0x5A).all() and n.value == 77
    assert sum(v["launches"] for v in m.kernel_times(reset=True).values()) == 0     # rejected before anything was launched
    for ms in (1, 64):
        want = _gpu_rule(m, buf, off1, k, 1, ms)
        assert _same(m.seq_edit_flat(buf, off1, 1, ms), want) and _same(_dev(m, buf, off1, 1, ms), want)
    times = m.kernel_times(reset=True)
    assert [c for c, v in times.items() if v["launches"]] == [api.KModel.KERNEL_CLASSES[6]]
    m.set_profile(0)
    # capacity one short: KMX_E_RANGE with the needed number and complete records, then success
    reads, _ = ER.make_reads(n_genome, k, n_reads=200, long_read=3000)
    rbuf, roff = R.flatten(reads)
    n_seqs = len(reads)
    want = _gpu_rule(m, rbuf, roff, k, 1, 1)
    need = len(want[0])
    assert need > 50 and _same(m.seq_edit_flat(rbuf, roff, 1, 1), want)
    small, r2 = np.zeros(need, dtype=np.uint64), np.zeros(n_seqs, REC)
    assert m.L.kmx_edit_seqs(m.h, rbuf.ctypes.data, roff.ctypes.data, n_seqs, 1, 1, 7, small.ctypes.data, need - 1, pn, r2.ctypes.data) == -5
    assert n.value == need and E.same(r2, want[1])
    assert m.L.kmx_edit_seqs(m.h, rbuf.ctypes.data, roff.ctypes.data, n_seqs, 1, 1, 7, small.ctypes.data, need, pn, r2.ctypes.data) == 0
    assert n.value == need and np.array_equal(small, want[0])
    # the device variants with guard bytes around d_edits / d_rec / d_seq_out; capacity one short there; then out-of-range,
    # decreasing and huge offsets: wrong output allowed, nothing outside the buffers
    guard = 256
    d_seq = torch.full((len(rbuf) + 2 * guard,), 0xEE, dtype=torch.uint8, device="cuda")
    d_seq[guard:-guard] = torch.from_numpy(rbuf).to("cuda")
    for kind in ("good", "one short", "past the end", "decreasing", "huge"):
        bad = roff.copy()
        if kind == "past the end":
            bad[n_seqs // 2:] += np.uint64(len(rbuf))
        elif kind == "decreasing":
            bad[1:-1] = bad[1:-1][::-1]
        elif kind == "huge":
            bad[3::7] = np.uint64(2**64 - 1)
        cap = need - 1 if kind == "one short" else len(rbuf) // 3 + 1
        d_off = torch.from_numpy(bad.view(np.int64)).to("cuda")
        d_ed = torch.full(((cap + 2 * 32) * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        d_rec = torch.full(((n_seqs + 2 * 16) * 80,), 0xFF, dtype=torch.uint8, device="cuda")
        if kind == "one short":
            with pytest.raises(api.KmxError) as e:
                m.seq_edit_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), 1, 1, 7, d_ed.data_ptr() + 32 * 8, cap, d_rec.data_ptr() + 16 * 80)
            assert e.value.code == -5 and e.value.needed == need
            n_ed = 0
        else:
            n_ed = m.seq_edit_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), 1, 1, 7, d_ed.data_ptr() + 32 * 8, cap, d_rec.data_ptr() + 16 * 80)
        d_out = torch.full((len(rbuf) + n_ed + 2 * guard,), 0xFF, dtype=torch.uint8, device="cuda")
        d_oo = torch.full(((n_seqs + 1 + 2 * 16) * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        m.apply_edits_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), d_ed.data_ptr() + 32 * 8, n_ed, d_out.data_ptr() + guard, len(rbuf) + n_ed, d_oo.data_ptr() + 16 * 8)
        torch.cuda.synchronize()
        he, hr, ho, hoo = d_ed.cpu().numpy(), d_rec.cpu().numpy(), d_out.cpu().numpy(), d_oo.cpu().numpy()
        assert (he[:32 * 8] == 0xFF).all() and (he[-32 * 8:] == 0xFF).all(), kind
        assert (hr[:16 * 80] == 0xFF).all() and (hr[-16 * 80:] == 0xFF).all(), kind
        assert (ho[:guard] == 0xFF).all() and (ho[-guard:] == 0xFF).all(), kind
        assert (hoo[:16 * 8] == 0xFF).all() and (hoo[-16 * 8:] == 0xFF).all(), kind
        r = hr[16 * 80:-16 * 80].view(REC)
        assert (r["n_windows"] <= len(rbuf)).all() and (r["n_weak"] <= r["n_windows"]).all(), kind        # every record was initialised
        if kind == "good":
            got = he[32 * 8:-32 * 8].view(np.uint64)[:n_ed]
            w_out, w_off = E.apply_edits(rbuf, roff, want[0])
            assert np.array_equal(got, want[0]) and E.same(r, want[1])
            assert np.array_equal(ho[guard:guard + len(w_out)], w_out) and np.array_equal(hoo[16 * 8:-16 * 8].view(np.uint64), w_off)
        if kind == "one short":
            assert E.same(r, want[1])
    # the device apply with its capacity one short: KMX_E_RANGE, nothing behind the capacity
    edits, _, w_out, w_off = _dev(m, rbuf, roff, 1, 1)
    grow = np.array([E.edit(5, E.INS, 0)], dtype=np.uint64)                         # a list that lengthens the output
    d_l = torch.from_numpy(grow.view(np.int64)).to("cuda")
    d_off = torch.from_numpy(roff.view(np.int64)).to("cuda")
    d_out = torch.full((len(rbuf) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(n_seqs + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(api.KmxError) as e:
        m.apply_edits_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), d_l.data_ptr(), 1, d_out.data_ptr(), len(rbuf), d_oo.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == -5 and (d_out.cpu().numpy()[len(rbuf):] == 0xFF).all()
    m.apply_edits_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), d_l.data_ptr(), 1, d_out.data_ptr(), len(rbuf) + 1, d_oo.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:len(rbuf) + 1], E.apply_edits(rbuf, roff, grow)[0])


def test_concurrent_callers_and_a_side_stream():
    import torch
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    reads, _ = ER.make_reads(n_bases, k, n_reads=3000, seed=101)
    buf, offsets = R.flatten(reads)
    occ = m.seq_to_occ_flat(buf, offsets)
    want = _gpu_rule(m, buf, offsets, k, ci, 1)
    errors = []

    def run(t):
        try:
            for _ in range(6):
                if t == 0:
                    assert _same(m.seq_edit_flat(buf, offsets, ci, 1), want)
                else:
                    assert np.array_equal(m.seq_to_occ_flat(buf, offsets), occ)
        except Exception as ex:  # noqa: BLE001
            errors.append((t, repr(ex)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    cap = len(buf) // 3 + 1
    with torch.cuda.stream(s):
        d_seq = torch.from_numpy(buf).to("cuda")
        d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda")
        d_ed = torch.full((cap * 8,), 0xFF, dtype=torch.uint8, device="cuda")
        d_rec = torch.full((len(reads) * 80,), 0xFF, dtype=torch.uint8, device="cuda")
    s.synchronize()
    for _ in range(2):
        n_ed = m.seq_edit_dev(d_seq.data_ptr(), d_off.data_ptr(), len(reads), len(buf), ci, 1, 7, d_ed.data_ptr(), cap, d_rec.data_ptr())
    s.synchronize()
    assert _same((d_ed.cpu().numpy().view(np.uint64)[:n_ed], d_rec.cpu().numpy().view(REC)), want)
    assert _same(m.seq_edit_flat(buf, offsets, ci, 1), want)


@pytest.mark.parametrize("k", [31, 55])
def test_allocation_failures(k, monkeypatch):
    """tests/test_gpu_alloc_failure.py's walk over seq_edit_flat on a freshly built handle: the model of a small genome's
    k-mers, reads of it with substitutions and indels"""
    import count_reads as CR
    g = R.genome_ascii(20000)
    km, cnt = CR.count(g, np.array([0, len(g)], dtype=np.uint64), k, 1, 1023)
    o = O.OracleModel(1, 1023, 7, 5)
    o.build(k, km, cnt)
    reads, _ = ER.make_reads(20000, k, n_reads=300, long_read=3000)
    buf, off = R.flatten(reads)
    w_ed, w_rec, _ = E.oracle_edit(o, buf, off, k, 1, 1, 7)
    assert w_rec["n_sites"].sum() > 100                            # (at k = 55 the two strands of a k-mer hash apart: sites are tried, none is fixed)
    # (edits that ARE made at k > 32, on models of as-asked listings: tests/test_gpu_two_word_seqs.py)
    assert k > 32 or (len(w_ed) > 50 and w_rec["n_del"].sum() > 10 and w_rec["n_ins"].sum() > 10)

    def fresh():
        m = KModel(1, 1023, 7, 5)
        m.build_packed(k, km, cnt)
        return m

    def call(m):
        try:
            return m.seq_edit_flat(buf, off, 1, 1)
        except api.KmxError as e:
            assert e.code == -6, e
            raise

    walk(monkeypatch, fresh, call, lambda m, got: _same(got, (w_ed, w_rec)) or pytest.fail("result differs"))


def test_device_result_has_the_golden_digest():
    sg = _golden()
    for name, e in sg["cases"].items():
        m, _, k, ci, n_bases = _genome_model(name, oracle=False)
        reads, _ = ER.make_reads(n_bases, k, **sg["recipe"])
        buf, offsets = R.flatten(reads)
        host = m.seq_edit_flat(buf, offsets, e["thr"], e["min_support"], e["ops"])
        dev = _dev(m, buf, offsets, e["thr"], e["min_support"], e["ops"])
        for ed, rec in (host, dev[:2]):
            assert E.sha(ed) == e["edits_sha256"] and E.sha(rec) == e["records_sha256"], name
        assert E.sha(dev[2]) == e["bases_sha256"] == E.sha(api.apply_edits(buf, offsets, host[0])[0]), name


def test_facade_seq_edit(tmp_path):
    """include/kmodel.hpp: seq_edit(read) and seq_edit(vector) against the rule over the GPU's own answers"""
    api.load_library()
    exe = str(tmp_path / "facade_seq_edit")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_edit.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    d = str(tmp_path / "model")
    os.makedirs(d)
    m.save(d)
    reads, _ = ER.make_reads(n_bases, k, n_reads=300, seed=77)
    with open(str(tmp_path / "reads.txt"), "wb") as f:
        f.write(b"\n".join(r if r else b"-" for r in reads) + b"\n")
    p = subprocess.run([exe, d, str(tmp_path / "reads.txt"), str(ci), "2", "7"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-500:]
    lines = p.stdout.split("\n")
    assert lines[len(reads)] == "ok"
    buf, offsets = R.flatten(reads)
    w_ed, w_rec = _gpu_rule(m, buf, offsets, k, ci, 2)
    w_out, w_off = E.apply_edits(buf, offsets, w_ed)
    assert int(w_rec["n_del"].sum()) > 20 and int(w_rec["n_ins"].sum()) > 20
    for i in range(len(reads)):
        f = lines[i].split(" ")
        assert f[0].encode("latin-1") == (w_out[int(w_off[i]):int(w_off[i + 1])].tobytes() or b"-"), i
        assert [int(x) for x in f[1:]] == [int(w_rec[i][n]) for n in E.FIELDS], i
