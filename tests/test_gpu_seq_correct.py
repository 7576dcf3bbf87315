"""kmx_correct_seqs / kmx_correct_seqs_dev: substitution errors of reads corrected on the device.  Corrected bases and records
must EQUAL, byte for byte, the reference rule (tests/seq_correct_ref.py) driven by the CPU oracle and by the GPU's own
seq_to_occ_flat / kmer_to_occ_rows: every field is an integer and no decision depends on another, there is no tolerance."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle_lib as O
import seq_correct_ref as S
import seq_reads as R
from common import CASE, GENOME_CASES, SMALL
from kmcex_amd import KModel, api, synth
from test_gpu_alloc_failure import walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCASE = {c[0]: c for c in GENOME_CASES}
REC = api.SEQ_CORRECTION_DTYPE


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


def _dev(m, buf, offsets, thr, ms, n_bases=None, records=True):
    """the device variant on fresh device copies; outputs pre-filled with 0xFF"""
    import torch
    n_seqs = len(offsets) - 1
    d_seq = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda") if len(buf) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda")
    d_out = torch.full((max(len(buf), 1),), 0xFF, dtype=torch.uint8, device="cuda")
    d_rec = torch.full((max(n_seqs, 1) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    m.seq_correct_dev(d_seq.data_ptr(), d_off.data_ptr(), n_seqs, len(buf) if n_bases is None else n_bases, thr, ms, d_out.data_ptr(),
                      d_rec.data_ptr() if records else 0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:len(buf)], d_rec.cpu().numpy()[:n_seqs * 64].view(REC)


def _gpu_rule(m, buf, offsets, k, thr, ms):
    """the reference rule over the GPU's own answers"""
    return S.correct(m.seq_to_occ_flat(buf, offsets), buf, offsets, k, thr, ms, lambda rows: m.kmer_to_occ_rows(rows, k))[:2]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and S.same(got[1], want[1])


@pytest.mark.parametrize("name", [c[0] for c in GENOME_CASES])
def test_reads_match_the_oracle(name):
    m, o, k, ci, n_bases = _genome_model(name)
    reads = R.make_reads(n_bases, k, n_reads=2000)
    buf, offsets = R.flatten(reads)
    with open(os.path.join(ROOT, "tests", "golden", "seq_correct_golden.json")) as f:
        sg = json.load(f)["cases"][name]
    for thr, ms in ((ci, 1), (ci, 4), (ci + 1, 1), (ci + 1, 4)):
        w_out, w_rec, _ = S.oracle_correct(o, buf, offsets, k, thr, ms)
        t = S.tallies(w_rec, buf, w_out, offsets)
        print(name, thr, ms, t)
        if (thr, ms) == (ci, 1):                                 # the data is not degenerate: judged on the ORACLE's result
            assert t["n_corrected"] >= 2000 and t["n_unfixable"] >= 500 and t["corrected_non_acgt"] >= 100 and t["reads_changed"] >= 1000
            assert t == sg["tallies"] and R.dirty_windows(buf, offsets, k) > 1000
        elif f"thr{thr}_ms{ms}" in sg["variants"]:
            assert t == sg["variants"][f"thr{thr}_ms{ms}"]
        got = m.seq_correct_flat(buf, offsets, thr, ms)
        assert got[0].dtype == np.uint8 and got[1].dtype == REC and got[1].shape == (len(reads),)
        assert _same(got, (w_out, w_rec)), (thr, ms)
        assert _same(_dev(m, buf, offsets, thr, ms), (w_out, w_rec)), (thr, ms)
        if (thr, ms) == (ci, 1):
            assert _same(_gpu_rule(m, buf, offsets, k, thr, ms), (w_out, w_rec))
            assert np.array_equal(_dev(m, buf, offsets, thr, ms, records=False)[0], w_out)        # d_rec == NULL
            fixed, rec = m.seq_correct(reads, thr, ms)               # the list form
            assert b"".join(fixed) == w_out.tobytes() and [len(f) for f in fixed] == [len(r) for r in reads] and S.same(rec, w_rec)
            i = max((j for j in range(len(reads)) if w_rec["n_corrected"][j]), key=lambda j: len(reads[j]))
            one, r1 = m.seq_correct(reads[i].decode("latin-1"), thr, ms)
            assert one == fixed[i] != reads[i] and r1.tobytes() == w_rec[i].tobytes()
            inplace = buf.copy()                                    # seq_out == seq on the host
            rec2 = np.zeros(len(reads), REC)
            assert m.L.kmx_correct_seqs(m.h, inplace.ctypes.data, offsets.ctypes.data, len(reads), thr, ms, inplace.ctypes.data, rec2.ctypes.data) == 0
            assert np.array_equal(inplace, w_out) and S.same(rec2, w_rec)


@pytest.mark.parametrize("name", SMALL)
def test_every_k_matches_the_existing_paths(name):
    """joined k-mers with substitutions and dirty bytes, k = 16 ... 64: against the rule over the GPU's own answers, a sample
    of the reads against the oracle"""
    _, k, ci, cs, nh, nb, n = CASE[name]
    km, cnt = synth.make_stream(n, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    rng = np.random.default_rng(k)
    strs = synth.to_ascii(km[rng.permutation(len(cnt))[:4000]], k)
    reads, cur = [], []
    for i, s in enumerate(strs):
        s = s.copy()
        if i % 3 == 0:                                             # a substitution inside a known k-mer
            p = int(rng.integers(0, k))
            s[p] = R.ACGT[(int(np.searchsorted(R.ACGT, s[p])) + int(rng.integers(1, 4))) % 4]
        if i % 13 == 5:
            s[int(rng.integers(0, k))] = ord("N") if i % 2 else ord("a")
        cur.append(s.tobytes())
        cur.append(R.ACGT[rng.integers(0, 4, size=int(rng.integers(0, 4)))].tobytes())
        if rng.random() < 0.1:
            reads.append(b"".join(cur))
            cur = []
    reads += [b"".join(cur), b"", strs[0].tobytes()[:k - 1], strs[1].tobytes()]
    buf, offsets = R.flatten(reads)
    for thr, ms in ((ci, 1), (ci + 2, 2)):
        want = _gpu_rule(m, buf, offsets, k, thr, ms)
        print(name, thr, ms, S.tallies(want[1], buf, want[0], offsets))
        assert int(want[1]["n_sites"].sum()) >= 100 and R.dirty_windows(buf, offsets, k) > 100
        assert _same(m.seq_correct_flat(buf, offsets, thr, ms), want), (thr, ms)
        assert _same(_dev(m, buf, offsets, thr, ms), want), (thr, ms)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    sample = np.arange(0, len(reads), 5)
    sbuf, soff = R.flatten([reads[i] for i in sample])
    w_out, w_rec, _ = S.oracle_correct(o, sbuf, soff, k, ci, 1)
    assert _same(m.seq_correct_flat(sbuf, soff, ci, 1), (w_out, w_rec))


def _long_sequence(n_bases, n=3_000_000):
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(5)
    parts = []
    while sum(len(p) for p in parts) < n:
        p = g.copy()
        subs = np.nonzero(rng.random(len(p)) < 0.01)[0]
        p[subs] = R.ACGT[rng.integers(0, 4, size=len(subs))]
        p[int(rng.integers(0, len(p) - 100)):][:50] = ord("n")
        parts.append(p)
    return np.concatenate(parts)[:n]


def test_small_chunks_give_the_same_result(monkeypatch):
    """KMX_SEQ_CHUNK_BASES (test hook): runs, sites and verification ranges cross thousands of piece and chunk boundaries; one
    sequence of 3 * 10^6 bases and 2 * 10^4 reads; host and device variants"""
    m, o, k, ci, n_bases = _genome_model("genome_k31_ci1")
    long_seq = _long_sequence(n_bases)
    reads = R.make_reads(n_bases, k, n_reads=20000, seed=31)
    for buf, offsets in [(long_seq, np.array([0, len(long_seq)], dtype=np.uint64)), R.flatten(reads)]:
        monkeypatch.delenv("KMX_SEQ_CHUNK_BASES", raising=False)
        plain = m.seq_correct_flat(buf, offsets, ci, 1)
        w_out, w_rec, _ = S.oracle_correct(o, buf, offsets, k, ci, 1)
        assert int(w_rec["n_corrected"].sum()) > 10000
        assert _same(plain, (w_out, w_rec))
        assert _same(_dev(m, buf, offsets, ci, 1), plain)
        for chunk in ("4099", "65536"):
            monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
            assert _same(m.seq_correct_flat(buf, offsets, ci, 1), plain), chunk
            assert _same(_dev(m, buf, offsets, ci, 1), plain), chunk


def test_empty_sequences_and_chunk_edges(monkeypatch):
    """empty sequences scattered between the reads, runs of them at multiples of the hooked chunk size, reads that end and
    start exactly on a chunk boundary (with an error in their last / first k bases), reads shorter than k at both ends"""
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
        a = int(rng.integers(0, n_bases - ln))
        r = g[a:a + ln].copy()
        if ln > 40:
            for p in (int(rng.integers(0, ln)), int(rng.integers(0, min(k, ln))), ln - 1 - int(rng.integers(0, min(k, ln)))):
                r[p] = ord("N") if rng.random() < 0.2 else R.ACGT[(int(np.searchsorted(R.ACGT, r[p])) + 1) % 4]
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
    assert int(want[1]["n_corrected"].sum()) > 500 and n_empty > 10000
    assert _same(m.seq_correct_flat(buf, offsets, ci, 1), want)
    for chunk in (str(C), "65536"):
        monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
        assert _same(m.seq_correct_flat(buf, offsets, ci, 1), want), chunk
        assert _same(_dev(m, buf, offsets, ci, 1), want), chunk


def test_edges_and_errors():
    import torch
    k, ci, cs, nh, nb = 31, 1, 1023, 7, 5
    m = KModel(ci, cs, nh, nb)
    buf = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    off1 = np.array([0, 160], dtype=np.uint64)
    out = np.full(160, 0x5A, dtype=np.uint8)
    rec = np.full(64, 0x5A, dtype=np.uint8).view(REC)
    with pytest.raises(api.KmxError) as e:                                       # before the build
        m.seq_correct_flat(buf, off1, 1, 1)
    assert e.value.code == -4
    assert m.L.kmx_correct_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 160, 1, 1, out.ctypes.data, None) == -4
    km, cnt = synth.make_stream(20000, k, ci, cs)
    m.build_packed(k, km, cnt)
    # n_seqs = 0: nothing written, whatever else is passed
    assert m.L.kmx_correct_seqs(m.h, None, np.zeros(1, np.uint64).ctypes.data, 0, 1, 1, None, None) == 0
    assert m.L.kmx_correct_seqs_dev(m.h, None, None, 0, 0, 1, 1, None, None) == 0
    assert m.seq_correct([], 1)[0] == []
    # no bases: all-zero records
    o0, r0 = m.seq_correct_flat(buf, np.zeros(4, dtype=np.uint64), 1, 1)
    assert o0.shape == (0,) and S.same(r0, np.zeros(3, REC))
    assert S.same(_dev(m, buf[:0], np.zeros(4, dtype=np.uint64), 1, 1)[1], np.zeros(3, REC))
    m.set_profile(1)
    m.kernel_times(reset=True)
    for ms in (0, 65, -1):                                                       # min_support outside [1, 64]
        assert m.L.kmx_correct_seqs(m.h, buf.ctypes.data, off1.ctypes.data, 1, 1, ms, out.ctypes.data, rec.ctypes.data) == -1
        assert m.L.kmx_correct_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 160, 1, ms, out.ctypes.data, rec.ctypes.data) == -1
    for bad in ([1, 160], [0, 100, 90, 160], [0, 0, 160, 159]):                  # bad offsets on the host
        o = np.array(bad, dtype=np.uint64)
        assert m.L.kmx_correct_seqs(m.h, buf.ctypes.data, o.ctypes.data, len(bad) - 1, 1, 1, out.ctypes.data, None) == -1, bad
    both = np.concatenate([buf, buf])                                            # overlap: only seq_out == seq is allowed on the host
    assert m.L.kmx_correct_seqs(m.h, both.ctypes.data, off1.ctypes.data, 1, 1, 1, both.ctypes.data + 10, None) == -1
    assert m.L.kmx_correct_seqs(m.h, both.ctypes.data + 10, off1.ctypes.data, 1, 1, 1, both.ctypes.data, None) == -1
    d = torch.from_numpy(both).to("cuda")
    d_off = torch.from_numpy(off1.view(np.int64)).to("cuda")
    for delta in (0, 10, 159):                                                   # any overlap on the device
        assert m.L.kmx_correct_seqs_dev(m.h, d.data_ptr(), d_off.data_ptr(), 1, 160, 1, 1, d.data_ptr() + delta, None) == -1
        assert m.L.kmx_correct_seqs_dev(m.h, d.data_ptr() + delta, d_off.data_ptr(), 1, 160, 1, 1, d.data_ptr(), None) == -1
    assert m.L.kmx_correct_seqs(m.h, None, None, 1, 1, 1, None, None) == -1
    assert (out == 0x5A).all() and (rec.view(np.uint8) == 0x5A).all()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), both)
    assert sum(v["launches"] for v in m.kernel_times(reset=True).values()) == 0     # rejected before anything was launched
    for ms in (1, 64):
        want = _gpu_rule(m, buf, off1, k, 1, ms)
        assert _same(m.seq_correct_flat(buf, off1, 1, ms), want) and _same(_dev(m, buf, off1, 1, ms), want)
    times = m.kernel_times(reset=True)
    assert [c for c, v in times.items() if v["launches"]] == [api.KModel.KERNEL_CLASSES[6]]
    m.set_profile(0)
    # the device variant with out-of-range, decreasing and huge offsets: wrong output allowed, nothing outside its three buffers
    reads = R.make_reads(20000, k, n_reads=200, long_read=3000)
    rbuf, roff = R.flatten(reads)
    n_seqs, guard = len(reads), 256
    d_seq = torch.full((len(rbuf) + 2 * guard,), 0xEE, dtype=torch.uint8, device="cuda")
    d_seq[guard:-guard] = torch.from_numpy(rbuf).to("cuda")
    for kind in ("past the end", "decreasing", "huge"):
        bad = roff.copy()
        if kind == "past the end":
            bad[n_seqs // 2:] += np.uint64(len(rbuf))
        elif kind == "decreasing":
            bad[1:-1] = bad[1:-1][::-1]
        else:
            bad[3::7] = np.uint64(2**64 - 1)
        d_off = torch.from_numpy(bad.view(np.int64)).to("cuda")
        d_out = torch.full((len(rbuf) + 2 * guard,), 0xFF, dtype=torch.uint8, device="cuda")
        d_rec = torch.full(((n_seqs + 2 * 16) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
        m.seq_correct_dev(d_seq.data_ptr() + guard, d_off.data_ptr(), n_seqs, len(rbuf), 1, 1, d_out.data_ptr() + guard, d_rec.data_ptr() + 16 * 64)
        torch.cuda.synchronize()
        h, hr = d_out.cpu().numpy(), d_rec.cpu().numpy()
        assert (h[:guard] == 0xFF).all() and (h[-guard:] == 0xFF).all(), kind
        assert (hr[:16 * 64] == 0xFF).all() and (hr[-16 * 64:] == 0xFF).all(), kind
        r = hr[16 * 64:-16 * 64].view(REC)
        assert (r["n_windows"] <= len(rbuf)).all() and (r["n_weak"] <= r["n_windows"]).all(), kind      # every record was initialised
        changed = h[guard:-guard] != rbuf
        assert np.isin(h[guard:-guard][changed], R.ACGT).all(), kind                                     # every base copied or corrected
    assert _same(_dev(m, rbuf, roff, 1, 1), _gpu_rule(m, rbuf, roff, k, 1, 1))


def test_concurrent_callers_and_a_side_stream():
    import torch
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    reads = R.make_reads(n_bases, k, n_reads=3000, seed=101)
    buf, offsets = R.flatten(reads)
    occ = m.seq_to_occ_flat(buf, offsets)
    want = _gpu_rule(m, buf, offsets, k, ci, 1)
    errors = []

    def run(t):
        try:
            for _ in range(6):
                if t == 0:
                    assert _same(m.seq_correct_flat(buf, offsets, ci, 1), want)
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
    with torch.cuda.stream(s):
        d_seq = torch.from_numpy(buf).to("cuda")
        d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda")
        d_out = torch.full((len(buf),), 0xFF, dtype=torch.uint8, device="cuda")
        d_rec = torch.full((len(reads) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    s.synchronize()
    for _ in range(2):
        m.seq_correct_dev(d_seq.data_ptr(), d_off.data_ptr(), len(reads), len(buf), ci, 1, d_out.data_ptr(), d_rec.data_ptr())
    s.synchronize()
    assert _same((d_out.cpu().numpy(), d_rec.cpu().numpy().view(REC)), want)
    assert _same(m.seq_correct_flat(buf, offsets, ci, 1), want)


@pytest.mark.parametrize("k", [31, 55])
def test_allocation_failures(k, monkeypatch):
    """tests/test_gpu_alloc_failure.py's walk over seq_correct_flat on a freshly built handle"""
    import test_gpu_alloc_failure as A
    o = A.case(k)[3]
    buf, off = R.flatten(R.make_reads(20000, k, n_reads=300, long_read=3000))
    w_out, w_rec, _ = S.oracle_correct(o, buf, off, k, 1, 1)

    def call(m):
        try:
            return m.seq_correct_flat(buf, off, 1, 1)
        except api.KmxError as e:
            assert e.code == A.KMX_E_NOMEM, e
            raise

    walk(monkeypatch, lambda: A.built(k), call, lambda m, got: _same(got, (w_out, w_rec)) or pytest.fail("result differs"))


def test_device_result_has_the_golden_digest():
    with open(os.path.join(ROOT, "tests", "golden", "seq_correct_golden.json")) as f:
        sg = json.load(f)
    for name, e in sg["cases"].items():
        m, _, k, ci, n_bases = _genome_model(name, oracle=False)
        buf, offsets = R.flatten(R.make_reads(n_bases, k, **sg["recipe"]))
        for out, rec in (m.seq_correct_flat(buf, offsets, e["thr"], e["min_support"]), _dev(m, buf, offsets, e["thr"], e["min_support"])):
            assert S.sha_bases(out) == e["bases_sha256"] and S.sha_records(rec) == e["records_sha256"], name


def test_facade_seq_correct(tmp_path):
    """include/kmodel.hpp: seq_correct(read) and seq_correct(vector) against the rule over the GPU's own answers"""
    api.load_library()
    exe = str(tmp_path / "facade_seq_correct")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_correct.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    m, _, k, ci, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    d = str(tmp_path / "model")
    os.makedirs(d)
    m.save(d)
    reads = [r for r in R.make_reads(n_bases, k, n_reads=300, seed=77)]
    with open(str(tmp_path / "reads.txt"), "wb") as f:
        f.write(b"\n".join(r if r else b"-" for r in reads) + b"\n")
    p = subprocess.run([exe, d, str(tmp_path / "reads.txt"), str(ci), "2"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-500:]
    lines = p.stdout.split("\n")
    assert lines[len(reads)] == "ok"
    buf, offsets = R.flatten(reads)
    w_out, w_rec = _gpu_rule(m, buf, offsets, k, ci, 2)
    assert int(w_rec["n_corrected"].sum()) > 100
    for i, r in enumerate(reads):
        f = lines[i].split(" ")
        assert f[0].encode("latin-1") == (w_out[int(offsets[i]):int(offsets[i + 1])].tobytes() or b"-"), i
        assert [int(x) for x in f[1:]] == [int(w_rec[i][n]) for n in S.FIELDS], i
