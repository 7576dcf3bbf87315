"""kmx_summarise_seqs / kmx_summarise_seqs_dev: the answers of kmx_query_seqs reduced per sequence on the device.  Every
record must EQUAL, byte for byte, the NumPy reduction (tests/seq_summary_ref.py) of the CPU oracle's per-base answers and of
kmx_query_seqs' own: all fields are integers, there is no tolerance."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle_lib as O
import seq_reads as R
import seq_summary_ref as S
from common import CASE, GENOME_CASES, SMALL
from kmcex_amd import KModel, api, synth
from test_gpu_alloc_failure import walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCASE = {c[0]: c for c in GENOME_CASES}
THR = (1, 3, 8)
REC = api.SEQ_SUMMARY_DTYPE


def _genome_model(name, oracle=True):
    _, k, ci, cs, nh, nb, n_bases = GCASE[name]
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    o = None
    if oracle:
        o = O.OracleModel(ci, cs, nh, nb)
        o.build(k, km, cnt)
    return m, o, k, n_bases


def _dev(m, buf, offsets, thr, n_bases=None, fill=0xFF):
    """the device variant on fresh device copies; d_out pre-filled with `fill` bytes"""
    import torch
    n_seqs = len(offsets) - 1
    d_seq = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda") if len(buf) else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda")
    d_out = torch.full((max(n_seqs, 1) * 64,), fill, dtype=torch.uint8, device="cuda")
    m.seq_summary_dev(d_seq.data_ptr(), d_off.data_ptr(), n_seqs, len(buf) if n_bases is None else n_bases, thr, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:n_seqs * 64].view(REC)


@pytest.mark.parametrize("name", [c[0] for c in GENOME_CASES])
def test_reads_match_the_oracle(name):
    m, o, k, n_bases = _genome_model(name)
    reads = R.make_reads(n_bases, k, n_reads=2000)
    buf, offsets = R.flatten(reads)
    want = S.summarise(R.oracle_per_base(o, buf, offsets, k), offsets, k, THR)
    # the data is not degenerate: judged on the ORACLE's records
    t = S.tallies(want)
    print(name, t, "dirty windows", R.dirty_windows(buf, offsets, k))
    assert t["all_known"] >= 200 and t["partly_known"] >= 1000
    assert t["median_reaches_thr1"] >= 100 and t["median_below_thr1"] >= 100 and t["median_reaches_thr2"] >= 20
    assert R.dirty_windows(buf, offsets, k) > 1000
    with open(os.path.join(ROOT, "tests", "golden", "seq_summary_golden.json")) as f:
        assert t == json.load(f)["tallies"][name]
    got = m.seq_summary_flat(buf, offsets, THR)
    assert got.dtype == REC and got.dtype.itemsize == 64 and got.shape == (len(reads),)
    assert S.same(got, want)
    assert S.same(got, S.summarise(m.seq_to_occ_flat(buf, offsets), offsets, k, THR))
    assert S.same(_dev(m, buf, offsets, THR), want)
    assert S.same(m.seq_summary(reads, THR), want)               # the list form
    one = max(reads, key=len)
    assert m.seq_summary(one.decode("latin-1"), THR).tobytes() == m.seq_summary(one, THR).tobytes() == want[reads.index(one)].tobytes()


@pytest.mark.parametrize("name", SMALL)
def test_every_k_matches_the_existing_paths(name):
    """the joined-k-mer reads and dirty bytes of test_gpu_seq_query.test_every_k_matches_the_existing_paths: k = 16 ... 64"""
    _, k, ci, cs, nh, nb, n = CASE[name]
    km, cnt = synth.make_stream(n, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    rng = np.random.default_rng(k)
    strs = synth.to_ascii(km[rng.permutation(len(cnt))[:4000]], k)
    reads, cur = [], []
    for i, s in enumerate(strs):
        cur.append(s.tobytes())
        cur.append(R.ACGT[rng.integers(0, 4, size=int(rng.integers(0, 4)))].tobytes())    # a random join
        if i % 13 == 5:
            cur.append(b"N" if i % 2 else b"a")
        if rng.random() < 0.1:
            reads.append(b"".join(cur))
            cur = []
    reads += [b"".join(cur), b"", strs[0].tobytes()[:k - 1], strs[1].tobytes()]
    buf, offsets = R.flatten(reads)
    thr = (1, ci + 2, 40)
    occ = m.seq_to_occ_flat(buf, offsets)
    want = S.summarise(occ, offsets, k, thr)
    assert int(want["n_ge"][:, 0].sum()) >= 2000 and R.dirty_windows(buf, offsets, k) > 100
    assert S.same(m.seq_summary_flat(buf, offsets, thr), want)
    assert S.same(_dev(m, buf, offsets, thr), want)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    sample = np.arange(0, len(reads), 5)                          # a sample of the reads against the oracle
    sbuf, soff = R.flatten([reads[i] for i in sample])
    assert S.same(want[sample], S.summarise(R.oracle_per_base(o, sbuf, soff, k), soff, k, thr))


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


def test_small_chunks_give_the_same_records(monkeypatch):
    """KMX_SEQ_CHUNK_BASES (test hook): thousands of chunk and piece boundaries; one sequence of 3 * 10^6 bases (every wave of
    every piece folds into ONE record) and 2 * 10^4 reads; host and device variants"""
    m, o, k, n_bases = _genome_model("genome_k31_ci1")
    long_seq = _long_sequence(n_bases)
    reads = R.make_reads(n_bases, k, n_reads=20000, seed=31)
    for buf, offsets in [(long_seq, np.array([0, len(long_seq)], dtype=np.uint64)), R.flatten(reads)]:
        monkeypatch.delenv("KMX_SEQ_CHUNK_BASES", raising=False)
        plain = m.seq_summary_flat(buf, offsets, THR)
        assert S.same(plain, S.summarise(R.oracle_per_base(o, buf, offsets, k), offsets, k, THR))
        assert S.same(_dev(m, buf, offsets, THR), plain)
        for chunk in ("4099", "65536"):
            monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
            assert S.same(m.seq_summary_flat(buf, offsets, THR), plain), chunk
            assert S.same(_dev(m, buf, offsets, THR), plain), chunk


def test_empty_sequences_and_chunk_edges(monkeypatch):
    """What rebased, deduplicated chunk boundaries would get wrong: 10^5 empty sequences scattered between the reads, runs of
    them exactly at multiples of the hooked chunk size, a sequence that starts on a chunk boundary, one that ends there,
    reads shorter than k at both ends of the batch"""
    m, _, k, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    C = 4099
    g = R.genome_ascii(n_bases)
    rng = np.random.default_rng(77)
    reads = [g[5:5 + k - 1].tobytes(), b"", g[40:40 + k - 3].tobytes()]          # shorter than k, at the front
    total = sum(len(r) for r in reads)

    def add(r):
        nonlocal total
        reads.append(r)
        total += len(r)

    def read_of(ln):
        a = int(rng.integers(0, n_bases - ln))
        r = g[a:a + ln].copy()
        if ln > 40 and rng.random() < 0.3:
            r[int(rng.integers(0, ln))] = ord("N")
        return r.tobytes()

    n_empty = 0
    for boundary in range(1, 40):
        while total + 400 < boundary * C:                                      # reads, with empty sequences scattered between them
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
    while n_empty < 100000:
        add(b"")
        n_empty += 1
    reads += [g[900:900 + k - 1].tobytes(), b"", g[77:77 + 3].tobytes()]        # shorter than k, at the back
    buf, offsets = R.flatten(reads)
    assert n_empty >= 100000 and len(buf) > 39 * C
    monkeypatch.delenv("KMX_SEQ_CHUNK_BASES", raising=False)
    want = S.summarise(m.seq_to_occ_flat(buf, offsets), offsets, k, THR)
    assert int((want["n_windows"] > 0).sum()) > 500 and int((want["first_below"] < want["n_windows"]).sum()) > 100
    assert S.same(m.seq_summary_flat(buf, offsets, THR), want)
    for chunk in (str(C), "65536"):
        monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
        assert S.same(m.seq_summary_flat(buf, offsets, THR), want), chunk
        assert S.same(_dev(m, buf, offsets, THR), want), chunk


def test_edges_and_errors():
    import torch
    k, ci, cs, nh, nb = 31, 1, 1023, 7, 5
    m = KModel(ci, cs, nh, nb)
    buf = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    off1 = np.array([0, 160], dtype=np.uint64)
    with pytest.raises(api.KmxError) as e:                                       # before the build
        m.seq_summary_flat(buf, off1, THR)
    assert e.value.code == -4
    out = np.zeros(1, REC)
    assert m.L.kmx_summarise_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 4, None, 0, out.ctypes.data) == -4
    km, cnt = synth.make_stream(20000, k, ci, cs)
    m.build_packed(k, km, cnt)
    thr = np.array(THR + (9,), dtype=np.int32)
    # n_seqs = 0: nothing written, whatever else is passed
    assert m.seq_summary_flat(buf, np.array([0], dtype=np.uint64), THR).shape == (0,)
    assert m.L.kmx_summarise_seqs(m.h, None, np.zeros(1, np.uint64).ctypes.data, 0, None, 0, None) == 0
    assert m.L.kmx_summarise_seqs_dev(m.h, None, None, 0, 0, None, 0, None) == 0
    assert m.seq_summary([]).shape == (0,)
    # n_bases = 0: every record is the empty record
    empty = np.zeros(3, REC)
    empty["min"] = empty["max"] = -1
    assert S.same(m.seq_summary_flat(buf, np.zeros(4, dtype=np.uint64), THR), empty)
    assert S.same(_dev(m, buf[:0], np.zeros(4, dtype=np.uint64), THR), empty)
    assert S.same(m.seq_summary(["", "ACG", ""], THR)[[0, 2]], empty[:2])
    # n_thr = 0 and 3 give records; 4 and -1, and a null thr with n_thr > 0, are refused and write nothing
    occ = m.seq_to_occ_flat(buf, off1)
    for t in ((), (1,), THR, (8, 1, -5)):
        assert S.same(m.seq_summary_flat(buf, off1, t), S.summarise(occ, off1, k, t)), t
        assert S.same(_dev(m, buf, off1, t), S.summarise(occ, off1, k, t)), t
    m.set_profile(1)
    m.kernel_times(reset=True)
    out = np.full(1, 0x5A, dtype=np.uint8).repeat(64).view(REC)
    untouched = out.copy()
    for n_thr, tp in ((4, thr.ctypes.data), (-1, thr.ctypes.data), (1, None), (3, None)):
        assert m.L.kmx_summarise_seqs(m.h, buf.ctypes.data, off1.ctypes.data, 1, tp, n_thr, out.ctypes.data) == -1, (n_thr, tp)
        assert m.L.kmx_summarise_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 160, tp, n_thr, out.ctypes.data) == -1, (n_thr, tp)
    with pytest.raises(api.KmxError) as e:
        m.seq_summary_flat(buf, off1, (1, 2, 3, 4))
    assert e.value.code == -1
    # bad offsets on the host: refused before anything runs
    for bad in ([1, 160], [0, 100, 90, 160], [0, 0, 160, 159]):
        o = np.array(bad, dtype=np.uint64)
        big = np.full(len(bad) - 1, 0x5A, dtype=np.uint8).repeat(64).view(REC)
        assert m.L.kmx_summarise_seqs(m.h, buf.ctypes.data, o.ctypes.data, len(bad) - 1, thr.ctypes.data, 3, big.ctypes.data) == -1, bad
        assert (big.view(np.uint8) == 0x5A).all()
    assert m.L.kmx_summarise_seqs(m.h, None, None, 1, None, 0, None) == -1
    assert S.same(out, untouched)
    assert sum(v["launches"] for v in m.kernel_times(reset=True).values()) == 0     # rejected before anything was launched
    # ... and a good call is timed as kernel class 6 (query)
    m.seq_summary_flat(buf, off1, THR)
    times = m.kernel_times(reset=True)
    assert [c for c, v in times.items() if v["launches"]] == [api.KModel.KERNEL_CLASSES[6]]
    m.set_profile(0)
    # the device variant with out-of-range and decreasing offsets: wrong records allowed, but nothing outside d_out[0, n_seqs)
    _, _, _, _, _, _, gb = GCASE["genome_k31_ci1"]
    reads = R.make_reads(20000, k, n_reads=200, long_read=3000)
    rbuf, roff = R.flatten(reads)
    n_seqs, guard = len(reads), 16
    d_seq = torch.from_numpy(rbuf).to("cuda")
    for kind in ("past the end", "decreasing", "huge"):
        bad = roff.copy()
        if kind == "past the end":
            bad[n_seqs // 2:] += np.uint64(len(rbuf))
        elif kind == "decreasing":
            bad[1:-1] = bad[1:-1][::-1]
        else:
            bad[3::7] = np.uint64(2**64 - 1)
        d_off = torch.from_numpy(bad.view(np.int64)).to("cuda")
        d_all = torch.full(((n_seqs + 2 * guard) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
        m.seq_summary_dev(d_seq.data_ptr(), d_off.data_ptr(), n_seqs, len(rbuf), THR, d_all.data_ptr() + guard * 64)
        torch.cuda.synchronize()
        h = d_all.cpu().numpy()
        assert (h[:guard * 64] == 0xFF).all() and (h[-guard * 64:] == 0xFF).all(), kind
        rec = h[guard * 64:-guard * 64].view(REC)
        assert (rec["n_windows"] <= len(rbuf)).all() and (rec["n_ge"] <= rec["n_windows"][:, None]).all(), kind   # every record was initialised
    # good offsets on the same buffers: d_out pre-filled with 0xFF is overwritten
    assert S.same(_dev(m, rbuf, roff, THR), S.summarise(m.seq_to_occ_flat(rbuf, roff), roff, k, THR))


def test_concurrent_callers_and_a_side_stream():
    """two host threads on one handle, one summarising and one calling seq_to_occ_flat / kmer_to_occ; then the device variant
    on a side stream set with kmx_set_stream"""
    import torch
    m, _, k, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    reads = R.make_reads(n_bases, k, n_reads=3000, seed=101)
    buf, offsets = R.flatten(reads)
    rows = np.stack([np.frombuffer(r[:k], dtype=np.uint8) for r in reads if len(r) >= k])
    occ, ans = m.seq_to_occ_flat(buf, offsets), m.kmer_to_occ_rows(rows, k)
    want = S.summarise(occ, offsets, k, THR)
    assert S.same(m.seq_summary_flat(buf, offsets, THR), want)
    errors = []

    def run(t):
        try:
            for rep in range(6):
                if t == 0:
                    assert S.same(m.seq_summary_flat(buf, offsets, THR), want)
                elif rep % 2:
                    assert np.array_equal(m.seq_to_occ_flat(buf, offsets), occ)
                else:
                    assert np.array_equal(m.kmer_to_occ_rows(rows, k), ans)
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
        d_out = torch.full((len(reads) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    s.synchronize()
    for _ in range(2):
        m.seq_summary_dev(d_seq.data_ptr(), d_off.data_ptr(), len(reads), len(buf), THR, d_out.data_ptr())
    s.synchronize()
    assert S.same(d_out.cpu().numpy().view(REC), want)
    assert S.same(m.seq_summary_flat(buf, offsets, THR), want)    # the host variant on the side stream too


@pytest.mark.parametrize("k", [31, 55])
def test_allocation_failures(k, monkeypatch):
    """tests/test_gpu_alloc_failure.py's walk over seq_summary_flat on a freshly built handle"""
    import test_gpu_alloc_failure as A
    o = A.case(k)[3]
    buf, off = R.flatten(R.make_reads(20000, k, n_reads=300, long_read=3000))
    want = S.summarise(R.oracle_per_base(o, buf, off, k), off, k, THR)

    def call(m):
        try:
            return m.seq_summary_flat(buf, off, THR)
        except api.KmxError as e:
            assert e.code == A.KMX_E_NOMEM, e                        # (walk itself also lets KMX_E_NODEVICE pass)
            raise

    walk(monkeypatch, lambda: A.built(k), call, lambda m, got: S.same(got, want) or pytest.fail("records differ"))


def test_device_records_have_the_golden_digest():
    with open(os.path.join(ROOT, "tests", "golden", "seq_summary_golden.json")) as f:
        sg = json.load(f)
    m, _, k, n_bases = _genome_model(sg["case"], oracle=False)
    buf, offsets = R.flatten(R.make_reads(n_bases, k, **sg["recipe"]))
    got = m.seq_summary_flat(buf, offsets, sg["thr"])
    assert len(got) == sg["n_reads"]
    assert S.sha_records(got) == sg["records_sha256"]
    assert S.sha_records(_dev(m, buf, offsets, sg["thr"])) == sg["records_sha256"]


def test_facade_seq_summary(tmp_path):
    """include/kmodel.hpp: seq_summary(read) and seq_summary(vector) against a reduction of seq_to_occ's vectors"""
    api.load_library()
    exe = str(tmp_path / "facade_seq_summary")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_summary.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    m, _, k, n_bases = _genome_model("genome_k31_ci1", oracle=False)
    d = str(tmp_path / "model")
    os.makedirs(d)
    m.save(d)
    reads = R.make_reads(n_bases, k, n_reads=300, seed=77)
    with open(str(tmp_path / "reads.txt"), "wb") as f:
        f.write(b"\n".join(r if r else b"-" for r in reads) + b"\n")   # "-": an empty read
    p = subprocess.run([exe, d, str(tmp_path / "reads.txt")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-500:]
    assert p.stdout.split()[-1] == "ok"
