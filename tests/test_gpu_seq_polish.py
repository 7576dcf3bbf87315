"""kmx_polish_seqs / kmx_polish_seqs_dev: reads polished to a fixed point on the device.  Reads, offsets_out, records and
passes_run must EQUAL, byte for byte, the host loop of the existing seq_edit and apply_edits entry points on the same model
(tests/seq_polish_ref.py drives it), and on the GENOME_CASES the fixture the CPU oracle made: every output is an integer or a
byte, there is no tolerance."""
import ctypes
import functools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import seq_edit_reads as ER
import seq_edit_ref as E
import seq_polish_ref as P
import seq_reads as R
from common import CASE, GENOME_CASES, SMALL
from kmcex_amd import KModel, api, synth
from test_gpu_alloc_failure import walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCASE = {c[0]: c for c in GENOME_CASES}
REC = api.SEQ_POLISH_DTYPE
GUARD = 256


@functools.lru_cache(maxsize=None)
def _genome_model(name):
    _, k, ci, cs, nh, nb, n_bases = GCASE[name]
    km, cnt = synth.genome_stream(n_bases, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    return m, k, ci, n_bases


@functools.lru_cache(maxsize=None)
def _reads_case(name):
    """the model and the recipe's 608 reads: computed once, shared, left unchanged"""
    m, k, ci, n_bases = _genome_model(name)
    reads, truths = ER.make_reads(n_bases, k, n_reads=600)
    return (m, k, ci, reads, truths) + R.flatten(reads)


def _loop(m, buf, offsets, thr, ms, ops, mp):
    """the host loop over the whole batch through the existing entry points"""
    return P.polish(lambda b, o: m.seq_edit_flat(b, o, thr, ms, ops), buf, offsets, mp, retire=False)


def _dev(m, buf, offsets, thr, ms, ops, mp, cap=None, records=True, n_bases=None):
    """the device variant on fresh device copies, every output between guard regions filled with 0xFF
    -> dict like the reference's, plus rc (0 or the KmxError's code)"""
    import torch
    n_seqs, n = len(offsets) - 1, len(buf) if n_bases is None else n_bases
    cap = n + n // 4 + 64 if cap is None else cap
    d_seq = torch.full((len(buf) + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    if len(buf):
        d_seq[GUARD:GUARD + len(buf)] = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to("cuda")
    d_out = torch.full((cap + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    d_oo = torch.full(((n_seqs + 1) * 8 + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    d_rec = torch.full((n_seqs * 96 + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    rc, passes = 0, None
    try:
        passes = m.seq_polish_dev(d_seq.data_ptr() + GUARD, d_off.data_ptr(), n_seqs, n, thr, ms, ops, mp, d_out.data_ptr() + GUARD, cap, d_oo.data_ptr() + GUARD,
                                  d_rec.data_ptr() + GUARD if records else 0)
    except api.KmxError as e:
        rc, passes = e.code, getattr(e, "passes_run", None)
    torch.cuda.synchronize()
    out, oo, rec = d_out.cpu().numpy(), d_oo.cpu().numpy(), d_rec.cpu().numpy()
    for a in (out, oo, rec):
        assert (a[:GUARD] == 0xFF).all() and (a[-GUARD:] == 0xFF).all(), "a guard region was written"
    assert np.array_equal(d_seq.cpu().numpy()[GUARD:GUARD + len(buf)], buf), "the input was written"
    oo = oo[GUARD:-GUARD].view(np.uint64)
    total = int(oo[-1]) if rc in (0, -5) else 0
    return {"bases": out[GUARD:GUARD + min(total, cap)], "tail": out[GUARD + min(total, cap):-GUARD], "offsets": oo, "records": rec[GUARD:GUARD + n_seqs * 96].view(REC),
            "passes_run": passes, "rc": rc}


def _host(m, buf, offsets, thr, ms, ops, mp):
    out, off, rec, passes = m.seq_polish_flat(buf, offsets, thr, ms, ops, mp)
    return {"bases": out, "offsets": off, "records": rec, "passes_run": passes}


def _same(got, want, records=True):
    return (np.array_equal(got["bases"], want["bases"]) and got["offsets"].dtype == np.uint64 and np.array_equal(got["offsets"], want["offsets"])
            and (not records or E.same(got["records"], want["records"])) and got["passes_run"] == want["passes_run"])


def _both(m, buf, offsets, thr, ms, ops, mp, want):
    dev = _dev(m, buf, offsets, thr, ms, ops, mp)
    assert dev["rc"] == 0 and (dev["tail"] == 0xFF).all() and _same(dev, want), ("dev", thr, ms, ops, mp)
    assert _same(_host(m, buf, offsets, thr, ms, ops, mp), want), ("host", thr, ms, ops, mp)


@pytest.mark.parametrize("name", [c[0] for c in GENOME_CASES])
def test_reads_match_the_loop_and_the_fixture(name):
    m, k, ci, reads, truths, buf, offsets = _reads_case(name)
    with open(os.path.join(ROOT, "tests", "golden", "seq_polish_golden.json")) as f:
        sg = json.load(f)["cases"][name]
    assert sg["n_reads"] == len(reads) == 608
    for ops, ms in ((7, 1), (1, 1), (7, 4), (1, 4)):
        for mp in (1, 2, 8):
            want = _loop(m, buf, offsets, ci, ms, ops, mp)
            print(name, ops, ms, mp, P.tallies(want, truths))
            _both(m, buf, offsets, ci, ms, ops, mp, want)
            if (ops, ms) == (7, 1):                                  # the CPU oracle's result
                g = sg["max_passes"][str(mp)]
                assert (E.sha(want["bases"]), E.sha(want["offsets"]), E.sha(want["records"])) == (g["bases_sha256"], g["offsets_sha256"], g["records_sha256"])
                assert want["passes_run"] == g["tallies"]["passes_run"]
            if ops == 1 and mp == 8:                                 # iterated kmx_correct_seqs
                x = buf
                for _ in range(want["passes_run"]):
                    x = m.seq_correct_flat(x, offsets, ci, ms)[0]
                assert np.array_equal(x, want["bases"]) and np.array_equal(want["offsets"], offsets)
    dev = _dev(m, buf, offsets, ci, 1, 7, 8, records=False)           # d_rec == NULL
    assert dev["rc"] == 0 and _same(dev, _loop(m, buf, offsets, ci, 1, 7, 8), records=False) and (dev["records"].view(np.uint8) == 0xFF).all()
    fixed, rec = m.seq_polish(reads, ci)                              # the list form, and one read
    want = _loop(m, buf, offsets, ci, 1, 7, 8)
    assert b"".join(fixed) == want["bases"].tobytes() and [len(f) for f in fixed] == np.diff(want["offsets"]).tolist() and E.same(rec, want["records"])
    i = int(np.argmax(want["records"]["n_passes"]))
    one, r1 = m.seq_polish(reads[i].decode("latin-1"), ci)
    assert one == fixed[i] != reads[i] and r1.tobytes() == want["records"][i].tobytes() and int(r1["n_passes"]) == 3


@pytest.mark.parametrize("name", SMALL)
def test_every_k(name):
    """one- and two-word k-mers: the model holds both strands of every window of a small genome, as
    test_gpu_seq_edit.test_every_k_finds_real_edits builds it"""
    _, k, ci, cs, nh, nb, _ = CASE[name]
    n_bases = 20000
    g = R.genome_ascii(n_bases)
    fwd = synth.from_strings([np.lib.stride_tricks.sliding_window_view(g, k).tobytes().decode()], k)
    km = synth.sort_unique(np.concatenate([fwd, synth.revcomp(fwd, k)]))
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, synth.d1_counts(len(km), ci, cs))
    reads, truths = ER.make_reads(n_bases, k, n_reads=300, long_read=3000)
    buf, offsets = R.flatten(reads)
    want = _loop(m, buf, offsets, ci, 1, 7, 8)
    t = P.tallies(want, truths)
    print(name, t)
    # judged on the LOOP's result: sites are tried and a second pass runs, so fold, compaction and apply all work on real edits
    # (a model with 3 hash functions and one array, or 32 < k < 64 where the two strands hash apart, fixes few of its sites)
    assert t["n_sites"] > 50 and t["passes_run"] >= 2 and t["edited_per_pass"][0] >= 1
    _both(m, buf, offsets, ci, 1, 7, 8, want)


def test_nothing_active_and_everything_active_in_pass_two():
    m, k, ci, reads, truths, buf, offsets = _reads_case("genome_k31_ci1")
    ref = _loop(m, buf, offsets, ci, 1, 7, 8)
    h = ref["history"]
    clean = [reads[i] for i in range(len(reads)) if i not in set(h[0]["edited"])]      # pass 1 finds nothing: no read is ever copied before the gather
    cbuf, coff = R.flatten(clean)
    want = _loop(m, cbuf, coff, ci, 1, 7, 8)
    assert len(clean) > 150 and want["passes_run"] == 1 and np.array_equal(want["bases"], cbuf)
    _both(m, cbuf, coff, ci, 1, 7, 8, want)
    busy = [reads[i] for i in h[0]["edited"]]                                            # every read goes on to pass 2
    bbuf, boff = R.flatten(busy)
    want = _loop(m, bbuf, boff, ci, 1, 7, 8)
    assert len(want["history"][1]["active"]) == len(busy) > 300 and want["passes_run"] == 3
    _both(m, bbuf, boff, ci, 1, 7, 8, want)
    twice = [reads[i] for i in h[1]["edited"]]                                           # ... and every read to pass 3
    tbuf, toff = R.flatten(twice)
    want = _loop(m, tbuf, toff, ci, 1, 7, 8)
    assert len(want["history"][2]["active"]) == len(twice) >= 20
    for mp in (1, 2, 3):
        _both(m, tbuf, toff, ci, 1, 7, mp, _loop(m, tbuf, toff, ci, 1, 7, mp))


def test_small_batches(monkeypatch):
    m, k, ci, reads, truths, buf, offsets = _reads_case("genome_k31_ci1")
    ref = _loop(m, buf, offsets, ci, 1, 7, 8)
    i3 = ref["history"][1]["edited"][0]
    long_i = max(range(len(reads)), key=lambda i: len(reads[i]))
    assert len(reads[long_i]) > 6900 and ref["records"]["n_passes"][long_i] >= 2
    short = [b"", reads[0][:k - 1], b"", b"", reads[1][:3], b""]
    for batch in ([reads[i3]], [reads[long_i]], short, [b"", reads[i3], b""]):
        bbuf, boff = R.flatten(batch)
        for mp in (1, 8):
            want = _loop(m, bbuf, boff, ci, 1, 7, mp)
            _both(m, bbuf, boff, ci, 1, 7, mp, want)
    want = _loop(m, *R.flatten(short), ci, 1, 7, 8)
    assert want["passes_run"] == 1 and want["records"]["converged"].all() and not want["records"]["n_windows"].any()
    # the piece size of the edit pipeline (test hook): runs and sites cross piece boundaries in every pass
    for chunk in ("4099", "300"):
        monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", chunk)
        _both(m, buf, offsets, ci, 1, 7, 8, ref)
    monkeypatch.delenv("KMX_SEQ_CHUNK_BASES")


def test_capacity_and_argument_errors():
    _, k, ci, cs, nh, nb, n_genome = GCASE["genome_k31_ci1"]
    _, _, _, reads, truths, rbuf, roff = _reads_case("genome_k31_ci1")
    m = KModel(ci, cs, nh, nb)
    buf = np.frombuffer(b"ACGT" * 40, dtype=np.uint8).copy()
    off1 = np.array([0, 160], dtype=np.uint64)
    out = np.full(400, 0x5A, dtype=np.uint8)
    oo = np.full(8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rec = np.full(96, 0x5A, dtype=np.uint8).view(REC)
    n = ctypes.c_uint64(77)
    pn = ctypes.addressof(n)

    def host(o, n_seqs, ms=1, ops=7, mp=8, seq=buf.ctypes.data, dst=out.ctypes.data, cap=400, poo=oo.ctypes.data):
        return m.L.kmx_polish_seqs(m.h, seq, o.ctypes.data if o is not None else None, n_seqs, 1, ms, ops, mp, dst, cap, poo, rec.ctypes.data, pn)

    def devc(ms=1, ops=7, mp=8, dst=out.ctypes.data, cap=400, poo=oo.ctypes.data):
        return m.L.kmx_polish_seqs_dev(m.h, buf.ctypes.data, off1.ctypes.data, 1, 160, 1, ms, ops, mp, dst, cap, poo, rec.ctypes.data, pn)

    assert host(off1, 1) == -4 and devc() == -4                                     # before the build
    km, cnt = synth.genome_stream(n_genome, k, ci, cs)
    m.build_packed(k, km, cnt)
    m.set_profile(1)
    m.kernel_times(reset=True)
    assert m.L.kmx_polish_seqs(m.h, None, np.zeros(1, np.uint64).ctypes.data, 0, 1, 1, 7, 8, None, 0, None, None, None) == 0    # n_seqs = 0: nothing written
    assert m.L.kmx_polish_seqs_dev(m.h, None, None, 0, 0, 1, 1, 7, 8, None, 0, None, None, None) == 0
    assert m.seq_polish([], 1)[0] == []
    for ops in (0, 8, -1):
        assert host(off1, 1, ops=ops) == -1 and devc(ops=ops) == -1
    for ms in (0, 65, -1):
        assert host(off1, 1, ms=ms) == -1 and devc(ms=ms) == -1
    for mp in (0, 17, -1):
        assert host(off1, 1, mp=mp) == -1 and devc(mp=mp) == -1
    for bad in ([1, 160], [0, 100, 90, 160], [0, 0, 160, 159]):                      # bad offsets on the host
        assert host(np.array(bad, dtype=np.uint64), len(bad) - 1) == -1, bad
    assert host(off1, 1, dst=buf.ctypes.data + 100) == -1 and host(off1, 1, dst=buf.ctypes.data - 300) == -1    # seq_out overlaps seq,
    assert host(off1, 1, dst=buf.ctypes.data) == -1 and devc(dst=buf.ctypes.data + 159, cap=10) == -1           # in place too
    assert host(None, 1) == -1 and host(off1, 1, poo=None) == -1 and host(off1, 1, seq=None) == -1 and host(off1, 1, dst=None) == -1 and devc(poo=None) == -1
    assert (out == 0x5A).all() and (oo == 0x5A5A5A5A5A5A5A5A).all() and (rec.view(np.uint8) == 0x5A).all() and n.value == 77
    assert sum(v["launches"] for v in m.kernel_times(reset=True).values()) == 0     # rejected before anything was launched
    # no bases: records of a converged empty read, offsets_out all 0
    empty = np.zeros(3, REC)
    empty["n_passes"], empty["converged"] = 1, 1
    o0, f0, r0, p0 = m.seq_polish_flat(buf, np.zeros(4, dtype=np.uint64), 1)
    assert o0.shape == (0,) and not f0.any() and E.same(r0, empty) and p0 == 1
    d0 = _dev(m, buf[:0], np.zeros(4, dtype=np.uint64), 1, 1, 7, 8)
    assert d0["rc"] == 0 and not d0["offsets"].any() and E.same(d0["records"], empty) and d0["passes_run"] == 1 and (d0["tail"] == 0xFF).all()
    m.kernel_times(reset=True)
    want = _loop(m, rbuf, roff, ci, 1, 7, 8)
    assert _same(_host(m, rbuf, roff, ci, 1, 7, 8), want)
    times = m.kernel_times(reset=True)
    assert [c for c, v in times.items() if v["launches"]] == [api.KModel.KERNEL_CLASSES[6]]
    m.set_profile(0)
    # out_capacity exact, then one byte short: KMX_E_RANGE, records and offsets complete, nothing behind the capacity
    need = len(want["bases"])
    assert need != len(rbuf)
    n_seqs = len(reads)
    for cap in (need, need - 1):
        dev = _dev(m, rbuf, roff, ci, 1, 7, 8, cap=cap)
        assert dev["rc"] == (0 if cap == need else -5) and (dev["tail"] == 0xFF).all()
        assert np.array_equal(dev["bases"], want["bases"][:cap]) and np.array_equal(dev["offsets"], want["offsets"]) and E.same(dev["records"], want["records"]) and dev["passes_run"] == 3
        h_out = np.full(need + 1, 0xFF, dtype=np.uint8)
        h_oo, h_rec = np.zeros(n_seqs + 1, np.uint64), np.zeros(n_seqs, REC)
        rc = m.L.kmx_polish_seqs(m.h, rbuf.ctypes.data, roff.ctypes.data, n_seqs, ci, 1, 7, 8, h_out.ctypes.data, cap, h_oo.ctypes.data, h_rec.ctypes.data, pn)
        assert rc == (0 if cap == need else -5) and n.value == 3 and (h_out[cap:] == 0xFF).all()
        assert np.array_equal(h_out[:cap], want["bases"][:cap]) and np.array_equal(h_oo, want["offsets"]) and E.same(h_rec, want["records"])


@pytest.mark.parametrize("kind", ["past the end", "decreasing", "huge", "one swapped"])
def test_bad_offsets_on_the_device_stay_inside_the_buffers(kind):
    """wrong results (or a refusal) are allowed; _dev checks the guard regions around every output and the input"""
    m, k, ci, reads, truths, buf, offsets = _reads_case("genome_k31_ci1")
    n_seqs = len(reads)
    bad = offsets.copy()
    if kind == "past the end":
        bad[n_seqs // 2:] += np.uint64(len(buf))
    elif kind == "decreasing":
        bad[1:-1] = bad[1:-1][::-1]
    elif kind == "huge":
        bad[3::7] = np.uint64(2**64 - 1)
    else:
        bad[[100, 101]] = bad[[101, 100]]
    for mp in (1, 8):
        dev = _dev(m, buf, bad, ci, 1, 7, mp)
        assert dev["rc"] in (0, -1, -5), dev["rc"]
    good = _dev(m, buf, offsets, ci, 1, 7, 8)                         # the handle is as good as before
    assert good["rc"] == 0 and _same(good, _loop(m, buf, offsets, ci, 1, 7, 8))


def test_concurrent_callers_and_a_side_stream():
    import torch
    _, k, ci, reads, truths, buf, offsets = _reads_case("genome_k27_ci2")
    m = _genome_model.__wrapped__("genome_k27_ci2")[0]                # a handle of its own: its stream changes
    occ = m.seq_to_occ_flat(buf, offsets)
    want = _loop(m, buf, offsets, ci, 1, 7, 8)
    errors = []

    def run(t):
        try:
            for _ in range(4):
                if t == 0:
                    assert _same(_host(m, buf, offsets, ci, 1, 7, 8), want)
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
    try:
        cap = len(buf) + 1000
        with torch.cuda.stream(s):
            d_seq = torch.from_numpy(buf).to("cuda")
            d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda")
            d_out = torch.full((cap,), 0xFF, dtype=torch.uint8, device="cuda")
            d_oo = torch.zeros(len(reads) + 1, dtype=torch.int64, device="cuda")
            d_rec = torch.full((len(reads) * 96,), 0xFF, dtype=torch.uint8, device="cuda")
        s.synchronize()
        for _ in range(2):
            passes = m.seq_polish_dev(d_seq.data_ptr(), d_off.data_ptr(), len(reads), len(buf), ci, 1, 7, 8, d_out.data_ptr(), cap, d_oo.data_ptr(), d_rec.data_ptr())
        s.synchronize()
        oo = d_oo.cpu().numpy().view(np.uint64)
        got = {"bases": d_out.cpu().numpy()[:int(oo[-1])], "offsets": oo, "records": d_rec.cpu().numpy().view(REC), "passes_run": passes}
        assert _same(got, want)
    finally:
        m.set_stream(0)
        torch.cuda.synchronize()
    assert _same(_host(m, buf, offsets, ci, 1, 7, 8), want)


def test_allocation_failures(monkeypatch):
    """tests/test_gpu_alloc_failure.py's walk over seq_polish_flat on a freshly built handle"""
    import count_reads as CR
    k = 31
    g = R.genome_ascii(20000)
    km, cnt = CR.count(g, np.array([0, len(g)], dtype=np.uint64), k, 1, 1023)
    reads, _ = ER.make_reads(20000, k, n_reads=300, long_read=3000)
    buf, off = R.flatten(reads)

    def fresh():
        m = KModel(1, 1023, 7, 5)
        m.build_packed(k, km, cnt)
        return m

    m0 = fresh()
    want = _loop(m0, buf, off, 1, 1, 7, 8)
    assert want["passes_run"] >= 2 and len(want["history"][1]["edited"]) >= 5

    def call(m):
        try:
            return _host(m, buf, off, 1, 1, 7, 8)
        except api.KmxError as e:
            assert e.code == -6, e
            raise

    walk(monkeypatch, fresh, call, lambda m, got: _same(got, want) or pytest.fail("result differs"))


def test_facade_seq_polish(tmp_path):
    """include/kmodel.hpp: seq_polish(read) and seq_polish(vector) against the loop of the existing entry points"""
    api.load_library()
    exe = str(tmp_path / "facade_seq_polish")
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_seq_polish.cpp"),
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    m, k, ci, n_bases = _genome_model("genome_k31_ci1")
    d = str(tmp_path / "model")
    os.makedirs(d)
    m.save(d)
    reads, _ = ER.make_reads(n_bases, k, n_reads=300, seed=77)
    with open(str(tmp_path / "reads.txt"), "wb") as f:
        f.write(b"\n".join(r if r else b"-" for r in reads) + b"\n")
    p = subprocess.run([exe, d, str(tmp_path / "reads.txt"), str(ci), "2", "7", "8"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-500:]
    lines = p.stdout.split("\n")
    assert lines[len(reads)] == "ok"
    buf, offsets = R.flatten(reads)
    want = _loop(m, buf, offsets, ci, 2, 7, 8)
    assert want["passes_run"] >= 2
    w_out, w_off, w_rec = want["bases"], want["offsets"], want["records"]
    for i in range(len(reads)):
        f = lines[i].split(" ")
        assert f[0].encode("latin-1") == (w_out[int(w_off[i]):int(w_off[i + 1])].tobytes() or b"-"), i
        assert [int(x) for x in f[1:]] == [int(w_rec[i][n]) for n in P.FIELDS], i
