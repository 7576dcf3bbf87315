"""kmx_count_* and kmx_build_from_reads on the MI355X: the listing against the numpy restatement of the counting rule
(tests/count_reads.py), the model against the CPU oracle built from that listing, and the file readers."""
import ctypes as C
import os

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_reads as R
from kmcex_amd import KModel
from kmcex_amd.api import KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing
GENOME = 6000
READS = {"n_reads": 1500, "seed": 41, "long_read": 2500}       # ~45x over GENOME: many counts above a small cs


def reads_for(k):
    return R.make_reads(GENOME, k, **READS)


def listing_equal(m, km, cnt):
    got_km, got_c = m.count_listing()
    assert got_km.shape == km.shape and np.array_equal(got_km, km), "listing k-mers differ"
    assert np.array_equal(got_c, cnt), "listing counts differ"


def model_arrays(m, nb):
    out = [m.download("km_back")]
    for a in range(nb):
        out += [m.download("tag", a), m.download("value", a)]
    for i in range(3):
        try:
            out += [m.download("bf", i), m.download("bf_back", i)]
        except KmxError:
            pass
    return out


def assert_same_model(m1, m2, nb):
    for x, y in zip(model_arrays(m1, nb), model_arrays(m2, nb)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("k", [16, 21, 27, 31, 32, 33, 55, 64, 4, 5, 7, 8, 11, 15])
@pytest.mark.parametrize("ci", [1, 2, 3])
def test_listing_matches_restatement(k, ci):
    cs = 20
    buf, off = R.flatten(reads_for(k))
    km, cnt = CR.count(buf, off, k, ci, cs)
    assert (cnt == cs).any() and len(km) > min(1000, 4 ** k // 4)      # (136 canonical 4-mers, 512 5-mers)
    m = KModel(ci, cs, NH, NB)
    m.count_begin(k)
    m.count_seqs(buf, off)
    assert m.count_finish() == len(km)
    listing_equal(m, km, cnt)
    assert m.stats().n_total == len(km)


def test_counts_sum_to_windows():
    for k in (31, 55):
        buf, off = R.flatten(reads_for(k))
        m = KModel(1, 65535, 7, 3)
        m.count_begin(k)
        m.count_seqs(buf, off)
        m.count_finish()
        km, cnt = m.count_listing()
        assert int(cnt.astype(np.int64).sum()) == len(CR.window_starts(buf, off, k))
        if km.ndim == 1:
            assert np.all(km[1:] > km[:-1]), "listing not strictly ascending"
        else:
            hi, lo = km[:, 0], km[:, 1]
            assert np.all((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))), "listing not strictly ascending"


@pytest.mark.parametrize("k,ci,cs,nh,nb", [(31, 1, 1023, 7, 5), (27, 2, 255, 7, 4), (55, 1, 4095, 9, 6), (21, 3, 1023, 7, 8)])
def test_model_equals_oracle(k, ci, cs, nh, nb):
    buf, off = R.flatten(reads_for(k))
    km, cnt = CR.count(buf, off, k, ci, cs)
    m = KModel(ci, cs, nh, nb)
    m.count_begin(k)
    m.count_seqs(buf, off)
    m.count_finish()
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    for a in range(nb):
        assert np.array_equal(m.download("tag", a), o.array_bytes("tag", a)), f"tag array {a}"
        assert np.array_equal(m.download("value", a), o.array_bytes("value", a)), f"value array {a}"
    assert np.array_equal(m.download("km_back"), o.array_bytes("km_back"))
    for i in range(1 if ci == 1 else 3):
        assert np.array_equal(m.download("bf", i), o.array_bytes("bf", i)), f"bf {i}"
        assert np.array_equal(m.download("bf_back", i), o.array_bytes("bf_back", i)), f"bf_back {i}"
    s, so = m.stats(), o.stats()
    for f in ("n_total", "n_km", "attempts", "successes", "rest_entries", "km_byte_size", "byte_km_back"):
        assert getattr(s, f) == getattr(so, f), f
    assert list(s.n_bf) == list(so.n_bf)
    # and the same as building from the listing directly
    m2 = KModel(ci, cs, nh, nb)
    m2.build_packed(k, km, cnt)
    assert_same_model(m, m2, nb)


@pytest.mark.parametrize("k", [31, 55])
def test_batches_pieces_and_device_input(k, monkeypatch):
    import torch
    ci, cs = 2, 20
    reads = reads_for(k)
    buf, off = R.flatten(reads)
    km, cnt = CR.count(buf, off, k, ci, cs)

    def run(batches, piece=None, dev=False):
        if piece:
            monkeypatch.setenv("KMX_COUNT_PIECE", str(piece))
        else:
            monkeypatch.delenv("KMX_COUNT_PIECE", raising=False)
        m = KModel(ci, cs, NH, NB)
        m.count_begin(k)
        cuts = np.linspace(0, len(reads), batches + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            bb, oo = R.flatten(reads[a:b])
            if dev:
                d_b = torch.from_numpy(bb).cuda()
                d_o = torch.from_numpy(oo.view(np.int64)).cuda()
                torch.cuda.synchronize()
                m.count_seqs_dev(d_b.data_ptr(), d_o.data_ptr(), len(oo) - 1, int(oo[-1]))
                torch.cuda.synchronize()
            else:
                m.count_seqs(bb, oo)
        m.count_finish()
        listing_equal(m, km, cnt)
        return m

    ref = run(1)
    for m in (run(2), run(7), run(1, piece=1000), run(7, piece=777), run(1, dev=True), run(3, piece=1500, dev=True)):
        assert_same_model(ref, m, NB)


def test_cap_state_and_arguments(tmp_path):
    k = 21
    m = KModel(1, 20, NH, NB)
    L = m.L
    # out of order
    assert L.kmx_count_seqs(m.h, b"ACGT", (C.c_uint64 * 2)(0, 4), 1) == -4
    assert L.kmx_count_finish(m.h, None) == -4
    assert L.kmx_count_seqs_dev(m.h, None, None, 1, 4) == -4
    n = C.c_uint64()
    assert L.kmx_count_listing(m.h, None, None, 0, C.byref(n)) == -4
    # one k-mer far above cs is listed at cs
    m.count_begin(k)
    m.count_seqs([b"A" * 500])
    # bad offsets: KMX_E_ARG before anything runs, and the session goes on
    assert L.kmx_count_seqs(m.h, b"ACGTACGT", (C.c_uint64 * 2)(1, 8), 1) == -1
    assert L.kmx_count_seqs(m.h, b"ACGTACGT", (C.c_uint64 * 3)(0, 6, 4), 2) == -1
    assert m.count_finish() == 1
    km, cnt = m.count_listing()
    assert km.tolist() == [0] and cnt.tolist() == [20]
    assert L.kmx_count_finish(m.h, None) == -4                  # the session ended with finish
    assert L.kmx_count_begin(m.h, 2) == -1 and L.kmx_count_begin(m.h, 65) == -1
    _k3_refused_everywhere(m, tmp_path)
    km, cnt = m.count_listing()                                  # the listing of the last finish is still there
    assert km.tolist() == [0] and cnt.tolist() == [20]


def _k3_refused_everywhere(m, tmp_path):
    """k = 3 (the reference's rest table is undefined there) is KMX_E_ARG at every entry point that builds, counts or loads a
    model, before anything is launched, and the model built before answers the same; k = 4 is taken"""
    from kmcex_amd import kmcdb
    import small_k as SK
    L = m.L
    q = np.array([0, 1, 5, 2 ** 42 - 1], dtype=np.uint64)
    before = m.kmer_to_occ_packed(q)
    st0 = m.stats()
    km3 = np.arange(10, dtype=np.uint64)
    cnt3 = np.ones(10, dtype=np.uint32)
    nbf = [10, 0, 0]
    CR.write_fastq(str(tmp_path / "r.fq"), [b"ACGTACGTAC"] * 3)
    # a KMC1 database whose header says k = 3 (write one of k = 4, then set the header's k)
    km4, cnt4 = SK.listing("k4_full")
    db = str(tmp_path / "db3")
    kmcdb.write_kmc1(db, km4, cnt4, 4, 1, 255)
    with open(db + ".kmc_pre", "r+b") as f:
        f.seek(-(8 + 64), os.SEEK_END)
        f.write((3).to_bytes(4, "little"))
    calls = {"begin": lambda: m.begin(3, nbf, 10),
             "build_dev": lambda: m.build_dev(3, 0, 0, 0),
             "build_host": lambda: m.build_packed(3, km3, cnt3),
             "count_begin": lambda: m.count_begin(3),
             "build_from_reads": lambda: m.init_reads(str(tmp_path / "r.fq"), 3),
             "build_from_kmc": lambda: m.init(db),
             "shard_begin (ring)": lambda: m.shard_begin(3, nbf, 10, 0, 1),
             "range_begin": lambda: m.range_begin(3, nbf, 10, 0, 1)}
    for what, call in calls.items():
        with pytest.raises(KmxError) as e:
            call()
        assert e.value.code == -1 and "k=3" in str(e.value) and "rest table" in str(e.value), what
        assert np.array_equal(m.kmer_to_occ_packed(q), before), what
        st = m.stats()
        assert (st.k, st.n_total, st.rest_entries, st.km_byte_size) == (st0.k, st0.n_total, st0.rest_entries, st0.km_byte_size), what
    # kmx_load: a saved model whose rest.bin says k = 3, and one whose prefix is longer than k
    m4 = KModel(1, 255, 3, 1)
    m4.build_packed(4, km4, cnt4)
    (tmp_path / "m4").mkdir()
    m4.save(str(tmp_path / "m4"))
    m7 = KModel(1, 255, 3, 1)
    km7, cnt7 = SK.listing("k7_part")
    m7.build_packed(7, km7, np.minimum(cnt7, 255))
    (tmp_path / "m7").mkdir()
    m7.save(str(tmp_path / "m7"))
    for name, k_field, code in (("m4", 3, -1), ("m7", 6, -3)):
        with open(str(tmp_path / name / "rest.bin"), "r+b") as f:
            f.write(k_field.to_bytes(4, "little"))
        with pytest.raises(KmxError) as e:
            KModel.load(str(tmp_path / name))
        assert e.value.code == code, name
    # k = 4 is the smallest k a model or a session takes
    m4b = KModel(1, 20, NH, NB)
    m4b.count_begin(4)
    m4b.count_seqs([b"ACGTTT" * 5])
    assert m4b.count_finish() > 0
    assert KModel(1, 20, NH, NB).begin(4, [1, 0, 0], 1) is None


def test_nothing_listed_is_build_dev_of_nothing():
    k = 31
    m1, m2 = KModel(1, 1023, 7, 5), KModel(1, 1023, 7, 5)
    m1.count_begin(k)
    m1.count_seqs([b"ACGT" * 7, b"", b"NNNN" * 20])
    rc1 = m1.L.kmx_count_finish(m1.h, None)
    rc2 = m2.L.kmx_build_dev(m2.h, k, None, None, 0)
    assert rc1 == rc2
    if rc1 == 0:
        s1, s2 = m1.stats(), m2.stats()
        assert (s1.n_total, s1.rest_entries, s1.km_byte_size) == (s2.n_total, s2.rest_entries, s2.km_byte_size)
        n = C.c_uint64(7)
        assert m1.L.kmx_count_listing(m1.h, None, None, 0, C.byref(n)) == 0 and n.value == 0


def test_files(tmp_path, monkeypatch):
    k, ci, cs = 31, 2, 255
    reads = reads_for(k)
    buf, off = R.flatten(reads)
    km, cnt = CR.count(buf, off, k, ci, cs)
    ref = KModel(ci, cs, NH, NB)
    ref.count_begin(k)
    ref.count_seqs(buf, off)
    ref.count_finish()
    half = len(reads) // 2
    p = {n: str(tmp_path / n) for n in ("a.fq", "a.fa", "a.fq.gz", "crlf.fq", "crlf.fa", "h1.fa.gz", "h2.fq", "list")}
    CR.write_fastq(p["a.fq"], reads)
    CR.write_fasta(p["a.fa"], reads, width=61)
    CR.write_fastq(p["a.fq.gz"], reads, gz=True)
    CR.write_fastq(p["crlf.fq"], reads, crlf=True)
    CR.write_fasta(p["crlf.fa"], reads, crlf=True)
    CR.write_fasta(p["h1.fa.gz"], reads[:half], gz=True)
    CR.write_fastq(p["h2.fq"], reads[half:])
    with open(p["list"], "w") as f:
        f.write(f"{p['h1.fa.gz']}\n\n{p['h2.fq']}\n")
    for src in ("a.fq", "a.fa", "a.fq.gz", "crlf.fq", "crlf.fa"):
        m = KModel(ci, cs, NH, NB)
        m.init_reads(p[src], k)
        listing_equal(m, km, cnt)
        assert_same_model(ref, m, NB)
    m = KModel(ci, cs, NH, NB)
    m.init_reads("@" + p["list"], k)
    listing_equal(m, km, cnt)
    assert_same_model(ref, m, NB)
    # records longer than a reader batch and a host chunk: single-line and multi-line FASTA
    monkeypatch.setenv("KMX_COUNT_PIECE", "1000")
    for width in (60, 100000):
        CR.write_fasta(p["a.fa"], reads, width=width)
        m = KModel(ci, cs, NH, NB)
        m.init_reads(p["a.fa"], k)
        listing_equal(m, km, cnt)
        assert_same_model(ref, m, NB)


def test_failed_session_keeps_the_model(tmp_path):
    k = 31
    buf, off = R.flatten(reads_for(k))
    m = KModel(1, 255, NH, NB)
    m.count_begin(k)
    m.count_seqs(buf, off)
    m.count_finish()
    q = CR.window_kmers(buf, off, k)[::5]
    before = m.kmer_to_occ_packed(q)
    bad = str(tmp_path / "cut.fq")
    CR.write_fastq(bad, reads_for(k)[:50])
    with open(bad, "rb") as f:
        data = f.read()
    with open(bad, "wb") as f:
        f.write(data[:len(data) - 200])                         # the last record loses its quality line
    with pytest.raises(KmxError) as e:
        m.init_reads(bad, k)
    assert e.value.code == -3 and "cut.fq" in str(e.value) and "record" in str(e.value)
    assert np.array_equal(m.kmer_to_occ_packed(q), before)
    # a gzip file cut short: what still decodes may well end on a whole record, and is a read error all the same
    cut_gz = str(tmp_path / "cut.fq.gz")
    CR.write_fastq(cut_gz, reads_for(k)[:400], gz=True)
    with open(cut_gz, "rb") as f:
        data = f.read()
    with open(cut_gz, "wb") as f:
        f.write(data[:len(data) // 2])
    with pytest.raises(KmxError) as e:
        m.init_reads(cut_gz, k)
    assert e.value.code == -3 and "cut.fq.gz" in str(e.value) and "read error" in str(e.value)
    assert np.array_equal(m.kmer_to_occ_packed(q), before)
    with pytest.raises(KmxError) as e:
        m.init_reads(str(tmp_path / "missing.fq"), k)
    assert e.value.code == -3
    assert np.array_equal(m.kmer_to_occ_packed(q), before)
    assert m.L.kmx_count_seqs(m.h, b"ACGT", (C.c_uint64 * 2)(0, 4), 1) == -4     # the failed session has ended


GOLDEN = CR.load_golden()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_model_files(name, tmp_path):
    """count -> build -> save gives the reference's files for these reads; so do init(db) on the KMC1 database of the
    same listing and kmx_build_from_reads on the reads as FASTQ"""
    from common import sha_file
    from kmcex_amd import kmcdb
    g = GOLDEN[name]
    k, ci, cs, nh, nb = g["k"], g["ci"], g["cs"], g["nh"], g["nb"]
    reads = R.make_reads(g["genome_bases"], k, **g["reads"])
    buf, off = R.flatten(reads)
    m = KModel(ci, cs, nh, nb)
    m.count_begin(k)
    m.count_seqs(buf, off)
    assert m.count_finish() == g["n_listed"]
    km, cnt = m.count_listing()
    assert CR.listing_sha(km, cnt) == g["listing_sha256"]
    kmcdb.write_kmc1(str(tmp_path / "db"), km, cnt, k, ci, cs)
    CR.write_fastq(str(tmp_path / "reads.fq"), reads)
    m_db, m_fq = KModel(ci, cs, nh, nb), KModel(ci, cs, nh, nb)
    m_db.init(str(tmp_path / "db"))
    m_fq.init_reads(str(tmp_path / "reads.fq"), k)
    for tag, mm in (("count", m), ("db", m_db), ("fastq", m_fq)):
        d = tmp_path / tag
        d.mkdir()
        mm.save(str(d))
        for f, h in g["files"].items():
            assert sha_file(str(d / f)) == h, (tag, f)


def test_driver_g_counts_fastq(tmp_path):
    """kmcEx -g: the FASTQ counted on the GPU, no KMC binary, the reference's model files"""
    import subprocess
    from common import sha_file
    from test_count_cpu import _compile
    name = "reads_k31_ci1"
    g = GOLDEN[name]
    reads = R.make_reads(g["genome_bases"], g["k"], **g["reads"])
    CR.write_fastq(str(tmp_path / "reads.fq"), reads)
    exe = _compile(tmp_path, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "kmcex_main.cpp"), "kmcEx")
    work = tmp_path / "work"
    work.mkdir()
    env = dict(os.environ, KMC_BIN="/nonexistent")
    p = subprocess.run([exe, "-g", f"-k{g['k']}", f"-nh{g['nh']}", f"-nb{g['nb']}", f"-ci{g['ci']}", f"-cs{g['cs']}",
                        str(tmp_path / "reads.fq"), str(tmp_path / "out"), str(work)], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    for f, h in g["files"].items():
        assert sha_file(str(work / "out" / f)) == h, f
    assert not any(x.name.startswith("out.kmc") for x in tmp_path.iterdir())    # no KMC database written
