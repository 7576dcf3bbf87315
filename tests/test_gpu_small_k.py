"""Small k on the MI355X: the reference's models of tests/golden/small_k_golden.json (k = 4 ... 15) built three ways, queries
on dirty strings and reads at small k against the CPU oracle, and reverse-complement palindromes counted once per window.

At k <= 7 the rest table's prefix is the whole k-mer (pre_len == k, a suffix field of 0 bits), at k <= 9 the (k-2)-mer hash
never reaches an 8-byte MurmurHash block, and the count's radix sorts run over 8 ... 30 key bits."""
import hashlib

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_reads as R
import small_k as SK
from common import sha_file
from kmcex_amd import KModel, kmcdb, synth

pytestmark = pytest.mark.gpu

GOLDEN = SK.load_golden()


def _assert_golden(m, g, k, km, d, tag):
    d.mkdir()
    m.save(str(d))
    for f, h in g["files"].items():
        assert sha_file(str(d / f)) == h, (tag, f)
    r = m.kmer_to_occ_packed(SK.queries(k, km))
    assert hashlib.sha256(r.astype("<i4").tobytes()).hexdigest() == g["occ_sha256"], tag
    st = m.stats()
    for f, v in g["stats"].items():
        assert (list(getattr(st, f)) if f == "n_bf" else getattr(st, f)) == v, (tag, f)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_three_builds(name, tmp_path):
    """build_packed, init(db) on the KMC1 database of the listing (k >= 8: at k <= 7 that database's prefix is the whole
    k-mer, which the KMC reader refuses) and count_seqs on reads whose listing it is: the reference's files and answers"""
    g = GOLDEN[name]
    _, k, ci, cs, nh, nb, draws, seed = SK.CASE[name]
    km, cnt = SK.listing(name)
    assert CR.listing_sha(km, cnt) == g["listing_sha256"]
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    _assert_golden(m, g, k, km, tmp_path / "packed", "packed")
    if k >= 8:
        kmcdb.write_kmc1(str(tmp_path / "db"), km, cnt, k, ci, cs)
        m_db = KModel(ci, cs, nh, nb)
        m_db.init(str(tmp_path / "db"))
        _assert_golden(m_db, g, k, km, tmp_path / "db_model", "db")
    buf, off = SK.reads_for_listing(km, cnt, k, ci, cs, seed)
    m_c = KModel(ci, cs, nh, nb)
    m_c.count_begin(k)
    m_c.count_seqs(buf, off)
    assert m_c.count_finish() == len(km)
    got_km, got_c = m_c.count_listing()
    assert np.array_equal(got_km, km) and np.array_equal(got_c, cnt)
    _assert_golden(m_c, g, k, km, tmp_path / "count", "count")


def _dirty_strings(km, k, rng, n=3000):
    """stored and random k-mers with N, lowercase and IUPAC bytes, and strings of other lengths (2, k - 1, k + 1)"""
    present = synth.to_ascii(km[rng.integers(0, len(km), size=n)], k)
    rand = synth.to_ascii(synth.random_kmers(n, k, seed_k=int(rng.integers(1, 1 << 30))), k)
    rows = np.concatenate([present, rand])
    out = []
    for i, r in enumerate(rows):
        r = r.copy()
        kind = i % 6
        if kind == 1:
            r[int(rng.integers(0, k))] = ord("N")
        elif kind == 2:
            r[int(rng.integers(0, k)):] += 32
        elif kind == 3:
            r[int(rng.integers(0, k))] = ord("RYKMSW"[int(rng.integers(0, 6))])
        s = r.tobytes().decode()
        if kind == 4:
            s = s[:-1]
        elif kind == 5:
            s = s + "ACGT"[i % 4]
        out.append(s)
    out += ["AC", "ac", "N" * k, "n" * k, "A" * (k - 1) + "N"]
    return out


@pytest.mark.parametrize("k,name", [(4, "k4_full"), (5, "k5_part"), (7, "k7_full"), (9, "k9"), (13, "k13")])
def test_dirty_strings_and_reads_match_the_oracle(k, name):
    _, k, ci, cs, nh, nb, draws, seed = SK.CASE[name]
    km, cnt = SK.listing(name)
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    rng = np.random.default_rng(100 + k)
    strs = _dirty_strings(km, k, rng)
    got = np.asarray(m.kmer_to_occ(strs), dtype=np.int32)
    by_len = {}
    for i, s in enumerate(strs):
        by_len.setdefault(len(s), []).append(i)
    want = np.zeros(len(strs), dtype=np.int32)
    for ln, idx in by_len.items():
        want[idx] = o.query_strings([strs[i] for i in idx])
    assert np.array_equal(got, want)
    assert (got[:3000:6] > 0).all()                             # clean stored k-mers are found
    reads = R.make_reads(6000, k, n_reads=800, long_read=2500, seed=k)
    buf, off = R.flatten(reads)
    got = m.seq_to_occ_flat(buf, off)
    assert np.array_equal(got, R.oracle_per_base(o, buf, off, k))
    assert R.dirty_windows(buf, off, k) > 100


def _palindromes(k, n, rng):
    half = synth.to_ascii(synth.random_kmers(n, k // 2, seed_k=int(rng.integers(1, 1 << 30))), k // 2)
    comp = np.frombuffer(b"TGCA", dtype=np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), half[:, ::-1])]
    return np.concatenate([half, comp], axis=1)


@pytest.mark.parametrize("k", [4, 16, 32, 34, 64])
def test_palindromes_are_counted_once_per_window(k):
    """reads stuffed with k-mers that are their own reverse complement (f == r): the forward / reverse tie of the canonical
    k-mer, in one word (k <= 32) and in two words with the full mask of the top word (k = 64)"""
    rng = np.random.default_rng(k)
    pal = _palindromes(k, 400, rng)
    reads = []
    for i in range(600):
        parts = []
        for _ in range(int(rng.integers(1, 6))):
            p = pal[int(rng.integers(0, len(pal)))].copy()
            if i % 7 == 3:
                p += 32
            parts.append(p.tobytes())
            parts.append(bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(0, 3)) if i % 2 else b"")
        reads.append(b"".join(parts))
    reads += [pal[0].tobytes()] * 9 + [pal[1].tobytes() + b"N" + pal[1].tobytes()]
    buf, off = R.flatten(reads)
    ci, cs = 1, 65535
    km, cnt = CR.count(buf, off, k, ci, cs)
    p_km = synth.from_strings([r.tobytes().decode() for r in pal[:2]], k)
    assert np.array_equal(synth.canonical(p_km, k), p_km)       # palindromes: their own canonical form
    m = KModel(ci, cs, 3, 2)
    m.count_begin(k)
    m.count_seqs(buf, off)
    assert m.count_finish() == len(km)
    got_km, got_c = m.count_listing()
    assert np.array_equal(got_km, km) and np.array_equal(got_c, cnt)
    idx = [int(np.nonzero(np.all(km.reshape(len(cnt), -1) == p_km.reshape(2, -1)[j], axis=1))[0][0]) for j in range(2)]
    assert cnt[idx[0]] >= 9 and cnt[idx[1]] >= 2
