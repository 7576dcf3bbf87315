"""The rest-table lookup and build of the device against the CPU oracle, where the table is more than a sprinkle of rows.

Every query entry point asks the rest table first (rest_check, kernels.hip), and so does each neighbour candidate of the
disambiguation.  The device lookup is not the reference's binary search: a bucket index over the top F bits, a narrowing
loop for buckets of more than 4 rows, a table of "the next group's first row" and a literal replay of the search where that
table matches -- all of it claimed equal to KRestData::check_kmer, inclusive upper bound included.  Ordinary builds leave
about 1 % of the k-mers in the table, so no bucket is long, the inclusive bound never answers and no neighbour is a row.

Here: tables written by hand (tests/rest_tables.py; tests/test_rest_lookup_cpu.py asserts, without a GPU, that they do what
they claim) loaded through kmx_load for every suffix width the loader accepts, and tables of 7 000 to 30 000 rows -- and one
of 10^6 that outgrows the accumulator of the build -- from builds whose arrays are declared too small.  Answers are
integers: everything is compared bit for bit.
"""
import os
import random

import numpy as np
import pytest

import oracle_lib as O
import rest_tables as T
import seq_reads as R
from common import sha_file
from kmcex_amd import KModel, synth

pytestmark = pytest.mark.gpu
CI, CS, NH, NB = T.MODEL


@pytest.fixture(scope="session")
def rest_base(tmp_path_factory):
    return tmp_path_factory.mktemp("rest_tables_gpu")


def by_length(o, strs):
    """o.query_strings of strings of mixed lengths"""
    out = np.zeros(len(strs), dtype=np.int32)
    for ln in sorted({len(s) for s in strs}):
        idx = [i for i, s in enumerate(strs) if len(s) == ln]
        out[idx] = o.query_strings([strs[i] for i in idx])
    return out


def overlap_join(strs):
    """the strings in one sequence, each laid over the longest tail of the sequence so far that it starts with"""
    seq = strs[0]
    for s in strs[1:]:
        j = next(j for j in range(len(s) - 1, -1, -1) if seq.endswith(s[:j]))
        seq += s[j:]
    return seq


def row_sequences(t, k):
    """Sequences whose windows are rows: every row followed by 3 more bases, a few rows joined through their overlaps; then
    the same with N for some A's (N reads as A: the dirty-list kernel meets the rows) and with lower-case stretches."""
    rows = [T.to_str(v, k) for v in t["rows"]]
    clean = [s + "CGA"[i % 3:] + "CGA"[:i % 3] for i, s in enumerate(rows)]
    clean += [overlap_join(rows[i:i + 4]) for i in range(0, min(len(rows) - 4, 40), 4)] + [overlap_join(rows[-3:])]
    def sub(s, every, c):
        pos = [i for i, ch in enumerate(s) if ch == "A"][::every]
        b = bytearray(s.encode())
        for i in pos:
            b[i] = ord(c)
        return b.decode()
    with_n = [sub(s, 5, "N") for s in clean]
    lower = [sub(s, 3, "a") if i % 2 else s[:k // 2] + s[k // 2:].lower() for i, s in enumerate(clean)]
    return clean + with_n + lower


def check_seqs(m, o, seqs, k, dev=False):
    buf, offsets = R.flatten([s.encode() for s in seqs])
    want = R.oracle_per_base(o, buf, offsets, k)
    assert (want > 0).sum() >= len(seqs) // 3, "the windows do not meet the table"
    assert np.array_equal(m.seq_to_occ_flat(buf, offsets), want)
    got = m.seq_to_occ(seqs)
    assert all(np.array_equal(g, want[int(a):int(a) + len(g)]) for g, a in zip(got, offsets[:-1]))
    if dev:
        import torch
        d_seq = torch.from_numpy(buf).to("cuda")
        d_off = torch.from_numpy(offsets.view(np.int64)).to("cuda")
        d_out = torch.full((len(buf),), 7, dtype=torch.int32, device="cuda")
        m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), len(offsets) - 1, len(buf), d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want)


@pytest.mark.parametrize("k,pre_len", T.SHAPES)
def test_crafted_table(rest_base, tmp_path, k, pre_len):
    t = T.info(k, pre_len)
    d1, _ = T.model_dirs(rest_base, k, pre_len)
    m, o = KModel.load(d1), O.OracleModel.load(d1)
    assert m.stats().rest_entries == len(t["rows"])
    q = T.pack(t["queries"], k)
    want = o.query_packed(k, q)
    assert np.array_equal(m.kmer_to_occ_packed(q), want)
    clean = [T.to_str(v, k) for v in t["queries"]]
    assert np.array_equal(m.kmer_to_occ(clean), want)
    rows = clean[:len(t["rows"])]
    dirty = [d for s in rows for d in T.dirty_variants(s)]
    dwant = o.query_strings(dirty)
    assert (dwant != 0).sum() * 2 >= len(dirty)
    assert np.array_equal(m.kmer_to_occ(dirty), dwant)
    # lengths k - 1, k and k + 1 in one batch (a string has at most 64 characters: no k + 1 at k = 64)
    mixed = [s[:-1] if i % 3 == 0 else s + "ACGT"[i % 4] if i % 3 == 1 and k < 64 else s for i, s in enumerate(rows + dirty[::5] + clean[-200:])]
    assert np.array_equal(m.kmer_to_occ(mixed), by_length(o, mixed))
    check_seqs(m, o, row_sequences(t, k), k, dev=(k, pre_len) == (31, 7))
    # save: k_rest_expand made full k-mers of the suffix rows at load, k_rest_suffix_bytes cuts them up again
    d2 = str(tmp_path / "saved")
    os.makedirs(d2)
    m.save(d2)
    for f in ("header", "km.bin", "rest.bin"):
        assert sha_file(os.path.join(d2, f)) == sha_file(os.path.join(d1, f)), f
    assert np.array_equal(m.kmer_to_occ_packed(q), want)
    m.close()


@pytest.mark.parametrize("k,pre_len", [(31, 7), (55, 7)])
def test_degenerate_tables(rest_base, tmp_path, k, pre_len):
    """no row at all (pre_buffer = [0]), one row, one group that holds every row"""
    t = T.info(k, pre_len)
    sbits = 2 * (k - pre_len)
    one = [r for r in t["rows"] if T.canonical_u64(r, k) == r and r >> sbits][:1]
    rng = random.Random(k)
    grp = sorted({T._reachable_fix((5 << sbits) | rng.getrandbits(sbits), k, pre_len) for _ in range(300)})
    for tag, rows in (("none", []), ("one", one), ("group", grp)):
        counts = [3 + i % 1000 for i in range(len(rows))]
        d = T.model_dirs(rest_base, k, pre_len, rows, counts, tag=tag)[0]
        m, o = KModel.load(d), O.OracleModel.load(d)
        assert m.stats().rest_entries == len(rows)
        qi = list(rows) + [T.revcomp(v, k) for v in rows] + [v + s for v in rows for s in (-1, 1)]
        qi += [(v & ((1 << sbits) - 1)) | (p << sbits) for v in rows[:50] for p in (4, 6)] + t["queries"][-500:]
        q = T.pack(qi, k)
        want = o.query_packed(k, q)
        if rows:
            assert np.array_equal(want[:len(rows)], counts), "the rows are not reached"
        assert np.array_equal(m.kmer_to_occ_packed(q), want), tag
        d2 = str(tmp_path / tag)
        os.makedirs(d2)
        m.save(d2)
        assert sha_file(os.path.join(d2, "rest.bin")) == sha_file(os.path.join(d, "rest.bin")), tag
        assert np.array_equal(m.kmer_to_occ_packed(q), want), tag
        m.close()


# ---------------------------------------------------------------------------------------------- large tables from real builds
N_BASES = 60000
LARGE = [(21, 4), (31, 4), (31, 2), (31, 8), (32, 4), (33, 4), (39, 4), (55, 4), (63, 4), (64, 4)]      # k, 1 / declared fraction
_large = {}


def declared(cnt, frac):
    """class counts of pass 1 with the coupled class declared at 1 / frac of what is inserted: the arrays overflow"""
    n_bf = int((cnt == CI).sum())
    return [n_bf], n_bf + (len(cnt) - n_bf) // frac


def large_case(k, frac, tmp):
    """per shape, once: the stream, the oracle's build with the given declaration, its files, the queries and their answers"""
    if (k, frac) not in _large:
        km, cnt = synth.genome_stream(N_BASES, k, CI, CS) if k <= 32 else T.genome_stream2(N_BASES, k, CI, CS)
        n, W = len(cnt), (k + 31) // 32
        n_bf, total = declared(cnt, frac)
        o = O.OracleModel(CI, CS, NH, NB)
        o.build_declared(k, km, cnt, n_bf, total)
        d = os.path.join(str(tmp), f"large_k{k}_f{frac}")
        o.save(d)
        one = km.reshape(n, -1)
        nbs = T.neighbours_np(km, k)
        q = np.concatenate([one, synth.revcomp(km, k).reshape(n, -1), nbs[:, ::7].reshape(-1, W), synth.random_kmers(5000, k, seed_k=0xABCDEF0123).reshape(5000, -1)]).reshape(-1)
        if frac > 1:
            # what the comparison rests on, from the oracle's own files: a table that is a real share of the k-mers, and
            # stored k-mers whose de Bruijn neighbours are rows (the neighbour candidates then come from the table)
            # (a fifth of them -- a tenth at the mildest declaration, 1/2, which leaves 12 %)
            assert o.stats().rest_entries >= n // (5 if frac > 2 else 10)
            table = T.read_rest_bin(os.path.join(d, "rest.bin"))
            assert table["entries"] == o.stats().rest_entries
            rows = T.pack(table["rows"], k)
            hit = np.zeros(n, dtype=bool)
            for x in range(8):
                hit |= T.member_np(T.canonical_u64_np(nbs[x], k), rows, k)
            assert hit.sum() >= 1000
        _large[(k, frac)] = (km, cnt, o, d, q, o.query_packed(k, q))
    return _large[(k, frac)]


def check_build(m, k, frac, base, tmp_path, tag):
    km, cnt, o, d, q, want = large_case(k, frac, base)
    n = len(cnt)
    n_bf, total = declared(cnt, frac)
    m.begin(k, n_bf, total)
    cut = n // 3 + 7
    m.insert_batch(km.reshape(n, -1)[:cut].reshape(-1), cnt[:cut])
    m.insert_batch(km.reshape(n, -1)[cut:].reshape(-1), cnt[cut:])
    m.finish()
    st, so = m.stats(), o.stats()
    assert (st.attempts, st.successes, st.rest_entries) == (so.attempts, so.successes, so.rest_entries), tag
    assert np.array_equal(m.kmer_to_occ_packed(q), want), f"{tag}: answers"
    d2 = str(tmp_path / tag)
    os.makedirs(d2)
    m.save(d2)
    for f in ("header", "km.bin", "rest.bin"):
        assert sha_file(os.path.join(d2, f)) == sha_file(os.path.join(d, f)), f"{tag}: {f}"
    assert np.array_equal(m.kmer_to_occ_packed(q), want), f"{tag}: answers after save"
    if k <= 32:
        g = R.genome_ascii(N_BASES).copy()
        g[::997] = ord("N")
        offsets = np.array([0, len(g)], dtype=np.uint64)
        assert np.array_equal(m.seq_to_occ_flat(g, offsets), R.oracle_per_base(o, g, offsets, k)), f"{tag}: the genome as one sequence"


@pytest.mark.parametrize("k,frac", LARGE)
def test_large_table_from_an_overfilled_build(rest_base, tmp_path, k, frac):
    m = KModel(CI, CS, NH, NB)
    check_build(m, k, frac, rest_base, tmp_path, f"k{k}_declared_1_{frac}")
    check_build(m, k, 1, rest_base, tmp_path, f"k{k}_honest")           # a small table after a large one, through the accelerators
    m.close()


# ---------------------------------------------------------------------------------------------- growth of the accumulator
GROW_NB = 2


def test_rest_accumulator_grows(tmp_path):
    """kmx_begin reserves max(n_km / 8, 2 blk) + blk rows for the survivors, blk = nb 2^18; a build that leaves more than that
    makes ensure_rest_capacity allocate, copy and move -- and ends on a partial block with the stale-slot duplicate."""
    nb, k = GROW_NB, 31
    blk = nb << 18
    km, cnt = synth.make_stream(4 * blk + 5000, k, CI, CS, seed_k=77)
    cnt = np.maximum(cnt, 2).astype(np.uint32)              # everything into the coupled arrays
    n = len(cnt)
    n_bf, total = [0], n // 64
    o = O.OracleModel(CI, CS, NH, nb)
    o.build_declared(k, km, cnt, n_bf, total)
    so = o.stats()
    assert so.rest_entries > 3 * blk, "the reservation holds this table: nothing grows"
    m = KModel(CI, CS, NH, nb)
    m.begin(k, n_bf, total)
    cut = n // 2 + 11
    m.insert_batch(km[:cut], cnt[:cut])
    m.insert_batch(km[cut:], cnt[cut:])
    m.finish()
    st = m.stats()
    assert (st.attempts, st.successes, st.rest_entries) == (so.attempts, so.successes, so.rest_entries)
    q = np.concatenate([km[::n // 20000], synth.random_kmers(5000, k, seed_k=0xABCDEF0123)])
    want = o.query_packed(k, q)
    assert np.array_equal(m.kmer_to_occ_packed(q), want)
    d1, d2 = str(tmp_path / "g"), str(tmp_path / "o")
    os.makedirs(d1)
    m.save(d1)
    o.save(d2)
    for f in ("header", "km.bin", "rest.bin"):
        assert sha_file(os.path.join(d1, f)) == sha_file(os.path.join(d2, f)), f
    assert np.array_equal(m.kmer_to_occ_packed(q), want)
    m.close()
