"""Models that answer at k > 32.  Above k = 32 a query canonicalises through ONE 64-bit word (quirk Q4, min_kmer in
kmcex_amd/csrc/device_common.h): a window is looked up as itself when its low word u satisfies u <= rc, otherwise as (0, rc).  A
listing of true canonical k-mers holds neither form for most windows of a text, so a model built from one finds almost nothing
again.  Here the listing is made from what the model WILL BE ASKED: the Q4 form of every forward window of a text.  On such a
model substitutions verify, indels are applied, walks run on and look ahead -- at two-word k.
The recipes of tests/test_two_word_models_cpu.py (which proves them good on the CPU oracle alone) and of
tests/test_gpu_two_word_seqs.py live here too, computed once and shared.  Not a test itself."""
import functools

import numpy as np

import count_reads as CR
import oracle_lib as O
import seq_correct_ref as S
import seq_edit_reads as ER
import seq_edit_ref as E
import seq_extend_ref as X
import seq_polish_ref as P
import seq_reads as R
from kmcex_amd import synth

# k: (ci, cs, nh, nb)
PARAMS = {32: (1, 1023, 7, 4), 33: (1, 1023, 7, 5), 34: (1, 1023, 7, 5), 35: (1, 1023, 7, 5), 55: (1, 4095, 9, 6), 63: (1, 4095, 9, 6),
          64: (1, 65535, 8, 3)}
N_GENOME, N_READS, LONG_READ = 20000, 400, 3000                 # the reads' recipe
N_TEXT, N_SEEDS, N_REVERSED, MAX_EXT = 6000, 600, 100, 200      # the seeds' recipe


def as_asked(km: np.ndarray, k: int) -> np.ndarray:
    """Q4 on packed two-word k-mers: [n, 2] uint64 (hi, lo) -> [n, 2], 33 <= k <= 64"""
    assert 33 <= k <= 64
    km = np.ascontiguousarray(km, dtype=np.uint64).reshape(-1, 2)
    lo = km[:, 1]
    s = 2 * (k - 32)
    if s >= 64:
        rc = np.full(len(lo), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    else:
        rc = (synth._rev2_u64(~lo) << np.uint64(s)) | np.uint64((1 << s) - 1)
    out = km.copy()
    other = lo > rc
    out[other, 0] = 0
    out[other, 1] = rc[other]
    return out


def forward_windows(buf: np.ndarray, offsets: np.ndarray, k: int) -> np.ndarray:
    """every clean window as it is read (no canonical form), packed [n, 2] (hi, lo); k > 32"""
    assert k > 32
    starts = CR.window_starts(buf, offsets, k)
    codes = CR.CODE[np.asarray(buf, dtype=np.uint8)].astype(np.uint64)
    hi = np.zeros(len(starts), dtype=np.uint64)
    lo = np.zeros(len(starts), dtype=np.uint64)
    for j in range(k):
        hi = (hi << np.uint64(2)) | (lo >> np.uint64(62))
        lo = (lo << np.uint64(2)) | codes[starts + j]
    return np.stack([hi, lo], axis=1)


def listing(seqs, k: int, ci: int, cs: int):
    """(k-mers ascending, uint32 counts) of a list of bytes.  k <= 32: count_reads.count (true canonical k-mers).  k > 32: the
    as_asked form of every clean window of every sequence as it is read -- the caller passes both strands when it wants
    both.  Kept where ci <= c, counts capped at cs."""
    buf, offsets = R.flatten(seqs)
    if k <= 32:
        return CR.count(buf, offsets, k, ci, cs)
    km = as_asked(forward_windows(buf, offsets, k), k)
    u, c = np.unique(km, axis=0, return_counts=True) if len(km) else (km.reshape(0, 2), np.zeros(0, np.int64))
    keep = c >= ci
    return np.ascontiguousarray(u[keep]), np.minimum(c[keep], cs).astype(np.uint32)


def text_with_alleles(n: int, seed: int, copies: int = 3, every: int = 150):
    """a seq_reads.genome_ascii(n, seed) genome plus `copies` copies of it, each with one substitution every `every` bases from a
    seeded offset in [40, every) on: most windows are in every copy, the others are the branches and joins of the graph.
    The offsets of the copies are step = (every - 40) // copies apart (36 by default): a window of at most `step` bases holds
    the site of one copy only, so it is in all the others (a window that two copies lack is below thr = 3 and ends every walk
    there).  -> list of bytes"""
    g = R.genome_ascii(n, seed)
    rng = np.random.default_rng(seed)
    out = [g.tobytes()]
    step = (every - 40) // copies
    first = int(rng.integers(40, every - (copies - 1) * step))
    for j in range(copies):
        c = g.copy()
        pos = np.arange(first + j * step, n, every)
        c[pos] = R.ACGT[(np.searchsorted(R.ACGT, c[pos]) + rng.integers(1, 4, size=len(pos))) % 4]
        out.append(c.tobytes())
    return out


def oracle_of(k: int, km: np.ndarray, cnt: np.ndarray) -> O.OracleModel:
    ci, cs, nh, nb = PARAMS[k]
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    return o


# ---------------------------------------------------------------- the reads' recipe: a genome with both strands
@functools.lru_cache(maxsize=None)
def genome_case(k: int) -> dict:
    """text: the genome and its reverse complement; km, cnt: their listing; o: the oracle built from it; reads / ereads: the
    reads with substitutions (seq_reads) and with indels too (seq_edit_reads), flat.  Computed once, shared, left unchanged."""
    ci, cs, _, _ = PARAMS[k]
    g = R.genome_ascii(N_GENOME).tobytes()
    text = [g, X.revcomp(g)]
    km, cnt = listing(text, k, ci, cs)
    reads = R.make_reads(N_GENOME, k, n_reads=N_READS, long_read=LONG_READ)
    ereads, truths = ER.make_reads(N_GENOME, k, n_reads=N_READS, long_read=LONG_READ)
    c = {"k": k, "text": text, "km": km, "cnt": cnt, "o": oracle_of(k, km, cnt), "reads": reads, "ereads": ereads, "truths": truths}
    c["buf"], c["off"] = R.flatten(reads)
    c["ebuf"], c["eoff"] = R.flatten(ereads)
    return c


@functools.lru_cache(maxsize=None)
def per_base(k: int, edit_reads: bool = False) -> np.ndarray:
    c = genome_case(k)
    return R.oracle_per_base(c["o"], c["ebuf" if edit_reads else "buf"], c["eoff" if edit_reads else "off"], k)


@functools.lru_cache(maxsize=None)
def want_correct(k: int, thr: int, ms: int):
    c = genome_case(k)
    return S.correct(per_base(k), c["buf"], c["off"], k, thr, ms, S.oracle_rows(c["o"], k))[:2]


@functools.lru_cache(maxsize=None)
def want_edit(k: int, thr: int, ms: int, ops: int):
    c = genome_case(k)
    return E.edit_seqs(per_base(k, True), c["ebuf"], c["eoff"], k, thr, ms, ops, S.oracle_rows(c["o"], k))[:2]


_polish_cache = {}


@functools.lru_cache(maxsize=None)
def want_polish(k: int, thr: int, ms: int, max_passes: int) -> dict:
    c = genome_case(k)
    return P.polish(P.oracle_fn(c["o"], k, thr, ms, 7, _polish_cache), c["ebuf"], c["eoff"], max_passes)


def chunk_subset(reads):
    """the long read and 100 reads: what the chunk-edge reruns take"""
    i = max(range(len(reads)), key=lambda j: len(reads[j]))
    return R.flatten([reads[i]] + [r for j, r in enumerate(reads) if j != i][:100])


# ---------------------------------------------------------------- the seeds' recipe: a genome and copies with alleles
@functools.lru_cache(maxsize=None)
def extend_case(k: int) -> dict:
    """text: text_with_alleles(6000, 100 + k); km, cnt: the listing of its sequences and their reverse complements (walks to
    the left and walks of reversed seeds find their k-mers too); o: the oracle; seeds: 600 stretches of k - 2 ... k + 40 bases of
    the first sequence, the reverse complements of 100 of them, an empty seed and one of k N"""
    ci, cs, _, _ = PARAMS[k]
    text = text_with_alleles(N_TEXT, 100 + k)
    km, cnt = listing(text + [X.revcomp(t) for t in text], k, ci, cs)
    rng = np.random.default_rng(100 + k)
    g = text[0]
    seeds = []
    for a in rng.integers(0, N_TEXT - k - 40, size=N_SEEDS).tolist():
        seeds.append(g[a:a + int(rng.integers(k - 2, k + 41))])
    seeds += [X.revcomp(s) for s in seeds[:N_REVERSED]] + [b"", b"N" * k]
    c = {"k": k, "text": text, "km": km, "cnt": cnt, "o": oracle_of(k, km, cnt), "seeds": seeds}
    c["buf"], c["off"] = R.flatten(seeds)
    return c


@functools.lru_cache(maxsize=None)
def want_extend(k: int, thr: int, depth: int):
    c = extend_case(k)
    return X.oracle_extend(c["o"], c["buf"], c["off"], k, thr, MAX_EXT, depth)[:2]
