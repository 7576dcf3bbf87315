"""The sweep of the partitioned bit-sets (k_bs_apply) at the shapes where a wide-load sweep can go wrong.

k_bs_apply reads a bin's tuples 16 bytes per lane, several loads in flight, and ORs a tile back 16 bytes per lane; single
tuples and single words remain at the ends: in front of the first 16-byte boundary of a bin's tuples (a capacity that is no
multiple of 4), behind the last whole piece (a count that is no multiple of 4), in bins of one or two words (tiny filters)
and in the partial last bin of a filter.  Every case builds through the Python API and compares km_back, every Bloom filter
and every back filter byte for byte with the CPU oracle's, and attempts / successes / rest entries with its statistics.

Everything here needs a real MI355X (`-m gpu`).  Bar: bit-exact.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS_BINS = 256

# k, ci, cs, nh, nb, draws
DEFAULT = (31, 1, 1023, 7, 5, 300000)
PARTIAL = (31, 1, 1023, 7, 5, 150037)                            # km_back: 10 183 words, 64 per bin, 7 in the last
THREE_CLASSES = (64, 2, 65535, 8, 3, 30000)
TWO_WORDS = (55, 1, 4095, 9, 6, 30000)
TINY = ((31, 1, 1023, 7, 5, 2300), (31, 1, 1023, 7, 5, 5800))      # ~2 000 and ~5 000 coupled k-mers


def _stream(cfg):
    from kmcex_amd import synth
    k, ci, cs, nh, nb, n = cfg
    return synth.make_stream(n, k, ci, cs, seed_k=90210, seed_c=90211)


def _filters(x, bf_num):
    """km_back, bf[i], bf_back[i] of a KModel or an OracleModel, as bytes"""
    get = x.download if hasattr(x, "download") else x.array_bytes
    out = {"km_back": get("km_back").tobytes()}
    for i in range(bf_num):
        out["bf%d" % i] = get("bf", i).tobytes()
        out["bf_back%d" % i] = get("bf_back", i).tobytes()
    return out


def _counters(st):
    return int(st.attempts), int(st.successes), int(st.rest_entries)


@functools.lru_cache(maxsize=None)
def _oracle(cfg):
    """the reference of a case, computed once: filters, counters, sizes"""
    import oracle_lib as O
    k, ci, cs, nh, nb, n = cfg
    km, cnt = _stream(cfg)
    o = O.OracleModel(ci, cs, nh, nb)
    o.build(k, km, cnt)
    so = o.stats()
    bf_num = sum(1 for i in range(3) if so.n_bf[i])
    ref = dict(filters=_filters(o, bf_num), counters=_counters(so), bf_num=bf_num, n_km=int(so.n_km), n_bf=[int(x) for x in so.n_bf],
               byte_km_back=int(so.byte_km_back), byte_bf=[int(x) for x in so.byte_bf], byte_bf_back=[int(x) for x in so.byte_bf_back])
    o.close()
    return ref


def _geometry(nwords):
    """what bs_geometry makes of a filter of nwords 32-bit words: log2 positions per bin, words per bin, bins used, words of the last"""
    wshift = 5
    while (BS_BINS << wshift) < nwords * 32:
        wshift += 1
    wpb = 1 << (wshift - 5)
    used = (nwords + wpb - 1) // wpb
    return wshift, wpb, used, nwords - (used - 1) * wpb


def _slab(ref):
    """the Bloom slab as the library lays it out: filters and back filters back to back, each padded by one word"""
    off, starts = 0, []
    for i in range(ref["bf_num"]):
        for nbytes in (ref["byte_bf"][i], ref["byte_bf_back"][i]):
            starts.append(off)
            off += (nbytes + 3) // 4 + 1
    return off, starts


def _build(cfg, model=None):
    from kmcex_amd import KModel
    k, ci, cs, nh, nb, n = cfg
    km, cnt = _stream(cfg)
    m = model if model is not None else KModel(ci, cs, nh, nb)
    m.build_packed(k, km, cnt)
    return m


def _check(m, ref, what=""):
    st = m.stats()
    assert st.bf_num == ref["bf_num"], what
    assert (int(st.byte_km_back), [int(x) for x in st.byte_bf], [int(x) for x in st.byte_bf_back]) == (ref["byte_km_back"], ref["byte_bf"], ref["byte_bf_back"]), what
    got = _filters(m, st.bf_num)
    for name, want in ref["filters"].items():
        assert got[name] == want, f"{what}{name} differs from the oracle's"
    assert _counters(st) == ref["counters"], what
    return got


def _check_deferred_and_direct(cfg, monkeypatch, **env):
    """the build through the partitioned bit-sets and the same build with plain atomics (KMX_KMB_DIRECT=1): both the oracle's"""
    ref = _oracle(cfg)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    a = _check(_build(cfg), ref, f"{env} ")
    monkeypatch.setenv("KMX_KMB_DIRECT", "1")
    b = _check(_build(cfg), ref, f"{env} direct ")
    monkeypatch.delenv("KMX_KMB_DIRECT")
    for name in env:
        monkeypatch.delenv(name)
    assert a == b


def test_default_geometry_small_model(monkeypatch):
    """One tile per bin, bins of 128 words -- far fewer than the 1024 threads, so most lanes have no piece of the tile --,
    thousands of tuples per bin.  The tuples of km_back are (nh - 2) per success: their total is no multiple of 4, so the bins'
    counts cannot all be (and counts of thousands, spread by a hash, are multiples of 4 in one bin of four)."""
    k, ci, cs, nh, nb, n = DEFAULT
    ref = _oracle(DEFAULT)
    wshift, wpb, used, last = _geometry((ref["byte_km_back"] + 3) // 4)
    assert wpb == 128 and used > 100
    tuples = ref["counters"][1] * (nh - 2)
    assert tuples % 4 != 0 and tuples // used > 2000
    slab_words, _ = _slab(ref)
    slab_tuples = sum(ref["n_bf"]) * (2 * nh - 3)
    wshift_s, wpb_s, used_s, _ = _geometry(slab_words)
    assert wpb_s <= 128 and slab_tuples % 4 != 0 and slab_tuples // used_s > 1000
    _check_deferred_and_direct(DEFAULT, monkeypatch)


@pytest.mark.parametrize("tlog2", [10, 13])
def test_small_tiles(tlog2, monkeypatch):
    """KMX_BS_TILE_LOG2 = 10: tiles of 32 words, four to a bin, so a tile meets tuples below and above it (the unsigned wrap
    of the word offset skips both) and the tile is cleared between two of them; 13: a tile of 256 words that the bin's 128
    fill by half."""
    ref = _oracle(DEFAULT)
    _, wpb, _, _ = _geometry((ref["byte_km_back"] + 3) // 4)
    assert (wpb // (1 << (tlog2 - 5)) == 4) if tlog2 == 10 else (wpb < (1 << (tlog2 - 5)))
    _check_deferred_and_direct(DEFAULT, monkeypatch, KMX_BS_TILE_LOG2=tlog2)


def _tiny_child(cap):
    """runs in a process of its own (KMX_BS_CAP is read once per process): both tiny models, deferred and direct"""
    os.environ["KMX_BS_CAP"] = str(cap)
    os.environ["KMX_TEST_HOOKS"] = "1"
    report = []
    for cfg in TINY:
        ref = _oracle(cfg)
        for direct in (0, 1):
            os.environ["KMX_KMB_DIRECT"] = str(direct)
            _check(_build(cfg), ref, f"cap {cap} n {cfg[5]} direct {direct}: ")
        report.append(dict(n_km=ref["n_km"], successes=ref["counters"][1]))
    print(json.dumps(report))


@pytest.mark.parametrize("cap", [64, 66, 65])
def test_tiny_filters_overflowing_bins(cap):
    """~2 000 and ~5 000 coupled k-mers: km_back has one and two words per bin (no 16-byte boundary inside a bin: the words go
    one by one).  KMX_BS_CAP forces these filters onto the deferred path with bins of `cap` tuples, which overflow: the
    producers set the rest with atomics and the sweep meets counts above the capacity.  With 66 (the hook takes any capacity) the
    tuples of odd bins start 8 bytes behind a 16-byte boundary, with 65 at every offset: single tuples in front.  The hook is
    read once per process, so each capacity runs in a process of its own."""
    nh = TINY[0][3]
    for cfg, words, fill in zip(TINY, (1, 2), (0.95, 1.9)):
        ref = _oracle(cfg)
        wshift, wpb, used, _ = _geometry((ref["byte_km_back"] + 3) // 4)
        assert wpb == words
        # a model of one block emits all its tuples between two sweeps.  Two words per bin: about twice what the bins of 64 take,
        # so bins must overflow; one word per bin: as many as they take, so the fuller half of the bins does
        assert ref["counters"][1] * (nh - 2) > fill * used * 64
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tiny-child", str(cap)], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert [x["n_km"] for x in json.loads(r.stdout.strip().splitlines()[-1])] == [_oracle(cfg)["n_km"] for cfg in TINY]


def test_partial_last_bin(monkeypatch):
    """The last used bin of km_back is partial and its words are no multiple of 4: whole 16-byte pieces, then single words, and
    nothing at or beyond the end of the filter."""
    ref = _oracle(PARTIAL)
    nwords = (ref["byte_km_back"] + 3) // 4
    _, wpb, used, last = _geometry(nwords)
    assert wpb >= 4 and last < wpb and last % 4 != 0 and nwords % 4 != 0
    m = _build(PARTIAL)
    assert (int(m.stats().byte_km_back) + 3) // 4 == nwords
    _check(m, ref)
    _check_deferred_and_direct(PARTIAL, monkeypatch, KMX_BS_TILE_LOG2=10)


def test_three_bloom_classes_in_one_slab(monkeypatch):
    """ci = 2, cs = 65535: three Bloom classes, six filters back to back in the slab, whose bins do not end where the filters do."""
    ref = _oracle(THREE_CLASSES)
    assert ref["bf_num"] == 3
    slab_words, starts = _slab(ref)
    _, wpb, _, _ = _geometry(slab_words)
    assert len(starts) == 6 and sum(1 for s in starts[1:] if s % wpb) >= 4   # a bin straddles the boundary
    _check_deferred_and_direct(THREE_CLASSES, monkeypatch)
    _check_deferred_and_direct(THREE_CLASSES, monkeypatch, KMX_BS_TILE_LOG2=10)


def test_two_word_kmers_wide_producers(monkeypatch):
    """k = 55, nh = 9, nb = 6, cs = 4095: two-word k-mers and the producers of the wide template (NHM = 16) feed the same sweep."""
    _check_deferred_and_direct(TWO_WORDS, monkeypatch)


def test_sweep_is_deterministic():
    """the default case twice on one handle (its bins, counters and filters are reused) and once on a fresh one: all equal"""
    ref = _oracle(DEFAULT)
    m = _build(DEFAULT)
    a = _check(m, ref, "first build ")
    b = _check(_build(DEFAULT, m), ref, "second build on the handle ")
    c = _check(_build(DEFAULT), ref, "fresh handle ")
    assert a == b == c


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--tiny-child":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _tiny_child(int(sys.argv[2]))
