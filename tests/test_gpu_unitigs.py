"""kmx_unitigs*, kmx_count_unitigs* on the MI355X: strings, offsets and records equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitigs_ref.py) gives, for the host and the device variant; closure; the edges."""
import ctypes as C
import functools

import numpy as np
import pytest

import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the listing


@functools.lru_cache(maxsize=None)
def ref(name):
    """(k, thr, packed k-mers, counts, k-mer strings, (buf, off, rec) of the restatement), computed once"""
    k, thr, km, cnt, strs, recs = U.case(name)
    return k, thr, U.pack(km, k), np.asarray(cnt, dtype=np.uint32), km, U.flat(strs, recs)


def same(got, want, what=""):
    buf, off, rec = got
    wbuf, woff, wrec = want
    assert np.array_equal(np.asarray(off, dtype=np.uint64), woff), f"{what}: offsets differ"
    assert np.asarray(buf).tobytes() == wbuf.tobytes(), f"{what}: strings differ"
    assert np.asarray(rec).tobytes() == wrec.tobytes(), f"{what}: records differ"


def from_torch(got):
    buf, off, rec = got
    return buf.cpu().numpy(), off.cpu().numpy().view(np.uint64), rec.cpu().numpy().reshape(-1).view(UNITIG_DTYPE)


def run_dev(m, km, cnt, k, thr):
    import torch
    d_km = torch.from_numpy(np.ascontiguousarray(km).view(np.int64).reshape(-1)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    return from_torch(m.unitigs_dev(d_km, d_cnt, k, thr))


@pytest.mark.parametrize("name", [n for n in U.CASES if not n.startswith("reads")])
def test_equals_the_restatement(name):
    """small k with self-loops and hairpins; isolated cycles, alone and beside a path; linear pieces; one path of thousands of
    k-mers (more than 12 doubling rounds); two-word k-mers, circular and linear"""
    k, thr, km, cnt, _, want = ref(name)
    m = KModel(1, 1023, NH, NB)
    same(m.unitigs(km, cnt, k, thr), want, "host")
    if name == "k15_long_path":
        assert m.unitigs_phases()["rounds"] > 12
    same(run_dev(m, km, cnt, k, thr), want, "device")
    same(m.unitigs(km, cnt, k, thr), want, "second call on the same handle")


@pytest.mark.parametrize("thr", [1, 3])
def test_thr_on_a_counted_session(thr):
    """reads at 20x with 1 % errors over a 5000-base genome, counted through kmx_count_*: count_unitigs == unitigs on the
    downloaded listing == the device variants == the restatement; the model the session built answers as before"""
    k, _, km, cnt, km_s, want = ref(f"reads_thr{thr}")
    reads = U.CASES[f"reads_thr{thr}"]()[2]
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(reads)
    assert m.count_finish() == len(cnt)
    lk, lc = m.count_listing()
    assert np.array_equal(lk, km) and np.array_equal(lc, cnt), "the listing is not the restatement's"
    probe = km_s[:: max(len(km_s) // 200, 1)]
    before = m.kmer_to_occ(probe)
    got = m.count_unitigs(thr)
    same(got, want, "count_unitigs")
    assert (len(got[1]) - 1 > 1000) if thr == 1 else (len(got[1]) - 1 < 10)
    same(from_torch(m.count_unitigs_dev(thr)), want, "count_unitigs_dev")
    same(m.unitigs(lk, lc, k, thr), want, "unitigs on the downloaded listing")
    same(run_dev(m, lk, lc, k, thr), want, "unitigs_dev on the downloaded listing")
    assert m.kmer_to_occ(probe) == before
    lk2, lc2 = m.count_listing()
    assert np.array_equal(lk2, lk) and np.array_equal(lc2, lc), "the listing changed"


def test_closure_at_2e5_nodes():
    """counting the k-mers of the emitted unitigs (ci = 1) lists exactly the node set"""
    k, thr = 31, 2
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = acgt[rng.integers(0, 4, 200000)]
    g2 = g.copy()
    hit = rng.random(g2.size) < 0.002                            # a second copy with substitutions: its own k-mers count 1
    g2[hit] = acgt[(np.searchsorted(acgt, g2[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    buf = np.concatenate([g, g, g2])
    off = np.array([0, g.size, 2 * g.size, 3 * g.size], dtype=np.uint64)
    m = KModel(1, 1023, NH, NB)
    m.count_begin(k)
    m.count_seqs(buf, off)
    m.count_finish()
    km, cnt = m.count_listing()
    nodes = km[cnt >= thr]
    assert 180000 < len(nodes) < len(km)
    ubuf, uoff, rec = m.count_unitigs(thr)
    assert int(rec["n_kmers"].sum()) == len(nodes) and int(rec["sum_count"].sum()) == int(cnt[cnt >= thr].sum())
    assert np.array_equal(np.diff(uoff.astype(np.int64)), rec["n_kmers"].astype(np.int64) + k - 1)
    assert np.all(np.diff(rec["first_node"].astype(np.int64)) > 0)
    m2 = KModel(1, 1023, NH, NB)
    m2.count_begin(k)
    m2.count_seqs(ubuf, uoff)
    m2.count_finish()
    km2, cnt2 = m2.count_listing()
    assert np.array_equal(km2, nodes), "the unitigs' k-mers are not the node set"
    assert np.all(cnt2 == 1), "a node lies in two unitigs, or twice in one"


def raw(m, fn, args, seq_cap, rec_cap, with_rec=True, canary=0xA5, give_seq=True):
    """one call on device buffers that are longer than the capacities it is told: -> (rc, n_unitigs, n_bases, seq, offs, rec)"""
    import torch
    seq = torch.full((seq_cap + 64,), canary, dtype=torch.uint8, device="cuda")
    offs = torch.full((rec_cap + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    rec = torch.full(((rec_cap + 2) * 40,), canary, dtype=torch.uint8, device="cuda")
    nu, nb = C.c_uint64(0), C.c_uint64(0)
    rc = fn(m.h, *args, seq.data_ptr() if give_seq else None, seq_cap, offs.data_ptr(), rec.data_ptr() if with_rec else None, rec_cap, C.byref(nu), C.byref(nb))
    torch.cuda.synchronize()
    return rc, nu.value, nb.value, seq.cpu().numpy(), offs.cpu().numpy(), rec.cpu().numpy()


def test_capacities_sizing_and_canaries():
    import torch
    k, thr, km, cnt, _, (wbuf, woff, wrec) = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    d_km = torch.from_numpy(km.view(np.int64)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    args = (k, d_km.data_ptr(), d_cnt.data_ptr(), len(cnt), thr)
    nu, nb = len(wrec), len(wbuf)
    fn = m.L.kmx_unitigs_dev
    # the sizing call: counts only
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu, give_seq=False)
    assert (rc, gu, gb) == (0, nu, nb) and np.all(seq == 0xA5) and np.all(offs == -6) and np.all(rec == 0xA5)
    # exact capacities: everything inside, nothing behind
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu)
    assert (rc, gu, gb) == (0, nu, nb)
    assert seq[:nb].tobytes() == wbuf.tobytes() and np.all(seq[nb:] == 0xA5)
    assert np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(offs[nu + 1:] == -6)
    assert rec[:nu * 40].tobytes() == wrec.tobytes() and np.all(rec[nu * 40:] == 0xA5)
    # rec == NULL
    rc, gu, gb, seq, offs, rec = raw(m, fn, args, nb, nu, with_rec=False)
    assert rc == 0 and seq[:nb].tobytes() == wbuf.tobytes() and np.array_equal(offs[:nu + 1].view(np.uint64), woff) and np.all(rec == 0xA5)
    # one short in each dimension: KMX_E_RANGE, exact needs, nothing at or behind a capacity
    for sc, rcap in ((nb - 1, nu), (nb, nu - 1)):
        rc, gu, gb, seq, offs, rec = raw(m, fn, args, sc, rcap)
        assert (rc, gu, gb) == (-5, nu, nb)
        assert np.all(seq[sc:] == 0xA5) and np.all(offs[rcap + 1:] == -6) and np.all(rec[rcap * 40:] == 0xA5)
    # the host variant reports the same
    obuf = np.full(nb + 8, 0xA5, dtype=np.uint8)
    ooff = np.zeros(nu + 1, dtype=np.uint64)
    cu, cb = C.c_uint64(0), C.c_uint64(0)
    rc = m.L.kmx_unitigs(m.h, k, km.ctypes.data, cnt.ctypes.data, len(cnt), thr, obuf.ctypes.data, nb - 1, ooff.ctypes.data, None, nu, C.byref(cu), C.byref(cb))
    assert (rc, cu.value, cb.value) == (-5, nu, nb) and np.all(obuf[nb - 1:] == 0xA5)


def test_empty_and_thr_above_every_count():
    import torch
    k, _, km, cnt, _, _ = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    for kk, cc, thr in ((km[:0], cnt[:0], 1), (km, cnt, int(cnt.max()) + 1)):
        buf, off, rec = m.unitigs(kk, cc, k, thr)
        assert len(buf) == 0 and len(rec) == 0 and off.tolist() == [0]
        d_km = torch.from_numpy(np.ascontiguousarray(kk).view(np.int64)).cuda()
        d_cnt = torch.from_numpy(np.ascontiguousarray(cc).view(np.int32)).cuda()
        rc, gu, gb, seq, offs, _ = raw(m, m.L.kmx_unitigs_dev, (k, d_km.data_ptr() or None, d_cnt.data_ptr() or None, len(cc), thr), 4, 4)
        assert (rc, gu, gb) == (0, 0, 0) and offs[0] == 0 and np.all(offs[1:] == -6) and np.all(seq == 0xA5)


def test_bad_listings_and_arguments():
    k, _, km, cnt, km_s, want = ref("k7_linear300")
    m = KModel(1, 1023, NH, NB)
    swapped = km.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    dup = km.copy()
    dup[20] = dup[19]
    noncanon = km.copy()
    i = next(j for j, s in enumerate(km_s) if (j == 0 or U.rc(s) > km_s[j - 1]) and (j + 1 == len(km_s) or U.rc(s) < km_s[j + 1]))
    noncanon[i] = U.pack([U.rc(km_s[i])], k)[0]                    # still ascending, no longer canonical
    assert np.all(np.diff(noncanon.astype(np.int64)) > 0)
    wide = km.copy()
    wide[-1] |= np.uint64(1) << np.uint64(2 * k + 3)
    for bad in (swapped, dup, noncanon, wide):
        with pytest.raises(KmxError) as e:
            m.unitigs(bad, cnt, k, 1)
        assert e.value.code == -1
    for kk in (4, 6, 30, 32, 64, 3, 65):                            # even, or out of range
        with pytest.raises(KmxError) as e:
            m.unitigs(np.zeros(2 * ((kk + 31) // 32), np.uint64), np.ones(2, np.uint32), kk, 1)
        assert e.value.code == -1
    nu, nb = C.c_uint64(0), C.c_uint64(0)
    assert m.L.kmx_unitigs_dev(m.h, 31, None, None, 1 << 31, 1, None, 0, None, None, 0, C.byref(nu), C.byref(nb)) == -1
    same(m.unitigs(km, cnt, k, 1), want, "after the refusals")       # the handle is still usable


def test_no_listing_and_even_session_k():
    m = KModel(1, 1023, NH, NB)
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -4
    m.count_begin(31)
    with pytest.raises(KmxError) as e:                              # a session under way has no listing yet
        m.count_unitigs(1)
    assert e.value.code == -4
    m.count_seqs([U.rand_seq(300, 5)])
    m.count_finish()
    assert len(m.count_unitigs(1)[2]) >= 1
    m.count_begin(30)
    m.count_seqs([U.rand_seq(300, 5)])
    m.count_finish()
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -1
    km, cnt = m.count_listing()
    m.build_packed(30, km, cnt)                                     # a build from other data drops the listing
    with pytest.raises(KmxError) as e:
        m.count_unitigs(1)
    assert e.value.code == -4


def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first call, for kmx_unitigs and for kmx_count_unitigs: the same call then succeeds,
    and the session's listing and model are as they were"""
    k, thr, km, cnt, _, want = ref("k9_linear2000")
    seq = U.CASES["k9_linear2000"]()[2]
    failed = {"unitigs": 0, "count_unitigs": 0}
    for which in failed:
        for nth in range(1, 16):
            m = KModel(1, 1023, NH, NB)                             # fresh: every buffer of the call is still to be allocated
            if which == "count_unitigs":
                m.count_begin(k)
                m.count_seqs(seq)
                m.count_finish()
                lk, lc = m.count_listing()
                assert np.array_equal(lk, km) and np.array_equal(lc, cnt)
                probe = U.unpack(km[::40], k)
                before = m.kmer_to_occ(probe)
                call = lambda: m.count_unitigs(thr)                 # noqa: E731
            else:
                call = lambda: m.unitigs(km, cnt, k, thr)           # noqa: E731
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                same(call(), want, f"{which}: allocation {nth} did not happen")
            except KmxError as e:
                assert e.code == -6
                failed[which] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(call(), want, f"{which} after a failed allocation ({nth})")
            if which == "count_unitigs":
                lk2, lc2 = m.count_listing()
                assert np.array_equal(lk2, km) and np.array_equal(lc2, cnt), "the listing changed"
                assert m.kmer_to_occ(probe) == before, "the model changed"
    assert failed["unitigs"] >= 8 and failed["count_unitigs"] >= 6, failed   # (11 and 9 buffers are allocated by a first call)


def parse_fasta(text):
    heads, strs = [], []
    for line in text.splitlines():
        (heads if line.startswith(">") else strs).append(line)
    return heads, strs


def fasta_heads(rec):
    return [f">u{u} n_kmers={int(r['n_kmers'])} mean_count={int(r['sum_count']) / int(r['n_kmers']):.2f} circular={int(r['circular'])}" for u, r in enumerate(rec)]


def test_facade_and_driver_fasta(tmp_path):
    """tests/facade_unitigs.cpp (count_unitigs == unitigs on the listing, inside the program) and the driver's -u switch: the
    FASTA they write, parsed back, is the Python result"""
    import os
    import subprocess
    import count_reads as CR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, thr = 21, 3
    reads = [r.encode() for r in U.CASES["reads_thr3"]()[2]]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, reads)
    m = KModel(1, 1023, NH, NB)
    m.init_reads(fa, k)
    km, cnt = m.count_listing()
    buf, off, rec = m.count_unitigs(thr)
    want = [buf[int(off[u]):int(off[u + 1])].tobytes().decode() for u in range(len(rec))]
    same((buf, off, rec), ref("reads_thr3")[5], "init_reads + count_unitigs")
    listing = str(tmp_path / "listing.txt")
    with open(listing, "w") as f:
        f.write("".join(f"{int(x)} {int(c)}\n" for x, c in zip(km, cnt)))

    def build(source, name):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(root, "include"), os.path.join(root, source),
                               "-L" + os.path.join(root, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(root, "kmcex_amd"), "-o", exe])
        return exe

    out = subprocess.check_output([build("tests/facade_unitigs.cpp", "facade_unitigs"), fa, str(k), str(thr), listing], timeout=120).decode()
    assert parse_fasta(out) == (fasta_heads(rec), want)
    work = tmp_path / "work"
    work.mkdir()
    subprocess.check_call([build("examples/kmcex_main.cpp", "kmcEx"), "-g", f"-u{thr}", f"-k{k}", "-nh3", "-nb2", fa, "db", str(work)], timeout=120)
    assert parse_fasta((work / "db" / "unitigs.fa").read_text()) == (fasta_heads(rec), want)
