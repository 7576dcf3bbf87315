"""kmx_unitig_contigs*, kmx_unitig_resolve* and kmx_unitig_map_seqs_dev on the MI355X in the three regimes the other suites do not
reach (the cases are pinned on the CPU by tests/test_unitig_scale_cpu.py): emit tiles that hold up to 820 unitig starts, resolved
and unresolved ones mixed; chains of 65536 to 131072 unitigs (more than 16 doubling rounds, hundreds of blocks, 17000 contigs, a
ladder of resolved unitigs whose neighbours are resolved); and device byte buffers that are not aligned.  Host form and device form
equal the plain-Python restatements byte for byte in every output array, the stats and the counts; where a closed form exists the
returned bytes are also compared with it."""
import functools

import numpy as np
import pytest

import test_gpu_unitig_contigs as TC
import test_gpu_unitig_map as TM
import test_gpu_unitig_resolve as TR
import test_unitig_scale_cpu as S
import unitig_contigs_ref as G
import unitig_resolve_ref as X
from kmcex_amd import KModel
from kmcex_amd.api import UNITIG_DTYPE

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the graph calls
GUARD = 64
LINE_RING = pytest.mark.parametrize("ring", (False, True), ids=("line", "ring"))
lens_id = lambda v: str(v) if isinstance(v, int) else f"lens{len(v)}"


def chain_both_forms(n, k, lens, ring, fork_every=0):
    """host and device form of the contigs of a chain case against the restatement; without forks cseq is the closed form too
    -> the model the calls ran on"""
    kk, strs, rows, hits, text = G.chain_case(n, k, lens, ring, fork_every)
    exp = G.flat(G.want_chain(n, k, lens, ring, fork_every))
    ubuf, uoff, _, loff, lk = TC.flat_input(k, strs, None, rows)
    h = np.array(hits, dtype=np.uint64)
    m = KModel(1, 1023, NH, NB)
    what = f"chain n={n} k={k} ring={ring} fork_every={fork_every}"
    for form, got in (("host", TC.run_host(m, k, ubuf, uoff, None, loff, lk, h, 1, 0)), ("device", TC.run_dev(m, k, TC.dev_input(ubuf, uoff, None, loff, lk), len(ubuf), h, 1, 0))):
        TC.same(got, exp, f"{what}: {form}")
        if not fork_every:
            assert got[0].tobytes().decode() == G.chain_expected(n, k, lens, ring), f"{what}: {form}, cseq is not the sequence"
    return m


@LINE_RING
@pytest.mark.parametrize("n,lens", S.DENSE_CHAINS, ids=lens_id)
def test_contigs_of_dense_tiles(n, lens, ring):
    """k = 5: every lane of k_ctg_emit owns pieces, s_part is full and the search for a word's piece goes to its depth"""
    chain_both_forms(n, 5, lens, ring)


@LINE_RING
@pytest.mark.parametrize("n", S.DEEP_N)
def test_contigs_of_deep_chains(n, ring):
    """2 U is a power of two at the first and the last n; the rounds the library reports prove the depth"""
    m = chain_both_forms(n, 5, (5, 6), ring)
    assert m.unitig_contigs_phases()["rounds"] > 16


@LINE_RING
def test_many_contigs_and_their_graph(ring):
    n, k, lens, fork_every = S.FORKED
    chain_both_forms(n, k, lens, ring, fork_every)
    assert G.want_chain(n, k, lens, ring, fork_every)["stats"]["n_contigs"] == G.fork_counts(n, fork_every, ring)[0] > 17000


@functools.lru_cache(maxsize=None)
def gadgets(k):
    """a gadget case with records and link hits -> (k, strs, recs, rows, hits, through)"""
    n, lens = S.GADGETS[k]
    kk, strs, rows, t = X.gadget_case(n, k, lens, S.SPOIL_EVERY)
    recs, hits = X.records_for(strs, rows, k, 8100 + k)
    return k, strs, recs, rows, hits, t


@pytest.mark.parametrize("k", sorted(S.GADGETS))
def test_resolve_of_dense_tiles_and_every_verdict(k):
    """tiles of k_res_emit with hundreds of starts, copy counts 1 to 4 side by side, centres longer than a tile next to them; at the
    pairs every case runs at and at the pair that gives every spoiled gadget its planned verdict; urec and link_hits present and NULL"""
    kk, strs, recs, rows, hits, t = gadgets(k)
    TR.compare(KModel(1, 1023, NH, NB), f"gadgets k={k}", k, strs, recs, rows, hits, t, X.PARAMS + (X.GADGET_PIN,))


@pytest.mark.parametrize("k", (5, 31))
def test_resolve_where_every_neighbour_is_resolved(k):
    """the ladder: every edge between two centres is renamed at both ends, through both branches of res_target and res_inv"""
    kk, strs, rows, t = X.ladder_case(S.LADDER_N, k)
    recs, hits = X.records_for(strs, rows, k, 8200 + k)
    TR.compare(KModel(1, 1023, NH, NB), f"ladder k={k}", k, strs, recs, rows, hits, t)


def test_contigs_through_resolved_repeats():
    """the library's resolution of the k = 21 gadget case, with its rlink_hits, fed to the contigs: host and device form equal the
    restatement of the contigs on the restatement's resolved graph; every resolved copy joins its way in to its way out"""
    k, strs, recs, rows, hits, t = gadgets(21)
    m = KModel(1, 1023, NH, NB)
    res = TR.run_host(m, k, TR.flat_input(strs, recs, rows), hits, t, (2, 0))
    want = X.resolve(k, strs, recs, rows, hits, t, 2, 0)
    TR.same(res, X.flat(want), "gadgets k=21 (2, 0): host")
    ct = G.contigs(k, want["rstrs"], want["rrecs"], want["rrows"], want["rlink_hits"], 1, 0)
    assert want["stats"]["n_copies_added"] > 1500 and ct["stats"]["n_multi"] >= want["stats"]["n_resolved"] + want["stats"]["n_copies_added"]
    exp = G.flat(ct)
    ubuf, uoff, urec, loff, lk, rhits = res[0], res[1], res[2], res[5], res[6], res[8]
    TC.same(TC.run_host(m, k, ubuf, uoff, urec, loff, lk, rhits, 1, 0), exp, "contigs of the resolved graph: host")
    TC.same(TC.run_dev(m, k, TC.dev_input(ubuf, uoff, urec, loff, lk), len(ubuf), rhits, 1, 0), exp, "contigs of the resolved graph: device")


# ---- misaligned device buffers (the device forms only: the host forms copy into buffers of the library's own)

class Guarded:
    """nbytes of device memory `shift` bytes behind a 64-byte boundary, GUARD bytes of 0xA5 on both sides"""

    def __init__(self, nbytes, shift=0, fill=None):
        import torch
        self.lo, self.n = GUARD + shift, int(nbytes)
        self.big = torch.full((self.lo + self.n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.big.data_ptr() % 64 == 0
        if fill is not None:
            fill = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
            assert fill.size == self.n
            if self.n:
                self.big[self.lo:self.lo + self.n] = torch.from_numpy(fill).cuda()
        self.before = self.big.clone()

    def view(self, dtype=None):
        import torch
        v = self.big[self.lo:self.lo + self.n]
        return v if dtype is None else v.view(dtype)

    def unchanged(self):
        import torch
        return bool(torch.equal(self.big, self.before))

    def bytes(self):
        """the buffer's bytes, after asserting that both guard bands are intact"""
        h = self.big.cpu().numpy()
        assert np.all(h[:self.lo] == 0xA5) and np.all(h[self.lo + self.n:] == 0xA5), "a guard byte was written"
        return h[self.lo:self.lo + self.n]


USEQ_SHIFTS = (1, 3, 4, 8, 15)
OUT_SHIFTS = (0, 1, 8, 15)
MISALIGNED_CHAIN = (613, 21, (21, 22, 37, 5000), False)     # with a fork at every 11th junction: 778416 bytes


@functools.lru_cache(maxsize=None)
def misaligned_chain():
    n, k, lens, ring = MISALIGNED_CHAIN
    kk, strs, rows, hits, text = G.chain_case(n, k, lens, ring, 11)
    res = G.contigs(k, strs, None, rows, hits, 1, 0)
    assert max(map(len, strs)) > 4096 and 0 < sum(o & 1 for o in res["steps"]) < n and res["stats"]["n_multi"] > 40
    assert sum(map(len, strs)) % 16 == 0, "the aligned run must load every byte by wide words: only a shifted run takes the byte-wise path"
    return (k,) + TC.flat_input(k, strs, None, rows) + (np.array(hits, dtype=np.uint64), G.flat(res))


def contigs_shifted(m, s_in, s_out):
    """kmx_unitig_contigs_dev with useq s_in and cseq s_out bytes off a 64-byte boundary, every buffer between guard bands
    -> the outputs cut to the counts, as TC.run_dev returns them"""
    import torch
    k, ubuf, uoff, _, loff, lk, hits, exp = misaligned_chain()
    nu, nb, nl = len(uoff) - 1, len(ubuf), len(lk)
    useq = Guarded(nb, s_in, ubuf)
    ins = [TC.to_dev(uoff, np.int64), TC.to_dev(loff, np.int64), TC.to_dev(lk, np.int32), TC.to_dev(hits, np.int64)]
    before = [x.clone() for x in ins]
    outs = [Guarded(nb, s_out)] + [Guarded(s) for s in ((nu + 1) * 8, nu * 64, nu * 4, nu * 8, (2 * nu + 1) * 8, nl * 4, nl * 8)]
    assert useq.view().data_ptr() % 16 == s_in and outs[0].view().data_ptr() % 16 == s_out
    _, (nc, ncb, ncl), st = m.unitig_contigs_dev(k, useq.view(), ins[0], ins[1], ins[2], ins[3], 1, 0, None, out=tuple(o.view() for o in outs))
    torch.cuda.synchronize()
    assert useq.unchanged() and all(torch.equal(a, b) for a, b in zip(ins, before)), "an input was written"
    h = [o.bytes() for o in outs]
    return (h[0][:ncb], h[1][:(nc + 1) * 8], h[2][:nc * 64], h[3], h[4], h[5][:(2 * nc + 1) * 8], h[6][:ncl * 4], h[7][:ncl * 8], TC.stats_array(st), np.array([nc, ncb, ncl], dtype=np.uint64))


@pytest.mark.parametrize("s_in", USEQ_SHIFTS)
def test_contigs_of_misaligned_buffers(s_in):
    """the byte-wise load of k_ctg_emit (useq not 16-byte aligned) and its byte stores (cseq not 16-byte aligned): the bytes of the
    aligned run and of the restatement, every guard band and every input intact"""
    m = KModel(1, 1023, NH, NB)
    exp = misaligned_chain()[-1]
    aligned = contigs_shifted(m, 0, 0)
    TC.same(aligned, exp, "aligned")
    for s_out in OUT_SHIFTS:
        got = contigs_shifted(m, s_in, s_out)
        TC.same(got, exp, f"useq + {s_in}, cseq + {s_out}")
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, aligned))


@functools.lru_cache(maxsize=None)
def misaligned_resolve(which):
    if which == "geometry":
        k, strs, rows, t = X.geometry_case(4097, 7)
    else:
        k, strs, rows, t = X.gadget_case(72, 21, S.GADGETS[21][1], S.SPOIL_EVERY)
    recs, hits = X.records_for(strs, rows, k, 8300)
    pair = (2, 0)
    want = X.resolve(k, strs, recs, rows, hits, t, *pair)
    assert want["stats"]["n_resolved"] >= 1 and max(map(len, strs)) > 4096
    return (k,) + TR.flat_input(strs, recs, rows) + (np.array(hits, dtype=np.uint64), np.array(t, dtype=np.uint64), pair, X.flat(want))


def resolve_shifted(m, which, s_in, s_out, s_through):
    """kmx_unitig_resolve_dev with useq, rseq and through that many bytes off a 64-byte boundary, every buffer between guard bands"""
    import torch
    k, ubuf, uoff, urec, loff, lk, hits, t, pair, exp = misaligned_resolve(which)
    nu, nl = len(uoff) - 1, len(lk)
    n, b = (int(x) for x in exp[10])
    useq, through = Guarded(len(ubuf), s_in, ubuf), Guarded(16 * nu * 8, s_through, t)
    ins = [TR.to_dev(uoff, np.int64), TR.to_dev(loff, np.int64), TR.to_dev(lk, np.int32), TR.to_dev(urec.view(np.uint8).reshape(-1, 40), np.uint8), TR.to_dev(hits, np.int64)]
    before = [x.clone() for x in ins]
    outs = [Guarded(b, s_out)] + [Guarded(s) for s in ((n + 1) * 8, n * 40, n * 4, nu * 8, (2 * n + 1) * 8, nl * 4, nl * 8, nl * 8)]
    assert useq.view().data_ptr() % 16 == s_in and outs[0].view().data_ptr() % 16 == s_out and through.view().data_ptr() % 16 == s_through
    _, (gn, gb), st = m.unitig_resolve_dev(k, useq.view(), ins[0], ins[1], ins[2], through.view(torch.int64), pair[0], pair[1], ins[3], ins[4], capacity=(n, b),
                                           out=tuple(o.view() for o in outs))
    torch.cuda.synchronize()
    assert (gn, gb) == (n, b) and useq.unchanged() and through.unchanged() and all(torch.equal(x, y) for x, y in zip(ins, before)), "an input was written"
    h = [o.bytes() for o in outs]
    return (h[0], h[1], h[2].view(UNITIG_DTYPE), h[3], h[4], h[5], h[6], h[7], h[8], TR.stats_array(st), np.array([gn, gb], dtype=np.uint64))


@pytest.mark.parametrize("s_in", USEQ_SHIFTS)
def test_resolve_of_misaligned_buffers(s_in):
    """the byte-wise load of k_res_emit and its byte stores, on a unitig of 4097 bytes with four copies and on 72 gadgets"""
    m = KModel(1, 1023, NH, NB)
    for which in ("geometry", "gadgets"):
        exp = misaligned_resolve(which)[-1]
        aligned = resolve_shifted(m, which, 0, 0, 0)
        TR.same(aligned, exp, f"{which}: aligned")
        for s_out in OUT_SHIFTS:
            got = resolve_shifted(m, which, s_in, s_out, 0)
            TR.same(got, exp, f"{which}: useq + {s_in}, rseq + {s_out}")
            assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, aligned))


@pytest.mark.parametrize("which", ("geometry", "gadgets"))
def test_resolve_of_a_through_matrix_that_is_8_aligned(which):
    """d_through 8 bytes off: rows that are not 16-byte aligned, the scalar loads of k_res_verdict"""
    m = KModel(1, 1023, NH, NB)
    exp = misaligned_resolve(which)[-1]
    for s_in, s_out in ((0, 0), (3, 1)):
        TR.same(resolve_shifted(m, which, s_in, s_out, 8), exp, f"{which}: through + 8, useq + {s_in}, rseq + {s_out}")


@pytest.mark.parametrize("name", ("long_read", "k31_tangle"))
def test_map_of_a_misaligned_read_buffer(name):
    """kmx_unitig_map_seqs_dev with the reads 1, 2 and 3 bytes off a 4-byte boundary: the byte path of k_map_windows"""
    import torch
    from kmcex_amd.api import SEQ_MAP_DTYPE, SEQ_SEGMENT_DTYPE
    k, km, cnt, thr, strs, reads, want = TM.ref(name)
    buf, off = TM.R.join(reads)
    n_seqs, cap, nu = len(reads), max(len(buf), 1), len(strs)
    m = KModel(1, 1023, NH, NB)
    TM.begin(m, "host", km, k, strs)
    runs = []
    for shift in (0, 1, 2, 3):
        seq = Guarded(len(buf), shift, buf)
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        segs, so, rec, hits = Guarded(cap * 24), Guarded((n_seqs + 1) * 8), Guarded(n_seqs * 64), Guarded(nu * 8, 0, np.zeros(nu, dtype=np.uint64))
        assert seq.view().data_ptr() % 4 == shift
        ns, _ = m.seq_to_unitigs_dev(seq.view(), d_off, segs.view().reshape(cap, 24), so.view(torch.int64), rec.view().reshape(n_seqs, 64), hits.view(torch.int64))
        torch.cuda.synchronize()
        assert seq.unchanged() and d_off.cpu().numpy().view(np.uint64).tolist() == off.tolist(), "an input was written"
        got = (segs.bytes()[:ns * 24].view(SEQ_SEGMENT_DTYPE), so.bytes().view(np.uint64), rec.bytes().view(SEQ_MAP_DTYPE), hits.bytes().view(np.uint64))
        TM.same(got, want, f"{name}: reads + {shift}")
        runs.append(got)
    m.unitig_map_end()
    assert len(want[0]) > 0 and all(a.tobytes() == b.tobytes() for got in runs[1:] for a, b in zip(got, runs[0]))
