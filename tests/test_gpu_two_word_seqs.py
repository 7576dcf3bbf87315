"""The sequence calls at two-word k on models that ANSWER: kmx_query_seqs, seq_summary, kmx_correct_seqs, seq_edit,
kmx_polish_seqs and kmx_extend_seqs at k = 33, 34, 35, 55, 63, 64 (the walks at k = 32 too) on models built from as-asked
listings (tests/as_asked.py; tests/test_two_word_models_cpu.py proves on the CPU oracle alone that substitutions verify, indels
are applied and walks run on and look ahead there).  Every output must EQUAL, byte for byte, the reference rule driven by the CPU
oracle: there is no tolerance.  The word-edge widths are here: ext_node's full masks at k = 32 and 64, its backward branch
pos < 64 (k = 33, 34, 35 with 2 - 4 lookahead digits split across the two words), c0 shifts of 0, 2, 4 and 62."""
import functools
import os

import numpy as np
import pytest

import as_asked as A
import seq_correct_ref as S
import seq_edit_ref as E
import seq_extend_ref as X
import seq_reads as R
import seq_summary_ref as SS
import test_gpu_seq_correct as TC
import test_gpu_seq_edit as TE
import test_gpu_seq_extend as TX
import test_gpu_seq_polish as TP
import test_gpu_seq_summary as TS
from common import sha_file
from kmcex_amd import KModel
from test_gpu_parity import _check_arrays

pytestmark = pytest.mark.gpu

KS = [33, 34, 35, 55, 63, 64]
THR = (1, 2, 8)
CHUNK = "4099"                                                    # the smaller KMX_SEQ_CHUNK_BASES of test_small_chunks_*


@functools.lru_cache(maxsize=None)
def _model(kind: str, k: int) -> KModel:
    """the GPU's model of the reads' (kind "genome") or the seeds' ("extend") listing: built once, shared, left unchanged"""
    c = A.genome_case(k) if kind == "genome" else A.extend_case(k)
    ci, cs, nh, nb = A.PARAMS[k]
    m = KModel(ci, cs, nh, nb)
    m.build_packed(k, c["km"], c["cnt"])
    return m


@pytest.mark.parametrize("kind,k", [("genome", k) for k in KS] + [("extend", k) for k in [32] + KS])
def test_the_build_is_the_oracles(kind, k, tmp_path):
    """many entries with hi == 0 and, at k = 63, two entries that carry thousands of windows each"""
    c = A.genome_case(k) if kind == "genome" else A.extend_case(k)
    m, o = _model(kind, k), c["o"]
    st, so = m.stats(), o.stats()
    assert (st.n_km, list(st.n_bf), st.km_byte_size, st.byte_km_back) == (so.n_km, list(so.n_bf), so.km_byte_size, so.byte_km_back)
    _check_arrays(m, o, A.PARAMS[k][3], st.bf_num)
    assert (st.attempts, st.successes, st.rest_entries) == (so.attempts, so.successes, so.rest_entries)
    d1, d2 = str(tmp_path / "g"), str(tmp_path / "o")
    os.makedirs(d1)
    m.save(d1)
    o.save(d2)
    for f in ("header", "km.bin", "rest.bin"):
        assert sha_file(os.path.join(d1, f)) == sha_file(os.path.join(d2, f)), f
    assert np.array_equal(m.kmer_to_occ_packed(c["km"].reshape(-1)), o.query_packed(k, c["km"]))


@pytest.mark.parametrize("k", KS)
def test_query_and_summary(k):
    import torch
    c, m = A.genome_case(k), _model("genome", k)
    text = R.flatten(c["text"])
    for buf, off, want, found in ((c["buf"], c["off"], A.per_base(k), 0.2), text + (R.oracle_per_base(c["o"], *text, k), 0.49)):
        valid = R.valid_mask(off, k)
        assert (want[valid] >= 1).mean() > found and (found > 0.2 or (want[valid] == 0).sum() >= 1000)     # the oracle finds, and misses in the reads
        got = m.seq_to_occ_flat(buf, off)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        d_seq = torch.from_numpy(buf).to("cuda")
        d_off = torch.from_numpy(off.view(np.int64)).to("cuda")
        d_out = torch.full((len(buf),), 7, dtype=torch.int32, device="cuda")
        m.seq_to_occ_dev(d_seq.data_ptr(), d_off.data_ptr(), len(off) - 1, len(buf), d_out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want)
        rec = SS.summarise(want, off, k, THR)
        assert SS.same(m.seq_summary_flat(buf, off, THR), rec)
        assert SS.same(TS._dev(m, buf, off, THR), rec)


@pytest.mark.parametrize("k", [32] + KS)
def test_extend(k, monkeypatch):
    c, m = A.extend_case(k), _model("extend", k)
    buf, off = c["buf"], c["off"]
    monkeypatch.delenv("KMX_EXTEND_STEPS", raising=False)
    for thr in (1, 3):
        for depth in (0, 1, 2, 3):
            want = A.want_extend(k, thr, depth)
            got = m.seq_extend_flat(buf, off, thr, A.MAX_EXT, depth)
            assert TX._same(got, want), ("host", thr, depth, TX._explain(got, want))
            got = TX._dev(m, buf, off, thr, A.MAX_EXT, depth)
            assert TX._same(got, want), ("device", thr, depth, TX._explain(got, want))
    want = A.want_extend(k, 1, 2)
    assert TX._same(TX._gpu_rule(m, buf, off, k, 1, A.MAX_EXT, 2), want)      # the rule over the GPU's own kmer_to_occ_rows
    monkeypatch.setenv("KMX_EXTEND_STEPS", "7")                              # every long walk is launched again and again
    thr = 3 if k == 32 else 1
    want = A.want_extend(k, thr, 3)
    assert int(want[1]["n_ext"].max()) > 7
    assert TX._same(m.seq_extend_flat(buf, off, thr, A.MAX_EXT, 3), want) and TX._same(TX._dev(m, buf, off, thr, A.MAX_EXT, 3), want)
    monkeypatch.delenv("KMX_EXTEND_STEPS")
    seeds = c["seeds"][A.N_SEEDS:A.N_SEEDS + 50]                             # reversed seeds: to the left they walk along the text
    l_ext, l_rec, _ = X.extend_left(*R.flatten(seeds), k, 1, A.MAX_EXT, 2, S.oracle_rows(c["o"], k))
    got, rec = m.seq_extend(seeds, 1, A.MAX_EXT, 2, left=True)
    assert X.same(rec, l_rec) and got == [X.revcomp(l_ext[i, :int(l_rec["n_ext"][i])].tobytes()) for i in range(len(seeds))]
    assert int(l_rec["n_ext"].sum()) >= 100


def _correct_all_ways(m, buf, off, thr, ms, want):
    got = m.seq_correct_flat(buf, off, thr, ms)
    assert got[0].dtype == np.uint8 and got[1].dtype == TC.REC and TC._same(got, want), ("host", thr, ms)
    assert TC._same(TC._dev(m, buf, off, thr, ms), want), ("device", thr, ms)
    assert np.array_equal(TC._dev(m, buf, off, thr, ms, records=False)[0], want[0]), ("d_rec == NULL", thr, ms)
    inplace = buf.copy()                                                     # seq_out == seq on the host
    rec = np.zeros(len(off) - 1, TC.REC)
    assert m.L.kmx_correct_seqs(m.h, inplace.ctypes.data, off.ctypes.data, len(off) - 1, thr, ms, inplace.ctypes.data, rec.ctypes.data) == 0
    assert np.array_equal(inplace, want[0]) and S.same(rec, want[1]), ("in place", thr, ms)


@pytest.mark.parametrize("k", KS)
def test_correct(k):
    c, m = A.genome_case(k), _model("genome", k)
    for thr, ms in ((1, 1), (2, 4)):
        _correct_all_ways(m, c["buf"], c["off"], thr, ms, A.want_correct(k, thr, ms))
    assert TC._same(TC._gpu_rule(m, c["buf"], c["off"], k, 1, 1), A.want_correct(k, 1, 1))


def _edit_both(m, buf, off, thr, ms, ops, want):
    got = m.seq_edit_flat(buf, off, thr, ms, ops)
    assert got[1].dtype == TE.REC and TE._same(got, want), ("host", thr, ms, ops)
    dev = TE._dev(m, buf, off, thr, ms, ops)
    assert TE._same(dev, want) and TE._applied(dev, buf, off, want[0]), ("device", thr, ms, ops)
    w_out, w_off = E.apply_edits(buf, off, want[0])
    assert np.array_equal(np.diff(w_off), want[1]["out_len"])


@pytest.mark.parametrize("k", KS)
def test_edit(k):
    c, m = A.genome_case(k), _model("genome", k)
    for ms in (1, 2):
        for ops in (7, 1, 2, 4):
            _edit_both(m, c["ebuf"], c["eoff"], 1, ms, ops, A.want_edit(k, 1, ms, ops))
    assert np.array_equal(TE._dev(m, c["ebuf"], c["eoff"], 1, 1, 7, records=False, apply=False)[0], A.want_edit(k, 1, 1, 7)[0])   # d_rec == NULL


@pytest.mark.parametrize("k", [33, 64])
def test_polish(k):
    c, m = A.genome_case(k), _model("genome", k)
    for mp in (8, 1):
        want = A.want_polish(k, 1, 1, mp)
        TP._both(m, c["ebuf"], c["eoff"], 1, 1, 7, mp, want)              # bases, final offsets, per-read records, passes_run
    assert A.want_polish(k, 1, 1, 8)["passes_run"] == 3


@pytest.mark.parametrize("k", [33, 64])
def test_chunk_edges(k, monkeypatch):
    """KMX_SEQ_CHUNK_BASES (test hook): the 3 000-base read and 100 reads in pieces of 4 099 bases -- runs, sites and the two-word
    verification windows cross the pieces"""
    c, m = A.genome_case(k), _model("genome", k)
    buf, off = A.chunk_subset(c["reads"])
    ebuf, eoff = A.chunk_subset(c["ereads"])
    assert int(np.diff(off).max()) == A.LONG_READ and len(off) == len(eoff) == 102 and len(buf) > 3 * int(CHUNK)
    w_c = S.oracle_correct(c["o"], buf, off, k, 1, 1)[:2]
    w_e = E.oracle_edit(c["o"], ebuf, eoff, k, 1, 1, 7)[:2]
    assert int(w_c[1]["n_corrected"].sum()) >= 20 and len(w_e[0]) >= 20 and int(w_e[1]["n_del"].sum()) >= 3 and int(w_e[1]["n_ins"].sum()) >= 3
    monkeypatch.setenv("KMX_SEQ_CHUNK_BASES", CHUNK)
    _correct_all_ways(m, buf, off, 1, 1, w_c)
    _edit_both(m, ebuf, eoff, 1, 1, 7, w_e)
    monkeypatch.delenv("KMX_SEQ_CHUNK_BASES")
    _correct_all_ways(m, buf, off, 1, 1, w_c)
    _edit_both(m, ebuf, eoff, 1, 1, 7, w_e)
