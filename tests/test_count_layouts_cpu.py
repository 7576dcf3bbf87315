"""tests/count_layouts.py checks itself without a GPU: for every k the geometry tests use, every layout's expected listing
(count_reads.count) equals the plain-Python dictionary count, and no case is vacuous (at least 150 k-mers listed, a count
of 4 or more where long sequences remain, nothing listed where every sequence is shorter than k)."""
import numpy as np
import pytest

import count_layouts as CL


@pytest.mark.parametrize("k", CL.KS)
def test_layouts_self_check(k):
    assert CL.self_check(k) == 2 * len(CL.LAYOUTS)


def test_the_dirt_sits_on_the_edges():
    for k in CL.KS:
        clean, dirty = CL.text(), CL.dirty_text(k)
        assert len(clean) == CL.N == 3 * 4096 + 100
        assert (dirty[CL.n_positions(k)] == ord("N")).all()
        changed = np.nonzero(clean != dirty)[0]
        lower = changed[dirty[changed] == clean[changed] + 32]
        assert 200 <= len(lower) <= 300                        # 15 stretches of 20, some under an N or an IUPAC letter, some overlapping
        other = np.setdiff1d(changed, lower)
        assert set(CL.n_positions(k)) <= set(other.tolist()) and len(other) <= 11 + 15
        assert np.isin(dirty[np.setdiff1d(other, CL.n_positions(k))], np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)).all()


def test_layout_shapes():
    for k in CL.KS:
        length = np.diff(CL.layout("cut_every_run", k).astype(np.int64))[:-1]
        assert (length % 16 == 0).all() and (length > k).all() and (length < k + 17).all()
        assert (np.diff(CL.layout("all_length_k", k).astype(np.int64))[:-1] == k).all()
        assert (np.diff(CL.layout("all_length_k_plus_1", k).astype(np.int64))[:-1] == k + 1).all()
        one = np.diff(CL.layout("all_length_1", k).astype(np.int64))
        assert (one[:-1] == 1).all() and one[-1] == CL.tail_bases(k)
        assert (np.diff(CL.layout("shorter_than_k", k).astype(np.int64)) < k).all()
        blk = set(CL.layout("cuts_round_block_edge", k).tolist())
        assert {4096 + d for d in range(-k - 1, 3)} <= blk
        wav = set(CL.layout("cuts_round_wave_edge", k).tolist())
        assert {1024 + d for d in range(-k - 1, 3)} | {2 * 4096 - k + 1, 2 * 4096} <= wav
        e = CL.layout("empties_between", k)
        assert (e == 700).sum() == 5001 and (e == 4103).sum() == 301 and len(e) == 5304
        r = np.diff(CL.layout("random_with_empties", k).astype(np.int64))
        assert (r == 0).sum() >= 300
