"""The two helpers every sequence call of kmcex_amd.api goes through, without a device: _flat_seqs normalises (bases, offsets) and
refuses offsets that are none; _join_seqs turns a str / bytes sequence or a list of them into bases and offsets."""
import numpy as np
import pytest

from kmcex_amd import api
from kmcex_amd.api import KmxError


def test_flat_seqs_refuses_empty_offsets():
    with pytest.raises(KmxError) as e:
        api._flat_seqs(np.frombuffer(b"ACGT", dtype=np.uint8), np.zeros(0, dtype=np.uint64))
    assert e.value.code == -1 and "offsets must hold n_seqs + 1 entries" in str(e.value)


def test_flat_seqs_refuses_offsets_past_the_bases():
    with pytest.raises(KmxError) as e:
        api._flat_seqs(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 2, 5])
    assert e.value.code == -1 and "offsets end at 5, past the 4 bases given" in str(e.value)
    buf, off = api._flat_seqs(np.frombuffer(b"ACGT", dtype=np.uint8), [0, 2, 4])      # (ending at the last base is inside)
    assert buf.tobytes() == b"ACGT" and off.tolist() == [0, 2, 4]


@pytest.mark.parametrize("kind", ["2-D", "non-contiguous", "int64"])
def test_flat_seqs_normalises(kind):
    bases = np.frombuffer(b"ACGTTGCAACGT", dtype=np.uint8)
    offsets = np.array([0, 5, 5, 12], dtype=np.uint64)
    if kind == "2-D":
        b, o = bases.reshape(3, 4), offsets.reshape(2, 2)
    elif kind == "non-contiguous":
        b, o = np.repeat(bases, 2)[::2], np.repeat(offsets, 3)[::3]
        assert not b.flags["C_CONTIGUOUS"] and not o.flags["C_CONTIGUOUS"]
    else:
        b, o = bases.astype(np.int64), offsets.astype(np.int64)
    buf, off = api._flat_seqs(b, o)
    for a, dt, want in ((buf, np.uint8, bases), (off, np.uint64, offsets)):
        assert a.ndim == 1 and a.flags["C_CONTIGUOUS"] and a.dtype == dt
        assert np.array_equal(a, want)


@pytest.mark.parametrize("seqs, single, raw, offsets", [
    ("ACGT", True, [b"ACGT"], [0, 4]),
    (b"ACGTN", True, [b"ACGTN"], [0, 5]),
    (["ACG", b"TT", "", b"GATTACA"], False, [b"ACG", b"TT", b"", b"GATTACA"], [0, 3, 5, 5, 12]),
    ([], False, [], [0]),
])
def test_join_seqs(seqs, single, raw, offsets):
    got_single, got_raw, buf, off = api._join_seqs(seqs)
    assert got_single is single
    assert got_raw == raw
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.tobytes() == b"".join(raw)
    assert off.dtype == np.uint64 and off.tolist() == offsets
    assert api._split_seqs(buf, off) == raw
    assert api._flat_seqs(buf, off)[1].tolist() == offsets               # what it makes is what the calls accept
