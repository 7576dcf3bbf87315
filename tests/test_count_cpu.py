"""The counting rule restated in numpy (tests/count_reads.py) against a plain-Python count, the golden of
tests/golden/count_golden.json reproduced by the restatement and the CPU oracle, and the facade's init_reads / the
driver's -g compiled with the reference's flags.  No GPU needed."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import count_reads as CR
import oracle_lib as O
import seq_reads as R
from common import sha_file
from kmcex_amd import api, kmcdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = CR.load_golden()


@pytest.mark.parametrize("k", [3, 16, 31, 32, 33, 64])
def test_restatement_equals_dict_count(k):
    rng = np.random.default_rng(k)
    alphabet = list(b"ACGTacgtNRY")
    seqs = [bytes(rng.choice(alphabet, size=int(rng.integers(0, 3 * k)), p=[.195] * 4 + [.04] * 4 + [.02, .02, .02]).tolist()) for _ in range(60)]
    seqs += [b"", b"A" * (k - 1), b"A" * k, b"ACGT" * k, b"acgt" * k]
    if k % 2 == 0:
        half = bytes(rng.choice(list(b"ACGT"), size=k // 2).tolist())
        comp = bytes(b"TGCA"[b"ACGT".index(c)] for c in reversed(half))
        seqs += [half + comp, (half + comp).lower(), half + comp + b"N" + half + comp]   # a palindrome: its own reverse complement
    buf, off = R.flatten(seqs)
    km, cnt = CR.count(buf, off, k, 1, 2 ** 32 - 1)
    d = CR.dict_count(seqs, k)
    assert CR.packed_to_int(km) == sorted(d)
    assert [int(c) for c in cnt] == [d[x] for x in sorted(d)]
    assert int(cnt.sum()) == len(CR.window_starts(buf, off, k))
    if k % 2 == 0:
        p = CR.dict_count([half + comp], k)
        assert list(p.values()) == [1]


def test_lowercase_n_and_sequence_ends():
    k = 5
    assert CR.dict_count([b"ACGTA"], k) == CR.dict_count([b"acgta"], k) == CR.dict_count([b"AcGtA"], k)
    buf, off = R.flatten([b"ACGTAC", b"GTACG", b"ACGNACGTA"])
    km, cnt = CR.count(buf, off, k, 1, 100)
    assert int(cnt.sum()) == 2 + 1 + 1                         # no window across a sequence end or an N
    assert len(CR.window_starts(*R.flatten([b"ACGT", b"A"]), k)) == 0


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_listing_and_oracle_files(name):
    g = GOLDEN[name]
    k, ci, cs, nh, nb = g["k"], g["ci"], g["cs"], g["nh"], g["nb"]
    buf, off = R.flatten(R.make_reads(g["genome_bases"], k, **g["reads"]))
    km, cnt = CR.count(buf, off, k, ci, cs)
    assert len(CR.window_starts(buf, off, k)) == g["n_windows"]
    assert len(km) == g["n_listed"] and CR.listing_sha(km, cnt) == g["listing_sha256"]
    assert (cnt == cs).any() or ci == 1
    with tempfile.TemporaryDirectory() as d:
        o = O.OracleModel(ci, cs, nh, nb)
        o.build(k, km, cnt)
        o.save(d)
        for f, h in g["files"].items():
            assert sha_file(os.path.join(d, f)) == h, f
        kmcdb.write_kmc1(os.path.join(d, "db"), km, cnt, k, ci, cs)    # the KMC1 database the GPU test builds from


def _compile(tmp_path, source, name):
    api.load_library()
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), source,
                           "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
    return exe


def test_init_reads_and_driver_compile_as_cxx11(tmp_path):
    src = tmp_path / "init_reads.cpp"
    src.write_text('#include "kmodel.hpp"\nint main(int argc, char **argv) {\n'
                   '  if (argc < 3) return 2;\n  KModel *km = get_model(1, 1023, 7, 5);\n'
                   '  km->init_reads(std::string(argv[1]), atoi(argv[2]));\n  km->save(argv[3]);\n  delete km;\n  return 0;\n}\n')
    _compile(tmp_path, str(src), "init_reads")
    exe = _compile(tmp_path, os.path.join(ROOT, "examples", "kmcex_main.cpp"), "kmcEx")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "-g" in p.stdout
