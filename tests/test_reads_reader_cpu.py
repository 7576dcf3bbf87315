"""The FASTQ / FASTA reader of kmx_build_from_reads (kmcex_amd/csrc/reads_reader.cpp) on the CPU, under AddressSanitizer +
UBSan: tests/reads_reader_driver.cpp is a stand-alone program that prints every batch the reader gives, and a plain Python
parser says what the files hold.  The two are compared as counted windows (a FASTA record cut at a batch end rightly
comes as two sequences that overlap by k - 1 bases), and sequence by sequence where nothing can be cut (FASTQ, or a batch
larger than the file).  No GPU, no HIP; every run must exit 0 with no sanitizer report."""
import functools
import gzip
import os
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import count_reads as CR
import seq_reads as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF = 1 << 20                                                  # the reader's read buffer
WORKERS = max(1, min(8, (os.cpu_count() or 2) // 2))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reads_reader") / "reads_reader_driver")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
                           os.path.join(ROOT, "tests", "reads_reader_driver.cpp"), os.path.join(ROOT, "kmcex_amd", "csrc", "reads_reader.cpp"),
                           "-o", exe, "-ldl"])
    return exe


def run(exe, k, batch, inp):
    """-> (the batches: a list of lists of bytes, the ERR message or None); asserts a clean exit and no sanitizer report"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(k), str(batch), inp], capture_output=True, env=env, timeout=120)
    err = p.stderr.decode("latin-1")
    assert p.returncode == 0, (inp, batch, err)
    assert "ERROR" not in err and "runtime error" not in err and "Sanitizer" not in err, (inp, batch, err)
    lines = p.stdout.split(b"\n")
    assert lines.pop() == b""
    batches, i = [], 0
    while lines[i].startswith(b"BATCH "):
        n = int(lines[i][6:])
        assert n >= 1, "a batch without a sequence"
        batches.append(lines[i + 1:i + 1 + n])
        i += 1 + n
    assert i == len(lines) - 1, (inp, batch, lines[i:i + 3])
    if lines[i] == b"END":
        return batches, None
    assert lines[i].startswith(b"ERR "), lines[i]
    return batches, lines[i][4:].decode("latin-1")


def parse(data: bytes):
    """the sequences a FASTQ / FASTA file holds, in order: plain Python, well-formed input only"""
    body = data.lstrip(b"\n\r \t")
    if not body:
        return []
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines]
    seqs = []
    if body[:1] == b"@":
        i = 0
        while i < len(lines):
            if lines[i] == b"":
                i += 1
                continue
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+" and len(lines[i + 3]) == len(lines[i + 1])
            seqs.append(lines[i + 1])
            i += 4
        return seqs
    assert body[:1] == b">"
    cur = None
    for x in lines:
        if x == b"":
            continue
        if x[:1] == b">":
            if cur is not None:
                seqs.append(b"".join(cur))
            cur = []
        else:
            cur.append(x)
    seqs.append(b"".join(cur))
    return seqs


def flat(batches):
    return [s for b in batches for s in b]


# ---------------------------------------------------------------------------------------------- random small files
K = 5
ALPHABET = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)
QUALITY = np.frombuffer(b"I@+#>", dtype=np.uint8)              # a quality line may begin with '@', '+' or '>'


def random_file(rng, i):
    """(bytes, is FASTQ): both formats, both line ends, blank lines, leading white space, the final newline there or not"""
    fastq, crlf = bool(i % 2), bool((i // 2) % 2)
    nl = b"\r\n" if crlf else b"\n"
    seqs = [ALPHABET[rng.integers(0, len(ALPHABET), size=int(rng.choice([0, 1, K - 1, K, K + 1, 40])))].tobytes() for _ in range(int(rng.integers(0, 7)))]
    blank = lambda: nl * int(rng.choice([0, 0, 1, 2]))             # noqa: E731
    out = [[b"", b"\n", b" \t\n", b"\r\n\n  "][int(rng.integers(0, 4))]] if seqs else [[b"", b"\n \r\n"][int(rng.integers(0, 2))]]
    for j, s in enumerate(seqs):
        if fastq:
            out += [b"@r%d x" % j, nl, s, nl, b"+", [b"", b"r%d" % j][int(rng.integers(0, 2))], nl, QUALITY[rng.integers(0, len(QUALITY), size=len(s))].tobytes(), nl, blank()]
        else:
            w = int(rng.choice([1, 3, 7, 60]))
            out += [b">r%d test" % j, nl, blank()]
            for a in range(0, len(s), w):
                out += [s[a:a + w], nl, blank()]
    data = b"".join(out)
    # without the final newline -- but a FASTQ file whose last record is empty then ends before its quality line: see
    # test_empty_last_record_without_its_newline
    if seqs and rng.integers(0, 2) and not (fastq and not seqs[-1]):
        data = data.rstrip(b"\r\n")
    return data, fastq, seqs


def test_random_small_files(driver, tmp_path):
    rng = np.random.default_rng(20240)
    jobs = []
    for i in range(300):
        data, fastq, seqs = random_file(rng, i)
        assert parse(data) == seqs, i                              # the Python parser reads back what was written
        path = str(tmp_path / f"f{i}")
        with open(path, "wb") as f:
            f.write(data)
        want = CR.dict_count(seqs, K)
        for batch in (1, 2 * K, 13, 1000):
            jobs.append((i, path, fastq, seqs, want, batch))
    assert sum(1 for j in jobs if j[4]) > 600 and sum(1 for j in jobs if not j[3]) > 40

    def check(job):
        i, path, fastq, seqs, want, batch = job
        batches, err = run(driver, K, batch, path)
        assert err is None, (i, batch, err)
        got = flat(batches)
        assert CR.dict_count(got, K) == want, (i, batch)
        if fastq or batch == 1000:                                 # nothing can be cut
            assert got == seqs, (i, batch)
        if not seqs:
            assert batches == []
        return len(batches)

    with ThreadPoolExecutor(WORKERS) as ex:
        n_batches = list(ex.map(check, jobs))
    assert max(n_batches) > 5


# ---------------------------------------------------------------------------------------------- the read buffer's edge
KB = 31


@functools.lru_cache(maxsize=None)
def _genome(n, seed):
    return R.genome_ascii(n, seed=seed).tobytes()


def edge_file(fastq, crlf, d):
    """about 2.1 MiB whose first sequence line ends (its '\\n') at byte 2^20 + d: d = -1 puts the '\\n' last in the first
    buffer, d = 0 first in the second, and with CRLF the '\\r' one byte before"""
    nl = b"\r\n" if crlf else b"\n"
    g, g2 = _genome(1 << 20, 3), _genome(BUF + 77777, 4)
    head = (b"@r0" if fastq else b">r0 edge") + nl
    first = BUF + d - len(head) - (len(nl) - 1)
    seqs = [g[:first]]
    if fastq:
        seqs += [g[200000:250000], g[5000:5100], b"", g[7000:7031]]
        data = b"".join(b"@r" + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for s in seqs)
        data = head + data[len(b"@r" + nl):]
    else:
        seqs += [g2, g[7000:7031]]
        data = head + seqs[0] + nl
        for j, s in enumerate(seqs[1:]):
            data += b">r%d" % (j + 1) + nl + b"".join(s[a:a + 60] + nl for a in range(0, len(s), 60))
    assert data[BUF + d:BUF + d + 1] == b"\n" and data.index(b"\n", len(head)) == BUF + d and 2.0 * BUF < len(data) < 2.2 * BUF
    if crlf:
        assert data[BUF + d - 1:BUF + d] == b"\r"
    return data, seqs


def np_count(seqs, k):
    buf, off = R.flatten(seqs)
    return CR.count(buf, off, k, 1, 2 ** 32 - 1)


def test_read_buffer_edge(driver, tmp_path):
    contents = {}
    for fastq in (True, False):
        for crlf in (False, True):
            for d in (-2, -1, 0, 1, 2):
                data, seqs = edge_file(fastq, crlf, d)
                base = str(tmp_path / f"{'fq' if fastq else 'fa'}_{'crlf' if crlf else 'lf'}_{d + 2}")
                with open(base, "wb") as f:
                    f.write(data)
                with gzip.open(base + ".gz", "wb", compresslevel=1) as f:
                    f.write(data)
                contents[base] = (fastq, seqs)
    small = edge_file(True, False, 0)[1][2:]
    km, cnt = np_count(small, KB)
    d = CR.dict_count(small, KB)
    assert CR.packed_to_int(km) == sorted(d) and cnt.tolist() == [d[x] for x in sorted(d)]     # the numpy count against the dictionary count
    assert parse(edge_file(False, True, -1)[0]) == edge_file(False, True, -1)[1]

    def check(base):
        fastq, seqs = contents[base]
        want = None
        n = 0
        for batch in (62, 10 ** 5, 1 << 26):
            batches, err = run(driver, KB, batch, base)
            assert err is None, (base, batch, err)
            got = flat(batches)
            if fastq or batch == 1 << 26:                          # nothing can be cut
                assert got == seqs, (base, batch)
            else:                                                  # counted windows: numpy's count of both sides (2 M windows each)
                if want is None:
                    want = np_count(seqs, KB)
                km, cnt = np_count(got, KB)
                assert np.array_equal(km, want[0]) and np.array_equal(cnt, want[1]), (base, batch)
                assert len(batches) > 10
            # the gzip twin holds the same bytes: the same batches of the same sequences, so the same windows
            twin, err = run(driver, KB, batch, base + ".gz")
            assert err is None and twin == batches, (base + ".gz", batch, err)
            n += 2
        return n

    with ThreadPoolExecutor(WORKERS) as ex:
        assert sum(ex.map(check, sorted(contents))) == 5 * 2 * 2 * 2 * 3


# ---------------------------------------------------------------------------------------------- "@list"
def test_list_of_files(driver, tmp_path):
    k = 7
    g = R.genome_ascii(3000, seed=9).tobytes()
    fa = [g[0:400], b"", g[500:900]]
    fq = [g[1000:1100], g[1100:1106], b""]
    fa2 = [g[2000:2500]]
    p = {n: str(tmp_path / n) for n in ("a.fa", "b.fq", "empty", "c.fa.gz", "list", "blank", "missing")}
    CR.write_fasta(p["a.fa"], fa, width=60)
    with open(p["a.fa"], "rb") as f:
        data = f.read()
    with open(p["a.fa"], "wb") as f:
        f.write(data.rstrip(b"\n"))                                # no final newline: the FASTQ file after it must not join its last line
    CR.write_fastq(p["b.fq"], fq)
    open(p["empty"], "wb").close()
    CR.write_fasta(p["c.fa.gz"], fa2, width=33, gz=True)
    with open(p["list"], "w") as f:
        f.write(f"\n{p['a.fa']}  \t\n\n{p['b.fq']}\r\n{p['empty']}\n   \n{p['c.fa.gz']}")
    want = fa + fq + fa2
    batches, err = run(driver, k, 1 << 20, "@" + p["list"])
    assert err is None and flat(batches) == want                   # the open FASTA record closed at its file's end
    for batch in (1, 2 * k, 150):
        batches, err = run(driver, k, batch, "@" + p["list"])
        assert err is None and CR.dict_count(flat(batches), k) == CR.dict_count(want, k), batch
        assert len(batches) > 3
    with open(p["blank"], "w") as f:
        f.write("\n  \n\t\r\n")
    batches, err = run(driver, k, 100, "@" + p["blank"])
    assert batches == [] and "names no file" in err and p["blank"] in err
    batches, err = run(driver, k, 100, "@" + p["missing"])
    assert batches == [] and "cannot open the list" in err and p["missing"] in err
    # a file of the list that cannot be opened: the batches before it, then the error
    with open(p["list"], "w") as f:
        f.write(f"{p['b.fq']}\n{p['missing']}\n")
    batches, err = run(driver, k, 100, "@" + p["list"])
    assert err == "cannot open " + p["missing"]


# ---------------------------------------------------------------------------------------------- malformed input
GOOD = b"@r1\nACGTACGT\n+\nIIIIIIII\n"


@pytest.mark.parametrize("name,data,record,what", [pytest.param(*c, id=c[0]) for c in [
    ("no_at", GOOD + b"r2\nACGT\n+\nIIII\n", 2, "does not start with '@'"),
    ("no_plus", GOOD + b"@r2\nACGT\nIIII\n@r3\n", 2, "no '+' line"),
    ("empty_plus", GOOD + b"@r2\nACGT\n\nIIII\n", 2, "no '+' line"),
    ("quality_short", GOOD + GOOD + b"@r3\nACGT\n+\nIII\n", 3, "differ in length"),
    ("quality_long", b"@r1\nACGT\n+\nIIIII\n", 1, "differ in length"),
    ("cut_after_header", GOOD + b"@r2\n", 2, "truncated"),
    ("cut_after_header_no_newline", GOOD + b"@r2", 2, "truncated"),
    ("cut_after_sequence", GOOD + b"@r2\nACGT\n", 2, "truncated"),
    ("cut_after_plus", GOOD + b"@r2\nACGT\n+\n", 2, "truncated"),
    ("cut_after_plus_no_newline", GOOD + b"@r2\nACGT\n+", 2, "truncated"),
    ("cut_crlf", GOOD.replace(b"\n", b"\r\n") + b"@r2\r\nACGT\r\n+\r\n", 2, "truncated"),
    ("fasta_after_white_space", b"\n \n>r1\nACGTAC\nGT\n", None, None),
    ("fasta_second_record_fine", b">r1\nACGTACG\n\n>r2\n\nAC\n", None, None),
]])
def test_malformed_records(driver, tmp_path, name, data, record, what):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    for batch in (1, 1 << 20):
        batches, err = run(driver, 5, batch, path)
        if what is None:
            assert err is None and CR.dict_count(flat(batches), 5) == CR.dict_count(parse(data), 5)
            assert batch == 1 or flat(batches) == parse(data)      # (a batch of 1 base cuts a FASTA record at every line)
            continue
        assert err is not None and path in err and f"record {record}:" in err and what in err, err
        if batch == 1:                                             # the records before the bad one came through
            assert flat(batches) == [b"ACGTACGT"] * (record - 1)


def test_malformed_files(driver, tmp_path):
    path = str(tmp_path / "x")
    # a FASTA sequence line before any header cannot be met in a file that starts with '>', and a file that starts otherwise
    # is refused for its first byte; in a list, a FASTQ file's end closes nothing, so a later FASTA file starts clean
    for data in (b"ACGT\n>r1\nACGT\n", b"\n\n  ACGT\n", b"+\n", b"\x00", b";comment\n>r1\nAC\n"):
        with open(path, "wb") as f:
            f.write(data)
        batches, err = run(driver, 5, 100, path)
        assert batches == [] and err is not None and path in err and "neither FASTQ" in err, (data, err)
    missing = str(tmp_path / "none.fq")
    batches, err = run(driver, 5, 100, missing)
    assert batches == [] and err == "cannot open " + missing
    batches, err = run(driver, 5, 100, str(tmp_path))              # a directory opens, and reads as an error or as nothing
    assert batches == []
    # an empty file, and one of white space only, is no error: no batch
    for data in (b"", b"\n", b" \t\r\n\n"):
        with open(path, "wb") as f:
            f.write(data)
        assert run(driver, 5, 100, path) == ([], None), data


def test_damaged_gzip(driver, tmp_path):
    """a gzip file that ends early, or is damaged after some good blocks, still decodes in part; whatever the part looks
    like -- here its first cut ends exactly on a record -- the reader reports a read error that names the file"""
    reads = [R.genome_ascii(5000, seed=2).tobytes()] * 40
    path = str(tmp_path / "g.fq.gz")
    CR.write_fastq(path, reads, gz=True)
    assert run(driver, 5, 1 << 20, path) == ([reads], None)
    with open(path, "rb") as f:
        z = f.read()
    plain = gzip.decompress(z)
    ends_on_a_record = 0
    for cut in (len(z) // 2, len(z) // 3, len(z) - 1):             # (the last: all the data, the trailer's checksum cut short)
        with open(path, "wb") as f:
            f.write(z[:cut])
        part = zlib.decompressobj(31).decompress(z[:cut])
        ends_on_a_record += part.endswith(b"I" * 5000) and len(part) < len(plain)
        for batch in (1, 1 << 20):
            batches, err = run(driver, 5, batch, path)
            assert err is not None and path in err and "read error" in err, (cut, batch, err)
    assert ends_on_a_record                                        # the case no parser can notice
    with open(path, "wb") as f:
        f.write(z[:len(z) // 2] + bytes(x ^ 0x55 for x in z[len(z) // 2:]))
    batches, err = run(driver, 5, 1 << 20, path)
    assert err is not None and path in err and "read error" in err, err


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_empty_last_record_without_its_newline(driver, tmp_path, nl):
    """a FASTQ file whose last record is empty and whose last newline is missing ends right after the '+' line's newline: the
    reader finds no quality line and reports the record truncated."""
    # This pins what the reader does today.  Whether such a file should rather read as an empty last record is a question of
    # what the reader accepts, which is not changed here: if this test fails, the reader's behaviour moved.
    path = str(tmp_path / "e.fq")
    good = GOOD.replace(b"\n", nl)
    with open(path, "wb") as f:
        f.write(good + b"@r2" + nl + nl + b"+" + nl)
    for batch in (1, 1 << 20):
        batches, err = run(driver, 5, batch, path)
        assert err is not None and path in err and "record 2:" in err and "truncated" in err, err
        if batch == 1:
            assert flat(batches) == [b"ACGTACGT"]
    # with its final newline the same file holds two records, the second one empty
    with open(path, "wb") as f:
        f.write(good + b"@r2" + nl + nl + b"+" + nl + nl)
    for batch in (1, 1 << 20):
        batches, err = run(driver, 5, batch, path)
        assert err is None and flat(batches) == [b"ACGTACGT", b""]
