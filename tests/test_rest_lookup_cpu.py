"""The crafted rest tables (tests/rest_tables.py) against the CPU oracle: do they exercise what they claim?

tests/test_gpu_rest_lookup.py compares the device lookup with the oracle on these tables.  That comparison is only worth
something if the oracle's answers on them come from the rest table, if the inclusive upper bound of its search really
answers some of the queries, and so on -- conditions (a)-(f) below are asserted here, without a GPU, so that the GPU test
cannot pass while testing nothing.  `lookup` (a plain-Python restatement of check_kmer) is held against the oracle on the
way, and the oracle against the compiled reference where that exists.
"""
import numpy as np
import pytest

import oracle_lib as O
import rest_tables as T

SHAPES = T.SHAPES


@pytest.fixture(scope="session")
def rest_base(tmp_path_factory):
    return tmp_path_factory.mktemp("rest_tables")


_answers = {}


def answers(base, k, pre_len):
    """per shape, once: the table, the query strings, what the oracle says with the crafted table and with an empty one"""
    if (k, pre_len) not in _answers:
        t = T.info(k, pre_len)
        d1, d0 = T.model_dirs(base, k, pre_len)
        o, o0 = O.OracleModel.load(d1), O.OracleModel.load(d0)
        strs = [T.to_str(v, k) for v in t["queries"]]
        _answers[(k, pre_len)] = (t, T.read_rest_bin(d1 + "/rest.bin"), o, o0, strs, o.query_strings(strs), o0.query_strings(strs))
    return _answers[(k, pre_len)]


def test_file_round_trip(tmp_path):
    rows, counts, _ = T.crafted(31, 7)
    T.write_rest_bin(tmp_path / "rest.bin", 31, 7, rows, counts)
    t = T.read_rest_bin(tmp_path / "rest.bin")
    assert t["rows"] == rows and t["counts"].tolist() == counts and t["entries"] == len(rows)
    assert (t["k"], t["pre_len"], t["map_size"], t["suff_group"]) == (31, 7, 4 ** 7, 6)
    assert len(t["pre_buffer"]) == len(T.info(31, 7)["prefixes"]) + 1 and t["pre_buffer"][-1] == len(rows)
    T.write_rest_bin(tmp_path / "empty.bin", 31, 7, [], [])
    e = T.read_rest_bin(tmp_path / "empty.bin")
    assert e["entries"] == 0 and e["pre_buffer"].tolist() == [0] and (e["hash2index"] == -1).all()
    assert T.lookup(e, rows[0]) == 0


def test_the_oracle_writes_the_same_file(tmp_path):
    """write_rest_bin of the rows read back from a file the oracle saved gives that file, byte for byte (one and two words)"""
    from kmcex_amd import synth
    for k in (31, 55):
        km, cnt = synth.make_stream(60000, k, 1, 1023)
        o = O.OracleModel(1, 1023, 7, 5)
        o.build(k, km, cnt)
        d = tmp_path / f"k{k}"
        o.save(str(d))
        t = T.read_rest_bin(d / "rest.bin")
        assert t["entries"] == o.stats().rest_entries > 100
        T.write_rest_bin(d / "again.bin", k, t["pre_len"], t["rows"], t["counts"].tolist())
        assert (d / "again.bin").read_bytes() == (d / "rest.bin").read_bytes()


@pytest.mark.parametrize("k,pre_len", SHAPES)
def test_layout(k, pre_len):
    """what `crafted` promises about the table itself"""
    t = T.info(k, pre_len)
    rows, counts, sbits, M = t["rows"], t["counts"], 2 * (k - pre_len), 4 ** pre_len
    assert rows == sorted(rows) and all(0 <= v < 4 ** k for v in rows) and all(1 <= c <= 1023 for c in counts)
    pre = [v >> sbits for v in rows]
    assert pre[0] == 0 and pre[-1] == M - 1
    assert len(set(pre)) >= (6 if pre_len > 1 else 4)
    if pre_len > 1:
        assert any(b - a > 1 for a, b in zip(t["prefixes"], t["prefixes"][1:])), "no empty prefix between groups"
    d = t["dup"]
    assert rows[d] == rows[d - 1] and counts[d] == counts[d - 1]
    assert sum(a == b for a, b in zip(rows, rows[1:])) == 1
    # (d) the long run: >= 40 rows sharing all but their last 12 bits -- in one group beside other rows wherever a group can
    # hold rows that differ elsewhere (sbits > 12)
    run = t["run"]
    assert len(run) >= 40 and len({v >> 12 for v in run}) == 1 and set(run) <= set(rows)
    if sbits > 12:
        assert len({v >> sbits for v in run}) == 1
        assert any(v >> sbits == run[0] >> sbits and v >> 12 != run[0] >> 12 for v in rows)
    if sbits:
        assert t["single"] is not None
        # the alternation: at least two groups whose successor starts above all their rows, at least one whose does not
        assert sum(g for _, _, g in t["next_first"]) >= 2 and sum(not g for _, _, g in t["next_first"]) >= 1


@pytest.mark.parametrize("k,pre_len", SHAPES)
def test_oracle_answers_come_from_the_table(rest_base, k, pre_len):
    t, table, o, o0, strs, ans, ans0 = answers(rest_base, k, pre_len)
    assert np.array_equal(o.query_packed(k, T.pack(t["queries"], k)), ans)
    canon = [T.from_str(O.min_kmer(s)) for s in strs]
    assert canon == [T.canonical_u64(v, k) for v in t["queries"]], "canonical_u64 is not the oracle's min_kmer"
    want = np.array([T.lookup(table, c) for c in canon], dtype=np.int32)
    changed = ans != ans0
    assert changed.sum() >= len(t["rows"]) // 2
    # isolating the rest table: where swapping the table for an empty one changes the answer, the answer is the lookup's ...
    # (or, where the lookup finds nothing for the k-mer itself, it finds one of its 8 de Bruijn neighbours: the neighbour
    # candidates of the disambiguation ask the table too, kmodel.hpp:326-342 -- dense models at tiny k get there)
    full = 4 ** k - 1
    for i in np.nonzero(changed & (ans != want))[0].tolist():
        c = canon[i]
        nbs = [((c << 2) | x) & full for x in range(4)] + [(c >> 2) | (x << (2 * (k - 1))) for x in range(4)]
        assert want[i] == 0 and any(T.lookup(table, T.canonical_u64(v, k)) for v in nbs), strs[i]
    # ... and wherever the lookup finds something that is the answer (kmodel.hpp:100-116 returns it before any filter)
    assert np.array_equal(ans[want != 0], want[want != 0])

    n = len(t["rows"])
    reach = np.array([canon[i] == t["rows"][i] for i in range(n)])
    own = ans[:n] == np.array(t["counts"])
    # (a) stored rows answer with their own count: all of them up to k = 32 -- but T...T where the k-mer is all prefix, which
    # no query reaches --, at least half above (the reference canonicalises through one u64 there)
    if k <= 32:
        expect = np.array([not (k == pre_len and v == 4 ** k - 1) for v in t["rows"]])
        assert np.array_equal(own, expect) and np.array_equal(reach, expect)
    else:
        assert own.sum() * 2 >= n and np.array_equal(own, reach)
    # and their reverse complements too, up to k = 32
    if k <= 32:
        assert np.array_equal(ans[n:2 * n] == np.array(t["counts"]), expect)

    by_q = dict(zip(t["queries"], ans.tolist()))
    nf = [(by_q[q], c, g) for q, c, g in t["next_first"]]
    print(f"(b) k={k} pre_len={pre_len}: next-group-first-suffix answers {[a for a, _, _ in nf]}")
    if k > pre_len:
        # (b) the inclusive bound answers: the next group's first count where that row is above the whole group, 0 elsewhere
        assert sum(a == c and g for a, c, g in nf) >= 2
        # (at k < 8 the 2 000 draws of the model underneath are most of the k-mers there are, and its filters answer whatever
        # the table does not: there "0" is the answer of the same model with an empty table)
        by_q0 = dict(zip(t["queries"], ans0.tolist()))
        zero = [a == (0 if k >= 8 else by_q0[q]) and T.lookup(table, T.canonical_u64(q, k)) == 0 for (a, _, g), (q, _, _) in zip(nf, t["next_first"]) if not g]
        assert sum(zero) >= 1
    else:
        # no suffix bases: every key of an existing prefix compares equal to its group's row, the bound has nothing to add
        assert all(a == T.lookup(table, T.canonical_u64(q, k)) for (a, _, _), (q, _, _) in zip(nf, t["next_first"]))

    # (c) keys above every row of the last group end on the row past the table: 0.  The first is one a query reaches,
    # wherever the shape has such a key (k == 2 pre_len has none: T^p A^p is the smallest key of its group)
    if k > pre_len:
        last = t["rows"][-1]
        assert t["d3"] and all(q > last and q >> (2 * (k - pre_len)) == last >> (2 * (k - pre_len)) for q in t["d3"])
        assert all(T.lookup(table, q) == 0 for q in t["d3"])
        reached = [q for q in t["d3"] if T.canonical_u64(q, k) == q]
        assert all(by_q[q] == (0 if k >= 8 else by_q0[q]) for q in reached)
        assert k == 2 * pre_len or reached[0] == t["d3"][0]

    # (e) dirty variants of reachable rows: N, n, X and - read as A, so they find the row
    dirty, dwant = [], []
    for i in np.nonzero(reach)[0].tolist():
        for s in T.dirty_variants(strs[i]):
            dirty.append(s)
            dwant.append(t["counts"][i])
    assert len(dirty) >= 40
    dans = o.query_strings(dirty)
    assert (dans != 0).sum() * 2 >= len(dirty)
    assert np.array_equal(dans, np.array(dwant)), "a dirty string that packs to a reachable row answers with its count"

    # (f) Q7: a string of another length never matches a row
    for cut in ([s[:-1] for s in strs[:n]], [s + "A" for s in strs[:n]], [s + "C" for s in strs[:n]]):
        assert np.array_equal(o.query_strings(cut), o0.query_strings(cut))


@pytest.mark.parametrize("k,pre_len", [(31, 7), (55, 7)])
def test_compiled_reference_agrees(rest_base, tmp_path, k, pre_len):
    if not O.have_ref():
        pytest.skip("the compiled reference driver is not built")
    t, table, o, o0, strs, ans, ans0 = answers(rest_base, k, pre_len)
    d3 = set(t["d3"])                                       # there the reference reads one row past its table (D3)
    keep = [i for i, q in enumerate(t["queries"]) if q not in d3]
    got = O.ref_query(T.model_dirs(rest_base, k, pre_len)[0], [strs[i] for i in keep], str(tmp_path / "ref"))
    assert np.array_equal(got, ans[keep])
