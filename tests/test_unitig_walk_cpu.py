"""CPU: the plain-Python restatement of kmx_unitig_walk_segs (tests/unitig_walk_ref.py) satisfies the consequences include/kmx.h
states, on every case the GPU tests compare the library with: no unlinked neighbours, walks that partition the segments, walks
without a bridge that spell their read, the mirror image under reverse complement, max_gap = k as the threshold of a single
substitution, every join kind and both signs of d in the new case, and the GAF text of a small case."""
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_walk_ref as W
import unitigs_ref as U


@pytest.mark.parametrize("name", W.WALK_CASES)
def test_consequences_on_every_case(name):
    k, km, cnt, thr, strs, reads, rows = W.case(name)
    segs, so = W.mapped(name)
    for max_gap, max_indel in W.params_of(k):
        walks, wo, steps, hits, st = W.walked(name, max_gap, max_indel)
        W.check(k, strs, reads, segs, so, walks, wo, steps, st)
        assert st["n_unlinked"] == 0
        assert sum(hits) == st["n_edge"] + st["n_across"]
        flat = W.flat(walks, wo, steps, hits, st)
        assert flat[0].dtype.itemsize == 80 and len(flat[4]) == 8
        if max_gap == 0:
            assert st["n_inside"] == st["n_across"] == 0 and all(w["indel"] == 0 for w in walks)


@pytest.mark.parametrize("name", W.WALK_CASES)
def test_reverse_complement_mirrors_the_walks(name):
    """consequence (c), read by read on every read of plain uppercase ACGT: the walks of the reverse complement are the mirrored
    walks, steps reversed with ^ 1, link_hits moved to the mirror edge"""
    k, km, cnt, thr, strs, reads, rows = W.case(name)
    plain = [r for r in reads if len(r) >= k and set(r) <= set("ACGT")]
    assert plain
    both = plain + [U.rc(r) for r in plain]
    segs, so, _, _ = R.map_reads(km, k, strs, both)              # one batch: the places are built once
    starts = [0]
    for r in both:
        starts.append(starts[-1] + len(r))

    def alone(i):
        """the segments of read i as if it were mapped alone, at flat position 0"""
        return [dict(g, pos=g["pos"] - starts[i]) for g in segs[so[i]:so[i + 1]]]

    seen = 0
    for i, read in enumerate(plain):
        fwd, rev = alone(i), alone(len(plain) + i)
        assert rev == R.mirrored(k, strs, fwd, len(read))
        for max_gap, max_indel in W.params_of(k):
            walks, wo, steps, hits, st = W.walk_segs(k, strs, fwd, [0, len(fwd)], rows, max_gap, max_indel)
            got = W.walk_segs(k, strs, rev, [0, len(rev)], rows, max_gap, max_indel)
            mw, ms, mh = W.mirrored(k, strs, rows, walks, steps, hits, len(read))
            assert got[0] == mw and got[2] == ms and got[3] == mh and got[4] == st
            seen += len(walks)
    assert seen > 0


def test_max_gap_k_is_what_bridges_a_substitution():
    """one substitution removes k windows: max_gap = k - 1 bridges none of them, max_gap = k does (the cleaned graph: one unitig,
    so every bridge is INSIDE with d = 0)"""
    name = "k21_noisy_clean"
    k, km, cnt, thr, strs, reads, rows = W.case(name)
    assert len(strs) == 1
    below, at = W.walked(name, k - 1, 0)[4], W.walked(name, k, 0)[4]
    assert below["n_inside"] == 0 == below["n_across"] and at["n_inside"] >= 20 and at["n_across"] == 0
    genome = U.rand_seq(600, 5)
    km2, cnt2 = U.listing_of(U.count_kmers([genome], k))
    strs2, _ = U.unitigs(km2, cnt2, k, 1)
    read = genome[100:300]
    read = read[:90] + ("A" if read[90] != "A" else "C") + read[91:]
    segs, so, _, _ = R.map_reads(km2, k, strs2, [read])
    assert len(segs) == 2 and segs[1]["pos"] - segs[0]["pos"] - segs[0]["n_windows"] == k
    rows2 = L.links(km2, cnt2, k, 1, strs2)
    assert W.walk_segs(k, strs2, segs, so, rows2, k - 1, 0)[4]["n_walks"] == 2
    walks, wo, steps, hits, st = W.walk_segs(k, strs2, segs, so, rows2, k, 0)
    assert st["n_walks"] == 1 and st["n_inside"] == 1 and walks[0]["indel"] == 0 and walks[0]["n_span"] == len(read) - k + 1
    assert walks[0]["n_covered"] == len(read) - 1                # every base but the substituted one lies in a mapped window


def test_every_join_kind_and_both_signs_of_d():
    name = W.NEW_CASE
    k, km, cnt, thr, strs, reads, rows = W.case(name)
    assert k == 21 and len(strs) == 25 and len(reads) == 440
    walks, wo, steps, hits, st = W.walked(name, 2 * k, 1)
    assert st["n_edge"] > 100 and st["n_inside"] > 100 and st["n_across"] > 10
    assert {w["indel"] for w in walks} >= {-1, 0, 1}
    tight = W.walked(name, k, 0)[4]
    assert 0 < tight["n_inside"] < st["n_inside"] and 0 < tight["n_across"] <= st["n_across"] and tight["n_edge"] == st["n_edge"]
    wide = W.walk_segs(k, strs, *W.mapped(name), rows, 2 * k, 2)
    assert max(w["indel"] for w in wide[0]) == 2
    name = "k21_noisy_clean"
    assert {w["indel"] for w in W.walked(name, 21, 1)[0]} <= {-1, 0, 1}


GAF_PINNED = ("0\t19\t0\t19\t+\t>u1\t19\t0\t19\t19\t19\t255\tid:i:0\tbg:i:0\n"
              "1\t19\t0\t19\t+\t<u1\t19\t0\t19\t19\t19\t255\tid:i:0\tbg:i:0\n")


def test_gaf_text():
    """the columns, on walks built by hand and on a case"""
    k = 5
    strs = ["ACGTTGCAAT", "GGATCCATTCAAGTCGATC"]
    walks = [{"pos": 0, "n_span": 15, "n_covered": 19, "first_step": 0, "n_steps": 1, "off_first": 0, "off_last": 14, "n_inside": 0, "n_across": 0, "indel": 0},
             {"pos": 19, "n_span": 15, "n_covered": 19, "first_step": 1, "n_steps": 1, "off_first": 0, "off_last": 14, "n_inside": 0, "n_across": 0, "indel": 0}]
    assert W.gaf(k, strs, [strs[1], U.rc(strs[1])], walks, [0, 1, 2], [2, 3]) == GAF_PINNED
    walks = [{"pos": 2, "n_span": 9, "n_covered": 11, "first_step": 0, "n_steps": 2, "off_first": 3, "off_last": 1, "n_inside": 0, "n_across": 1, "indel": -1}]
    assert W.gaf(k, strs, ["N" * 20], walks, [0, 1], [1, 2], first_read=7) == "7\t20\t2\t15\t+\t<u0>u1\t25\t3\t12\t11\t13\t255\tid:i:-1\tbg:i:1\n"
    name = "k21_cycle_and_tip"
    kk, km, cnt, thr, strs, reads, rows = W.case(name)
    walks, wo, steps, hits, st = W.walked(name, kk, 0)
    text = W.gaf(kk, strs, reads, walks, wo, steps)
    lines = text.splitlines()
    assert len(lines) == st["n_walks"] and all(len(x.split("\t")) == 14 for x in lines)
    for x, w in zip(lines, walks):
        c = x.split("\t")
        assert int(c[3]) - int(c[2]) == w["n_span"] + kk - 1 and c[4] == "+" and c[11] == "255" and int(c[8]) <= int(c[6])
