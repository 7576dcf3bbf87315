"""kmx_unitig_walk_segs* on the MI355X: walks, walk_offsets, steps, link_hits and stats equal, byte for byte, what the plain-Python
restatement of the rule (tests/unitig_walk_ref.py) gives, for the host and the device form after both forms of begin, on every
case and at three parameter pairs; one walk of 2 * 10^4 segments across every block and scan tile of the new kernels, with empty
reads and walk starts at a block's edges; the sizing call and the two capacities; accumulation; allocation failures; refusals;
crafted device input; the facade and the driver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_walk_ref as W
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import SEQ_SEGMENT_DTYPE, WALK_DTYPE, KmxError, WalkParams, WalkStats

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the segments
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def long_walk_case():
    """k5_complete (every canonical 5-mer is listed and is its own unitig, so every window is a segment and every neighbour an
    EDGE join): one read of 20 000 random bases whose first segment is the last lane of block 0, with reads of 0, k - 1 and k
    bases and one that maps nothing in front; a read that ends exactly at the end of block 79; the case's short reads from the
    first lane of block 80; empty reads at either side of both edges"""
    k, km, cnt, thr, strs, reads, rows = W.case("k5_complete")
    mine = [U.rand_seq(k - 1, 41), U.rand_seq(k, 42), "N" * 30, "", U.rand_seq(254 + k - 1, 43), "", U.rand_seq(20000, 44), "", "", U.rand_seq(229 + k - 1, 45), ""] + list(reads) + [""]
    return k, km, cnt, thr, strs, mine, rows


LOCAL = {"long_walk": long_walk_case}


@functools.lru_cache(maxsize=None)
def ref(name):
    """a case, the map's restatement of its reads and the CSR, computed once -> (k, km, strs, reads, rows, segs, so, loff, lk)"""
    if name in LOCAL:
        k, km, cnt, thr, strs, reads, rows = LOCAL[name]()
        segs, so, _, _ = R.map_reads(km, k, strs, reads)
    else:
        k, km, cnt, thr, strs, reads, rows = W.case(name)
        segs, so = W.mapped(name)
    loff, lk = L.flat_links(rows)
    return k, km, strs, reads, rows, segs, so, loff, lk


@functools.lru_cache(maxsize=None)
def want(name, max_gap, max_indel):
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    return W.flat(*W.walk_segs(k, strs, segs, so, rows, max_gap, max_indel))


def same(got, exp, what=""):
    for a, b, part in zip(got, exp, W.PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"


def stats_array(st):
    return np.array([st[f] for f in W.STAT_FIELDS], dtype=np.uint64)


def begin(m, how, km, k, strs):
    import torch
    packed = U.pack(km, k)
    if how == "host":
        m.unitig_map_begin(packed, k, *R.join(strs))
    else:
        d_km = torch.from_numpy(np.ascontiguousarray(packed).view(np.int64).reshape(-1)).cuda()
        m.unitig_map_begin_dev(d_km, k, *dev_pair(strs))


def dev_pair(strs):
    import torch
    buf, off = R.join(strs)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()


def run_host(m, name, max_gap, max_indel):
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    hits = np.zeros(len(lk), dtype=np.uint64)
    walks, wo, steps, st, gsegs, gso = m.seq_to_walks(reads, loff, lk, max_gap, max_indel, link_hits=hits)
    assert len(gsegs) == len(segs) and gso.tolist() == list(so)
    return walks, wo, steps, hits, stats_array(st)


def dev_mapped(m, name):
    """the reads mapped on the device: (d_segs uint8 [capacity, 24], n_segs, d_seg_offsets, d_link_offsets, d_links)"""
    import torch
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    d_seq, d_off = dev_pair(reads)
    d_segs = torch.zeros((max(d_seq.numel(), 1), 24), dtype=torch.uint8, device="cuda")
    ns, d_so = m.seq_to_unitigs_dev(d_seq, d_off, d_segs)
    assert ns == len(segs)
    return d_segs, ns, d_so, torch.from_numpy(loff.view(np.int64)).cuda(), torch.from_numpy(lk.view(np.int32)).cuda()


def run_dev(m, name, max_gap, max_indel, mapped=None):
    import torch
    d_segs, ns, d_so, d_lo, d_lk = mapped or dev_mapped(m, name)
    d_walks = torch.zeros((max(ns, 1), 80), dtype=torch.uint8, device="cuda")
    d_steps = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
    d_hits = torch.zeros(max(d_lk.numel(), 1), dtype=torch.int64, device="cuda")
    st, d_wo = m.unitig_walks_dev(d_segs, ns, d_so, d_lo, d_lk, max_gap, max_indel, d_walks, d_steps, None, d_hits)
    torch.cuda.synchronize()
    return (d_walks.cpu().numpy()[:st["n_walks"]].reshape(-1).view(WALK_DTYPE), d_wo.cpu().numpy().view(np.uint64), d_steps.cpu().numpy().view(np.uint32)[:st["n_steps"]],
            d_hits.cpu().numpy().view(np.uint64)[:d_lk.numel()], stats_array(st))


def all_four(m, name, pairs):
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    for how in ("host", "dev"):                                 # the second begin ends the first session
        begin(m, how, km, k, strs)
        mapped = dev_mapped(m, name)
        for max_gap, max_indel in pairs:
            exp = want(name, max_gap, max_indel)
            same(run_host(m, name, max_gap, max_indel), exp, f"{name} {max_gap, max_indel}: begin {how}, host")
            same(run_dev(m, name, max_gap, max_indel, mapped), exp, f"{name} {max_gap, max_indel}: begin {how}, device")
    m.unitig_map_end()


@pytest.mark.parametrize("name", W.WALK_CASES)
def test_equals_the_restatement(name):
    """every case of the map tests with the rows of its graph (the cleaned graph's for k21_noisy_clean) and the case that reaches
    every join kind, at (0, 0), (k, 0) and (2 k, 1)"""
    k = ref(name)[0]
    all_four(KModel(1, 1023, NH, NB), name, W.params_of(k))
    assert len(want(name, k, 0)[0]) > 0
    if name == W.NEW_CASE:
        st = dict(zip(W.STAT_FIELDS, want(name, 2 * k, 1)[4].tolist()))
        assert min(st["n_edge"], st["n_inside"], st["n_across"]) > 0 and {-1, 0, 1} <= set(want(name, 2 * k, 1)[0]["indel"].tolist())
        all_four(KModel(1, 1023, NH, NB), name, ((2 * k, 2),))
        assert 2 in want(name, 2 * k, 2)[0]["indel"].tolist()


def test_one_walk_across_every_block_and_reads_at_the_block_edges():
    name = "long_walk"
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    walks, wo, steps, hits, st = want(name, 0, 0)
    big = int(np.argmax(walks["n_segs"]))
    assert walks["n_segs"][big] == walks["n_steps"][big] == 20000 - k + 1 and walks["first_seg"][big] == 255
    starts = {int(so[i]) % 256 for i in range(len(reads)) if so[i + 1] > so[i]}
    assert {255, 0} <= starts and int(so[10]) == 80 * 256 and reads[5] == reads[7] == reads[10] == ""
    assert st[W.STAT_FIELDS.index("n_unlinked")] == 0
    all_four(KModel(1, 1023, NH, NB), name, ((0, 0), (2 * k, 1)))


def raw_dev(m, mapped, params, walk_cap, step_cap, give_walks=True, give_hits=True, n_seqs=None):
    """one kmx_unitig_walk_segs_dev call on buffers longer than it is told, filled with guard bytes
    -> (rc, stats, walks bytes, walk_offsets, steps, link_hits)"""
    import torch
    d_segs, ns, d_so, d_lo, d_lk = mapped
    n_seqs = d_so.numel() - 1 if n_seqs is None else n_seqs
    n_links = d_lk.numel()
    walks = torch.full(((walk_cap + 4) * 80,), 0xA5, dtype=torch.uint8, device="cuda")
    steps = torch.full((step_cap + 8,), -3, dtype=torch.int32, device="cuda")
    wo = torch.full((n_seqs + 1 + 8,), -6, dtype=torch.int64, device="cuda")
    hits = torch.zeros(n_links + 8, dtype=torch.int64, device="cuda")
    hits[n_links:] = -7
    par = params if isinstance(params, WalkParams) else WalkParams(*params)
    st = WalkStats()
    rc = m.L.kmx_unitig_walk_segs_dev(m.h, d_segs.data_ptr(), ns, d_so.data_ptr(), n_seqs, d_lo.data_ptr(), d_lk.data_ptr(), n_links, C.byref(par),
                                      walks.data_ptr() if give_walks else None, walk_cap, wo.data_ptr(), steps.data_ptr() if give_walks else None, step_cap,
                                      hits.data_ptr() if give_hits else None, C.byref(st))
    torch.cuda.synchronize()
    return rc, st.as_dict(), walks.cpu().numpy(), wo.cpu().numpy(), steps.cpu().numpy(), hits.cpu().numpy()


def test_sizing_call_capacities_and_guards():
    """the sizing call; both capacities exact; each one short in turn: KMX_E_RANGE with stats, walk_offsets and link_hits complete and
    nothing written at or behind either capacity; the session survives and succeeds; the host form reports the same"""
    name, pair = W.NEW_CASE, (42, 1)
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    ww, wwo, wsteps, whits, wst = want(name, *pair)
    nw, nst, nr, nl = len(ww), len(wsteps), len(reads), len(lk)
    assert nw < nst < len(segs)
    m = KModel(1, 1023, NH, NB)
    begin(m, "dev", km, k, strs)
    mapped = dev_mapped(m, name)

    def complete(st, wo, hits):
        return (stats_array(st).tobytes() == wst.tobytes() and wo[:nr + 1].tobytes() == wwo.tobytes() and np.all(wo[nr + 1:] == -6) and
                hits[:nl].tobytes() == whits.tobytes() and np.all(hits[nl:] == -7))

    rc, st, walks, wo, steps, hits = raw_dev(m, mapped, pair, 0, 0, give_walks=False)
    assert rc == 0 and complete(st, wo, hits) and np.all(walks == 0xA5) and np.all(steps == -3)
    for wcap, scap in ((nw - 1, nst), (nw, nst - 1)):
        rc, st, walks, wo, steps, hits = raw_dev(m, mapped, pair, wcap, scap)
        assert rc == -5 and complete(st, wo, hits) and np.all(walks[wcap * 80:] == 0xA5) and np.all(steps[scap:] == -3)
    rc, st, walks, wo, steps, hits = raw_dev(m, mapped, pair, nw, nst)
    assert rc == 0 and complete(st, wo, hits) and walks[:nw * 80].tobytes() == ww.tobytes() and np.all(walks[nw * 80:] == 0xA5)
    assert steps[:nst].view(np.uint32).tobytes() == wsteps.tobytes() and np.all(steps[nst:] == -3)
    rc, st, walks, wo, steps, hits = raw_dev(m, mapped, pair, nw, nst, give_hits=False)
    assert rc == 0 and walks[:nw * 80].tobytes() == ww.tobytes() and not hits[:nl].any()
    gsegs, gso, _ = m.seq_to_unitigs(reads)
    for wcap, scap in ((nw - 1, nst), (nw, nst - 1)):
        h = np.zeros(nl, dtype=np.uint64)
        with pytest.raises(KmxError) as e:
            m.unitig_walks_flat(gsegs, gso, loff, lk, *pair, walk_capacity=wcap, step_capacity=scap, link_hits=h)
        assert e.value.code == -5 and h.tobytes() == whits.tobytes()
    h = np.zeros(nl, dtype=np.uint64)
    walks, wo, steps, st = m.unitig_walks_flat(gsegs, gso, loff, lk, *pair, walk_capacity=nw, step_capacity=nst, link_hits=h)
    same((walks, wo, steps, h, stats_array(st)), (ww, wwo, wsteps, whits, wst), "host, exact capacities")
    m.unitig_map_end()


def test_link_hits_accumulate_and_empty_batches():
    import torch
    name, pair = "k31_tangle", (31, 0)
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    exp = want(name, *pair)
    m = KModel(1, 1023, NH, NB)
    begin(m, "host", km, k, strs)
    hits = np.zeros(len(lk), dtype=np.uint64)
    m.seq_to_walks(reads[:10], loff, lk, *pair, link_hits=hits)
    m.seq_to_walks(reads[10:], loff, lk, *pair, link_hits=hits)
    assert np.array_equal(hits, exp[3]) and hits.any()
    mapped = dev_mapped(m, name)
    d_hits = torch.zeros(len(lk), dtype=torch.int64, device="cuda")
    for _ in range(2):
        m.unitig_walks_dev(*mapped, *pair, None, None, None, d_hits)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint64), 2 * exp[3])
    par, st = WalkParams(31, 0), WalkStats()
    st.n_walks = 9                                                # n_seqs == 0: KMX_OK, all-zero stats, nothing else written
    assert m.L.kmx_unitig_walk_segs(m.h, None, 0, None, 0, None, None, 0, C.byref(par), None, 0, None, None, 0, None, C.byref(st)) == 0 and st.n_walks == 0
    walks, wo, steps, st, gsegs, gso = m.seq_to_walks(["", "", ""], loff, lk, *pair)       # reads without segments
    assert len(walks) == 0 == len(steps) and wo.tolist() == [0, 0, 0, 0] and not any(st.values())
    m.unitig_map_end()


def test_allocation_failure_leaves_handle_and_session_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first walk call in turn, host and device form: the session stays open and the same call
    then succeeds with the right bytes"""
    name, pair = "k21_cycle_and_tip", (21, 0)
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    exp = want(name, *pair)
    failed = {"host": 0, "dev": 0}
    for nth in range(1, 15):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            begin(m, variant, km, k, strs)
            mapped = dev_mapped(m, name) if variant == "dev" else None
            gs = m.seq_to_unitigs(reads) if variant == "host" else None
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                if variant == "host":
                    m.unitig_walks_flat(gs[0], gs[1], loff, lk, *pair)
                else:
                    run_dev(m, name, *pair, mapped)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run_host(m, name, *pair) if variant == "host" else run_dev(m, name, *pair, mapped), exp, f"after allocation {nth} failed, {variant}")
            m.unitig_map_end()
    assert failed["host"] >= 8 and failed["dev"] >= 4, failed


def test_refusals():
    """outside a session; max_indel = 256; non-zero reserved; seg_offsets that start above 0, decrease or end short of n_segs, and a
    links entry >= 2 U, in the host form; the handle then walks as if nothing had happened"""
    name, pair = "k31_tangle", (31, 0)
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    m = KModel(1, 1023, NH, NB)
    fs = R.flat(segs, so, [], [])[0]
    fso = np.array(so, dtype=np.uint64)
    with pytest.raises(KmxError) as e:
        m.unitig_walks_flat(fs, fso, loff, lk, *pair)
    assert e.value.code == -4
    begin(m, "host", km, k, strs)
    gsegs, gso, _ = m.seq_to_unitigs(reads)
    assert gsegs.tobytes() == fs.tobytes()
    mapped = dev_mapped(m, name)

    def host_rc(par, so_=gso, lo_=loff, lk_=lk):
        st = WalkStats()
        wo = np.zeros(len(so_), dtype=np.uint64)
        return m.L.kmx_unitig_walk_segs(m.h, gsegs.ctypes.data, len(gsegs), so_.ctypes.data, len(so_) - 1, lo_.ctypes.data, lk_.ctypes.data, len(lk_), C.byref(par), None, 0,
                                        wo.ctypes.data, None, 0, None, C.byref(st))

    assert host_rc(WalkParams(31, 0)) == 0
    bad_reserved = WalkParams(31, 0)
    bad_reserved.reserved[1] = 1
    for par in (WalkParams(31, 256), bad_reserved):
        assert host_rc(par) == -1
        assert raw_dev(m, mapped, par, 0, 0, give_walks=False)[0] == -1
    swapped = gso.copy()
    swapped[1], swapped[2] = gso[2], gso[1]
    assert gso[1] != gso[2]
    short = gso.copy()
    short[-1] -= 1
    above = gso.copy()
    above[0] = 1
    for bad in (swapped, short, above):
        assert host_rc(WalkParams(31, 0), so_=bad) == -1
    bad_lk = lk.copy()
    bad_lk[len(lk) // 2] = 2 * len(strs)
    assert host_rc(WalkParams(31, 0), lk_=bad_lk) == -1
    bad_lo = loff.copy()
    bad_lo[3], bad_lo[4] = loff[4] + 1, loff[3]
    assert host_rc(WalkParams(31, 0), lo_=bad_lo) == -1
    same(run_host(m, name, *pair), want(name, *pair), "after the refusals")
    m.unitig_map_end()
    with pytest.raises(KmxError) as e:
        m.unitig_walks_flat(gsegs, gso, loff, lk, *pair)
    assert e.value.code == -4
    assert raw_dev(m, mapped, pair, 0, 0, give_walks=False)[0] == -4


def test_crafted_device_input_stays_inside_the_buffers():
    """the _dev form clamps: segments with o >= 2 U, descending pos, zero and huge n_windows, row bounds beyond n_links and decreasing,
    seg_offsets beyond n_segs and decreasing: KMX_OK, wrong walks, and the guard bytes around walks, walk_offsets, steps and link_hits
    are intact"""
    import torch
    name, pair = "k31_tangle", (62, 1)
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    m = KModel(1, 1023, NH, NB)
    begin(m, "dev", km, k, strs)
    d_segs, ns, d_so, d_lo, d_lk = dev_mapped(m, name)
    good = d_segs.cpu().numpy()[:ns].reshape(-1).view(SEQ_SEGMENT_DTYPE)
    nr, nl, U2 = len(reads), len(lk), 2 * len(strs)
    big = np.uint64(2 ** 64 - 1)
    r = np.random.RandomState(5)

    def segs_with(**f):
        s = good.copy()
        for name_, v in f.items():
            s[name_] = v
        return torch.from_numpy(s.view(np.uint8).reshape(-1, 24)).cuda()

    bad_segs = [segs_with(o=np.where(np.arange(ns) % 3 == 1, U2 + r.randint(0, 5, ns), good["o"]).astype(np.uint32)), segs_with(o=np.full(ns, 0xFFFFFFFF, np.uint32)),
                segs_with(pos=good["pos"][::-1].copy()), segs_with(n_windows=np.where(np.arange(ns) % 2 == 0, 0, 0xFFFFFFFF).astype(np.uint32)),
                segs_with(off=np.full(ns, 0xFFFFFFFF, np.uint32), pos=np.full(ns, big))]
    bad_lo = [loff + np.uint64(nl), loff[::-1].copy(), np.full(len(loff), big), np.where(np.arange(len(loff)) % 2 == 1, big, loff)]
    fso = np.array(so, dtype=np.uint64)
    bad_so = [fso[::-1].copy(), fso + np.uint64(ns), np.full(nr + 1, big), np.zeros(nr + 1, np.uint64)]
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    crafted = [(s, d_so, d_lo) for s in bad_segs] + [(d_segs, d_so, to_dev(x)) for x in bad_lo] + [(d_segs, to_dev(x), d_lo) for x in bad_so] + [(bad_segs[0], to_dev(bad_so[0]), to_dev(bad_lo[3]))]
    for s, o, lo in crafted:
        rc, st, walks, wo, steps, hits = raw_dev(m, (s, ns, o, lo, d_lk), pair, ns, ns)
        assert rc == 0 and st["n_walks"] <= ns and st["n_steps"] <= ns
        assert np.all(walks[ns * 80:] == 0xA5) and np.all(wo[nr + 1:] == -6) and np.all(steps[ns:] == -3) and np.all(hits[nl:] == -7)
    rc, st, walks, wo, steps, hits = raw_dev(m, (d_segs, ns, d_so, d_lo, d_lk), pair, ns, ns)
    exp = want(name, *pair)
    assert rc == 0 and walks[:len(exp[0]) * 80].tobytes() == exp[0].tobytes() and wo[:nr + 1].tobytes() == exp[1].tobytes()
    m.unitig_map_end()


def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_walk.cpp prints what seq_walks returns for the case that reaches every join kind, and the driver's
    -u2 -M -W writes reads.gaf and unitigs.links.tsv: both equal the restatement's text"""
    import count_reads as CR
    name = W.NEW_CASE
    k, km, strs, reads, rows, segs, so, loff, lk = ref(name)
    thr, noisy = 2, reads[:400]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in noisy])
    lines = str(tmp_path / "reads.txt")
    with open(lines, "w") as f:
        f.write("".join(r + "\n" for r in reads))

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    def link_table(hits):
        return "".join(f"{int(loff[a]) + j}\tu{a >> 1}{'-' if a & 1 else '+'}\tu{b >> 1}{'-' if b & 1 else '+'}\t{hits[int(loff[a]) + j]}\n" for a, row in enumerate(rows) for j, b in enumerate(row))

    walks, wo, steps, hits, st = W.walk_segs(k, strs, segs, so, rows, 42, 2)
    fw = W.flat(walks, wo, steps, hits, st)
    out = subprocess.check_output([build("tests/facade_unitig_walk.cpp", "facade_unitig_walk"), fa, str(k), str(thr), lines, "42", "2"], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 7
    assert blocks[0] == "".join(" ".join(str(int(w[f])) for f, _ in W.WALK_FIELDS) + "\n" for w in fw[0])
    assert blocks[1] == "".join(f"{x}\n" for x in wo) and blocks[2] == "".join(f"{x}\n" for x in steps) and blocks[3] == "".join(f"{x}\n" for x in hits)
    assert blocks[4] == " ".join(str(st[f]) for f in W.STAT_FIELDS) + "\n"
    assert blocks[5] == W.gaf(k, strs, reads, walks, wo, steps) and blocks[6] == link_table(hits)
    # the driver maps the reads of its input, the 400 noisy reads, at the defaults max_gap = k, max_indel = 1
    nsegs, nso, _, _ = R.map_reads(km, k, strs, noisy)
    walks, wo, steps, hits, st = W.walk_segs(k, strs, nsegs, nso, rows, k, 1)
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    plain, with_walks = tmp_path / "plain", tmp_path / "walked"
    plain.mkdir()
    with_walks.mkdir()
    subprocess.check_call([exe, "-g", f"-u{thr}", "-M", f"-k{k}", "-nh3", "-nb2", fa, "db", str(plain)], timeout=120)
    log = subprocess.check_output([exe, "-g", f"-u{thr}", "-M", "-W", f"-k{k}", "-nh3", "-nb2", fa, "db", str(with_walks)], timeout=120).decode()
    assert (with_walks / "db" / "reads.gaf").read_text() == W.gaf(k, strs, noisy, walks, wo, steps)
    assert (with_walks / "db" / "unitigs.links.tsv").read_text() == link_table(hits)
    assert f"{st['n_walks']} walks, {st['n_steps']} steps" in log
    assert (plain / "db" / "reads.paths.tsv").read_text() == (with_walks / "db" / "reads.paths.tsv").read_text()
    assert not (plain / "db" / "reads.gaf").exists() and not (plain / "db" / "unitigs.links.tsv").exists() and not (with_walks / "db" / "unitigs.gfa").exists()
    assert subprocess.call([exe, "-g", f"-u{thr}", "-W", f"-k{k}", fa, "db", str(plain)], stdout=subprocess.DEVNULL) == 2     # -W without -M
