"""kmx_unitig_scaffold_fill* on the MI355X: the bases, offsets, records, steps, pieces and stats equal, byte for byte, what the
plain-Python restatement of the rule (tests/unitig_scaffold_fill_ref.py) gives, for the host and the device form (the device
form always between guard bands): on the acceptance case and the two islands through the library's scaffold and pair-path calls,
on crafted sets with every feature of the rule and every value of kinds, at the geometry of the gather emit (piece tiles, one-byte
pieces, a piece longer than a tile, all 16 destination alignments, steps and entries at the block edges); KMX_E_RANGE for the bases
and for the pieces, the sizing call, the refusals, crafted device input, determinism, the facade and the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import unitig_links_ref as L
import unitig_map_ref as R
import unitig_pair_paths_ref as Q
import unitig_pairs_ref as P
import unitig_scaffold_fill_ref as F
import unitig_scaffold_ref as S
import unitigs_ref as U
from kmcex_amd import KModel
from kmcex_amd.api import FillParams, FillStats, KmxError

pytestmark = pytest.mark.gpu

NH, NB = 3, 2                                                  # small models: the tests are about the filled scaffolds
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
PARTS = ("fseq", "foffsets", "frec", "fsteps", "pieces")


@pytest.fixture(scope="module")
def model():
    return KModel(1, 1023, NH, NB)


def expected(c, kinds=3):
    res = F.fill_of(c, kinds)
    F.check(c["k"], c["strs"], c["srecs"], c["steps"], c["plinks"], c["precs"], c["psteps"], kinds, res)
    return F.flat(res)


def same(got, exp, what):
    for a, b, part in zip(got[:5], exp[:5], PARTS):
        assert np.asarray(a).tobytes() == b.tobytes(), f"{what}: {part} differ"
    assert got[5] == exp[5], f"{what}: stats differ: {got[5]} != {exp[5]}"


def run_host(m, c, kinds=3, **kw):
    ubuf, uoffs, srec, steps, pl, precs, pst = F.craft_arrays(c)
    return m.unitig_scaffold_fill_flat(c["k"], ubuf, uoffs, srec, steps, pl, precs, pst, kinds, **kw)


def to_dev(a, view=None):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return None
    return torch.from_numpy(a.view(view) if view else a).cuda()


def raw_dev(m, k, arrays, cap, pcap, kinds=3, sizing=False, no_pieces=False, n_scaffolds=None, n_plinks=None, n_psteps=None):
    """one kmx_unitig_scaffold_fill_dev call whose five outputs lie between guard bands of GUARD elements -> (rc, n_fbases, n_pieces,
    stats, the five outputs with their bands as NumPy arrays)"""
    import torch
    ubuf, uoffs, srec, steps, pl, precs, pst = arrays
    nu, nb, ns = len(uoffs) - 1, len(ubuf), len(srec)
    d_buf, d_off = to_dev(ubuf if nb else np.zeros(1, np.uint8)), to_dev(uoffs, np.int64)
    d_srec, d_steps = to_dev(srec.view(np.uint8).reshape(-1, 64)), to_dev(steps.view(np.uint8).reshape(-1, 16))
    d_pl, d_precs, d_pst = to_dev(pl.view(np.uint8).reshape(-1, 32)), to_dev(precs.view(np.uint8).reshape(-1, 32)), to_dev(pst, np.int32)
    fseq = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    foffs = torch.full((ns + 1 + 2 * GUARD,), -7, dtype=torch.int64, device="cuda")
    frec = torch.full((ns + 2 * GUARD, 64), 0xA5, dtype=torch.uint8, device="cuda")
    fsteps = torch.full((nu + 2 * GUARD, 32), 0xA5, dtype=torch.uint8, device="cuda")
    pieces = torch.full((pcap + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    p, st, nf, npc = FillParams(kinds, 0), FillStats(), C.c_uint64(0), C.c_uint64(0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = m.L.kmx_unitig_scaffold_fill_dev(m.h, k, d_buf.data_ptr(), d_off.data_ptr(), nu, nb, ptr(d_srec), ns if n_scaffolds is None else n_scaffolds, ptr(d_steps), ptr(d_pl),
                                          len(pl) if n_plinks is None else n_plinks, ptr(d_precs), ptr(d_pst), len(pst) if n_psteps is None else n_psteps, C.byref(p),
                                          None if sizing else fseq[GUARD:].data_ptr(), 0 if sizing else cap, foffs[GUARD:].data_ptr(), frec[GUARD:].data_ptr(), fsteps[GUARD:].data_ptr(),
                                          None if no_pieces else pieces[GUARD:].data_ptr(), 0 if no_pieces else pcap, C.byref(nf), C.byref(npc), C.byref(st))
    torch.cuda.synchronize()
    return rc, nf.value, npc.value, st.as_dict(), tuple(t.cpu().numpy() for t in (fseq, foffs, frec, fsteps, pieces))


def bands_intact(out, cap, pcap, nu, ns):
    fseq, foffs, frec, fsteps, pieces = out
    return (np.all(fseq[:GUARD] == 0xA5) and np.all(fseq[GUARD + cap:] == 0xA5) and np.all(foffs[:GUARD] == -7) and np.all(foffs[GUARD + ns + 1:] == -7) and
            np.all(frec[:GUARD] == 0xA5) and np.all(frec[GUARD + ns:] == 0xA5) and np.all(fsteps[:GUARD] == 0xA5) and np.all(fsteps[GUARD + nu:] == 0xA5) and
            np.all(pieces[:GUARD] == -7) and np.all(pieces[GUARD + pcap:] == -7))


def parts_of(out, nf, npc, nu, ns, st):
    fseq, foffs, frec, fsteps, pieces = out
    return (fseq[GUARD:GUARD + nf], foffs[GUARD:GUARD + ns + 1].view(np.uint64), frec[GUARD:GUARD + ns].reshape(-1).view(F.SCAFFOLD_FILL_DTYPE),
            fsteps[GUARD:GUARD + nu].reshape(-1).view(F.FILL_STEP_DTYPE), pieces[GUARD:GUARD + npc].view(np.uint32), st)


def run_dev(m, c, kinds=3, slack=0):
    """-> the six parts as run_host gives them, from kmx_unitig_scaffold_fill_dev between guard bands, at exact capacities + slack"""
    exp = F.flat(F.fill_of(c, kinds))
    arrays = F.craft_arrays(c)
    nu, ns = len(c["strs"]), len(c["srecs"])
    cap, pcap = len(exp[0]) + slack, len(exp[4]) + slack
    rc, nf, npc, st, out = raw_dev(m, c["k"], arrays, cap, pcap, kinds)
    if rc:
        raise KmxError(rc, m.L.kmx_last_error().decode(errors="replace"))
    assert bands_intact(out, cap, pcap, nu, ns) and nf <= cap and npc <= pcap
    assert np.all(out[0][GUARD + nf:GUARD + cap] == 0xA5) and np.all(out[4][GUARD + npc:GUARD + pcap] == -7)   # nothing behind what is promised
    return parts_of(out, nf, npc, nu, ns, st)


def both(m, c, what, kinds=3):
    exp = expected(c, kinds)
    same(run_host(m, c, kinds), exp, f"{what}: host")
    same(run_dev(m, c, kinds), exp, f"{what}: device")
    same(run_dev(m, c, kinds, slack=37), exp, f"{what}: device with room to spare")
    return exp


# ---- through the library's own scaffold and pair-path calls
def test_the_acceptance_case_and_the_two_islands_through_the_library(model):
    """scaffolds_from_pairs -> unitig_pair_paths_flat -> the fill call: the filled scaffolds are the two genome pieces with 0 N; the
    two islands keep their 100 N"""
    m = model
    a = F.acceptance()
    k, strs, plinks = a["k"], a["strs"], a["plinks"]
    scf, pth, res = F.through_restatements(k, strs, a["rows"], plinks, a["par"], a["path_par"])
    exp = F.flat(res)
    loff, lk = L.flat_links(a["rows"])
    pl = S.plinks_array(plinks)
    sstrs, srec, steps, place, _ = m.scaffolds_from_pairs(k, strs, pl, **a["par"])
    assert sstrs == scf["sstrs"]
    buf, off = R.join(strs)
    q = a["path_par"]
    prec, pst, _ = m.unitig_pair_paths_flat(k, off, loff, lk, pl, q["inner"], q["tol"], q["min_pairs"], q["max_steps"], q["max_visits"])
    assert prec.tobytes() == Q.flat(pth)[0].tobytes() and pst.tolist() == pth["psteps"]
    got = m.unitig_scaffold_fill_flat(k, buf, off, srec, steps, pl, prec, pst)
    same(got, exp, "acceptance: host")
    c = dict(k=k, strs=strs, srecs=F.srecs_of(scf), steps=scf["steps"], plinks=plinks, precs=pth["recs"], psteps=pth["psteps"])
    same(run_dev(m, c), exp, "acceptance: device")
    texts = [t for t in F.fill_of(c)["fstrs"] if len(t) > 25]
    assert sorted(min(t, U.rc(t)) for t in texts) == sorted(min(g, U.rc(g)) for g in a["pieces"]) and not any("N" in t for t in texts)
    fstrs, frec, fst, pcs, st, _, _ = m.filled_scaffolds_from_pairs(k, strs, loff, lk, pl, a["par"]["inner"], a["par"]["min_pairs"], tol=q["tol"])
    assert fstrs == res["fstrs"] and st == res["stats"] and st["n_removed"] == 20 and frec.tobytes() == exp[2].tobytes()
    for kinds in (0, 2):                                          # consequence (a): nothing is ADJACENT here
        assert run_host(m, c, kinds)[0].tobytes().decode() == "".join(scf["sstrs"])
    # the two islands: no path across the hole
    k, strs, plinks, genome = S.two_islands()
    rows = P.case("two_islands")[5]
    par = S.TWO_ISLANDS_PARAMS
    scf, pth, res = F.through_restatements(k, strs, rows, plinks, par, dict(min_pairs=par["min_pairs"], inner=par["inner"], tol=k, max_steps=8, max_visits=4096))
    loff, lk = L.flat_links(rows)
    fstrs, frec, fst, pcs, st, _, _ = m.filled_scaffolds_from_pairs(k, strs, loff, lk, S.plinks_array(plinks), par["inner"], par["min_pairs"], par["ratio"], par["min_n"], par["max_n"])
    assert fstrs == scf["sstrs"] == res["fstrs"] and fstrs[0].count("N") == 100 and st == res["stats"] and st["n_n"] == 1 and pcs.size == 0
    c = dict(k=k, strs=strs, srecs=F.srecs_of(scf), steps=scf["steps"], plinks=plinks, precs=pth["recs"], psteps=pth["psteps"])
    both(m, c, "two islands")


# ---- crafted sets: lists, records and steps written by hand
@pytest.mark.parametrize("kinds", (0, 1, 2, 3))
def test_the_mixed_set_at_every_value_of_kinds(model, kinds):
    """paths of 1 and 16 steps, pieces of one byte, a unitig on 5 paths that is also a step, entries through the mirror with reverse
    pieces, both entries present, PATH records with first_step + t > n_psteps, t = 0, t = 17 or a step >= 2 U (all N steps), a
    cycle, scaffolds of one step"""
    c = F.mixed()
    exp = both(model, c, f"mixed, kinds {kinds}", kinds)
    assert exp[5]["n_path"] == (7 if kinds & 1 else 0) and exp[5]["n_adjacent"] == (2 if kinds & 2 else 0)
    if kinds == 0:                                                # consequence (a): what the scaffold call spells from these steps
        spelled = "".join("".join(("N" * g if j else "") + S.oriented(c["strs"][o >> 1], o & 1) for j, (o, g, _) in enumerate(c["steps"][f:f + (n & (S.CIRCULAR - 1))])) for f, n in c["srecs"])
        assert exp[0].tobytes().decode() == spelled


def test_no_unitig_one_unitig_and_no_list(model):
    m = model
    e = np.zeros(0, np.uint8)
    got = m.unitig_scaffold_fill_flat(21, e, np.zeros(1, np.uint64), np.zeros(0, S.SCAFFOLD_DTYPE), np.zeros(0, S.STEP_DTYPE), np.zeros(0, P.PAIR_LINK_DTYPE), np.zeros(0, Q.PAIR_PATH_DTYPE), None)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2].size == got[3].size == got[4].size == 0 and got[5] == dict.fromkeys(F.STAT_FIELDS, 0)
    import torch
    d_so = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    d_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    p, st, nf, npc = FillParams(3, 0), FillStats(), C.c_uint64(9), C.c_uint64(9)
    assert m.L.kmx_unitig_scaffold_fill_dev(m.h, 21, None, d_off.data_ptr(), 0, 0, None, 0, None, None, 0, None, None, 0, C.byref(p), None, 0, d_so.data_ptr(), None, None, None, 0, C.byref(nf),
                                            C.byref(npc), C.byref(st)) == 0
    assert int(d_so.cpu()[0]) == 0 and nf.value == npc.value == 0
    one = F.Craft(21, [33], 2).build()
    assert both(m, one, "one unitig")[5]["n_head"] == 1
    two = F.Craft(21, [21, 40], 2)
    two.scaffold([1, 2], [None])
    assert both(m, two.build(), "no list")[5] == dict(dict.fromkeys(F.STAT_FIELDS, 0), n_head=1, n_n=1, n_no_entry=1)
    for via in "FM":                                              # n_plinks = 1
        c = F.Craft(21, [30, 21, 50], 5)
        c.scaffold([0, 5], [dict(via=via, path=[3])])
        assert both(m, c.build(), f"one entry through {via}")[5]["n_path"] == 1


# ---- the geometry of the emit
@pytest.mark.parametrize("lead", range(16))
def test_every_destination_alignment(model, lead):
    both(model, F.alignments(lead), f"lead {lead}")


def test_piece_tiles(model):
    """more than a tile of one-byte pieces (4160 pieces of one byte over 260 links), pieces that straddle the 4096-byte piece tile,
    a piece longer than two tiles, forward and reverse"""
    exp = both(model, F.tile_of_small_pieces(), "a tile of one-byte pieces")
    assert len(exp[4]) == 4160 and exp[5]["n_filled"] == 4160
    exp = both(model, F.long_pieces(), "long pieces")
    assert exp[5]["n_filled"] > 5 * 4096


@pytest.mark.parametrize("nu", (255, 256, 257))
def test_steps_and_entries_at_the_block_edges(model, nu):
    c = F.chain(nu)
    both(model, c, f"{nu} steps")
    for n in (255, 256, 257):
        both(model, F.padded(c, n), f"{nu} steps, {n} entries")


# ---- capacities
def test_capacities(model):
    """seq_capacity exact and one short (KMX_E_RANGE, everything else complete, nothing written to fseq, bands intact), the sizing
    call, piece_capacity one short (everything else, fseq included, complete), pieces = NULL"""
    m = model
    c = F.mixed()
    exp = expected(c)
    arrays = F.craft_arrays(c)
    nu, ns, k = len(c["strs"]), len(c["srecs"]), c["k"]
    need, need_pc = len(exp[0]), len(exp[4])
    rc, nf, npc, st, out = raw_dev(m, k, arrays, need, need_pc)
    assert rc == 0 and bands_intact(out, need, need_pc, nu, ns)
    same(parts_of(out, nf, npc, nu, ns, st), exp, "exact capacities")
    for sizing in (False, True):
        cap = 0 if sizing else need - 1
        rc, nf, npc, st, out = raw_dev(m, k, arrays, cap, need_pc, sizing=sizing)
        assert rc == -5 and (nf, npc) == (need, need_pc) and bands_intact(out, cap, need_pc, nu, ns) and np.all(out[0] == 0xA5)
        got = parts_of(out, 0, npc, nu, ns, st)
        for a, b, part in list(zip(got[:5], exp[:5], PARTS))[1:]:
            assert a.tobytes() == b.tobytes(), f"bases short: {part} differ"
        assert st == exp[5]
    rc, nf, npc, st, out = raw_dev(m, k, arrays, need, need_pc - 1)
    assert rc == -5 and (nf, npc) == (need, need_pc) and bands_intact(out, need, need_pc - 1, nu, ns)
    got = parts_of(out, nf, need_pc - 1, nu, ns, st)
    assert got[4].tobytes() == exp[4][:-1].tobytes()
    same(got[:4] + (exp[4], st), exp, "pieces short")
    rc, nf, npc, st, out = raw_dev(m, k, arrays, need, 8, no_pieces=True)
    assert rc == 0 and (nf, npc) == (need, need_pc) and np.all(out[4] == -7)
    same(parts_of(out, nf, 0, nu, ns, st)[:4] + (exp[4], st), exp, "no piece list")
    # the host form
    for cap in (need - 1, 0):
        with pytest.raises(KmxError) as e:
            run_host(m, c, capacity=cap)
        assert e.value.code == -5 and e.value.needed == need and e.value.needed_pieces == need_pc
        foffs, frec, fst, pcs, stt = e.value.result
        assert foffs.tobytes() == exp[1].tobytes() and frec.tobytes() == exp[2].tobytes() and fst.tobytes() == exp[3].tobytes() and pcs.tobytes() == exp[4].tobytes() and stt == exp[5]
    with pytest.raises(KmxError) as e:
        run_host(m, c, piece_capacity=need_pc - 1)
    assert e.value.code == -5 and e.value.needed_pieces == need_pc and e.value.result[3].tobytes() == exp[4][:-1].tobytes()
    same(run_host(m, c, capacity=need, piece_capacity=need_pc), exp, "exact capacities: host")
    got = run_host(m, c, pieces=False)
    assert got[4] is None and got[0].tobytes() == exp[0].tobytes() and got[5] == exp[5]


# ---- refusals
def test_refusals(model):
    """KMX_E_ARG before anything runs: an even or out-of-range k, U >= 2^31, n_plinks >= 2^31, S > U, kinds > 3, reserved != 0, a NULL
    required buffer, an output that overlaps another buffer; in the host form also bad uoffsets, a unitig shorter than k, a list that
    is not strictly ascending and scaffolds whose steps are not the U steps; the handle then answers as if nothing had happened"""
    m = model
    c = F.mixed()
    exp = expected(c)
    k = c["k"]
    ubuf, uoffs, srec, steps, pl, precs, pst = F.craft_arrays(c)
    nu, ns, nb = len(c["strs"]), len(c["srecs"]), len(ubuf)
    cap, pcap = len(exp[0]) + 8, len(exp[4]) + 8
    fseq, foffs, frec, fst, pcs = np.zeros(cap, np.uint8), np.zeros(ns + 1, np.uint64), np.zeros(ns, F.SCAFFOLD_FILL_DTYPE), np.zeros(nu, F.FILL_STEP_DTYPE), np.zeros(pcap, np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def host_rc(kk=k, b=ubuf, o=uoffs, n=nu, sr=srec, s=ns, stp=steps, lst=pl, n_pl=None, pr=precs, ps=pst, par=(3, 0), fs=fseq, cp=cap, fo=foffs, fr=frec, ft=fst, pc=pcs, counts=True, stats=True):
        p, st, nf, npc = FillParams(*par) if par else None, FillStats(), C.c_uint64(0), C.c_uint64(0)
        return m.L.kmx_unitig_scaffold_fill(m.h, kk, ptr(b), ptr(o), n, ptr(sr), s, ptr(stp), ptr(lst), len(pl) if n_pl is None else n_pl, ptr(pr), ptr(ps), len(pst), C.byref(p) if par else None,
                                            ptr(fs), cp, ptr(fo), ptr(fr), ptr(ft), ptr(pc), pcap, C.byref(nf) if counts else None, C.byref(npc) if counts else None, C.byref(st) if stats else None)

    d = {name: to_dev(a if a.dtype != np.uint64 else a.view(np.int64)) for name, a in (("buf", ubuf), ("off", uoffs), ("srec", srec.view(np.uint8)), ("steps", steps.view(np.uint8)),
                                                                                          ("pl", pl.view(np.uint8)), ("precs", precs.view(np.uint8)), ("pst", pst.view(np.int32)), ("fseq", fseq), ("foffs", foffs),
                                                                                          ("frec", frec.view(np.uint8)), ("fst", fst.view(np.uint8)), ("pcs", pcs.view(np.int32)))}

    def dev_rc(kk=k, n=nu, s=ns, n_pl=len(pl), par=(3, 0), cp=cap, **swap):
        t = dict(d, **swap)
        g = lambda name: t[name].data_ptr() if t[name] is not None else None
        p, st, nf, npc = FillParams(*par), FillStats(), C.c_uint64(0), C.c_uint64(0)
        return m.L.kmx_unitig_scaffold_fill_dev(m.h, kk, g("buf"), g("off"), n, nb, g("srec"), s, g("steps"), g("pl"), n_pl, g("precs"), g("pst"), len(pst), C.byref(p), g("fseq"), cp, g("foffs"), g("frec"),
                                                g("fst"), g("pcs"), pcap, C.byref(nf), C.byref(npc), C.byref(st))

    assert host_rc() == 0 and dev_rc() == 0
    for kk in (20, 3, 65):
        assert host_rc(kk=kk) == -1 and dev_rc(kk=kk) == -1
    assert dev_rc(n=2 ** 31) == -1 and dev_rc(n_pl=2 ** 31) == -1 and host_rc(n_pl=2 ** 31) == -1 and dev_rc(s=nu + 1) == -1 and host_rc(s=nu + 1) == -1
    for par in ((4, 0), (3, 1)):
        assert host_rc(par=par) == -1 and dev_rc(par=par) == -1
    assert host_rc(par=None) == -1 and host_rc(counts=False) == -1 and host_rc(stats=False) == -1
    for name in ("b", "o", "sr", "stp", "lst", "pr", "ps", "fs", "fo", "fr", "ft"):
        assert host_rc(**{name: None}) == -1, name
    for name in ("buf", "off", "srec", "steps", "pl", "precs", "pst", "fseq", "foffs", "frec", "fst"):
        assert dev_rc(**{name: None}) == -1, name
    assert host_rc(fs=ubuf, cp=nb) == -1 and host_rc(fo=uoffs) == -1 and host_rc(ft=fseq[:nu * 32].view(F.FILL_STEP_DTYPE)) == -1 and host_rc(pc=pst) == -1      # overlaps
    assert dev_rc(fseq=d["buf"], cp=nb) == -1 and dev_rc(pcs=d["pst"]) == -1
    swapped, above, short = uoffs.copy(), uoffs.copy(), uoffs.copy()
    swapped[3], swapped[4] = uoffs[4] + 1, uoffs[3]
    above[0] = 1
    short[1:] -= np.uint64(1)                                     # unitig 0 has k - 1 bytes
    for bad in (swapped, above, short):
        assert host_rc(o=bad) == -1
    dup, desc = pl.copy(), pl.copy()
    dup[3] = dup[2]
    desc[[2, 3]] = desc[[3, 2]]
    assert host_rc(lst=dup) == -1 and host_rc(lst=desc) == -1
    beyond, hole, none = srec.copy(), srec.copy(), srec.copy()
    beyond["first_step"][ns - 1] = nu                             # first_step + n_steps > U
    hole["first_step"][1] += 1
    none["n_steps"][ns - 1] = 0
    for bad in (beyond, hole, none):
        assert host_rc(sr=bad) == -1
    same(run_host(m, c), exp, "after the refusals: host")
    same(run_dev(m, c), exp, "after the refusals: device")


# ---- crafted device input between guard bands
def test_crafted_device_input_stays_inside_the_buffers(model):
    """the _dev form clamps: offsets that decrease, lie beyond n_ubases or are all ones, a list that is not ascending, scaffolds whose
    first_step lies beyond U, steps and pieces that are no unitig, records that point beyond psteps: wrong strings, KMX_OK or
    KMX_E_RANGE, and the guard bands around the five outputs are intact"""
    m = model
    c = F.mixed()
    exp = expected(c)
    k = c["k"]
    arrays = F.craft_arrays(c)
    ubuf, uoffs, srec, steps, pl, precs, pst = arrays
    nu, ns, nb = len(c["strs"]), len(c["srecs"]), len(ubuf)
    cap, pcap = len(exp[0]) + 500, len(exp[4]) + 40
    big = np.uint64(2 ** 64 - 1)
    bad = []
    for o in (uoffs[::-1].copy(), uoffs + np.uint64(nb), np.full(len(uoffs), big), np.zeros(len(uoffs), np.uint64), np.where(np.arange(len(uoffs)) % 2 == 1, big, uoffs), uoffs * np.uint64(3)):
        bad.append((ubuf, o, srec, steps, pl, precs, pst))
    bad.append((ubuf, uoffs, srec, steps, pl[::-1].copy(), precs, pst))                      # a list that is not ascending
    x = srec.copy()
    x["first_step"] = np.where(np.arange(ns) % 2 == 0, nu + 5, x["first_step"])
    bad.append((ubuf, uoffs, x, steps, pl, precs, pst))                                      # first_step beyond U
    x = srec.copy()
    x["first_step"] = 0xFFFFFFFF
    bad.append((ubuf, uoffs, x, steps, pl, precs, pst))
    x = steps.copy()
    x["o"] = np.where(np.arange(nu) % 3 == 0, 2 * nu + 7, x["o"])
    x["n_gap"] = np.where(np.arange(nu) % 5 == 0, 0xFFFFFFFF, x["n_gap"])
    bad.append((ubuf, uoffs, srec, x, pl, precs, pst))                                       # steps that are no unitig, huge gaps
    bad.append((ubuf, uoffs, srec, steps, pl, precs, np.where(np.arange(len(pst)) % 2 == 0, 0xFFFFFFFF, pst).astype(np.uint32)))
    x = precs.copy()
    x["first_step"] = np.where(np.arange(len(x)) % 2 == 0, big - np.uint64(3), x["first_step"])
    x["n_steps"] = np.where(np.arange(len(x)) % 3 == 0, 0xFFFFFFFF, x["n_steps"])
    bad.append((ubuf, uoffs, srec, steps, pl, x, pst))
    for i, arr in enumerate(bad):
        rc, nf, npc, st, out = raw_dev(m, k, arr, cap, pcap)
        assert rc in (0, -5) and bands_intact(out, cap, pcap, nu, ns), i
        assert nf <= cap or np.all(out[0] == 0xA5), i
        assert st["n_head"] + st["n_path"] + st["n_adjacent"] + st["n_n"] == nu, i
    rc, nf, npc, st, out = raw_dev(m, k, arrays, cap, pcap, n_psteps=len(pst) - 3)                 # a shorter count reads a shorter list: the last path is refused
    assert rc == 0 and bands_intact(out, cap, pcap, nu, ns) and st["n_path"] == exp[5]["n_path"] - 1
    same(run_dev(m, c), exp, "after the crafted input")


# ---- determinism
def test_two_runs_give_identical_bytes(model):
    for c in (F.mixed(), F.tile_of_small_pieces()):
        a, b, h = run_dev(model, c), run_dev(model, c), run_host(model, c)
        same(b, a, "two runs")
        same(h, a, "host and device form")
    model.set_profile(1)
    run_dev(model, F.mixed())
    ph = model.unitig_scaffold_fill_phases()
    model.set_profile(0)
    assert set(ph) == {"kinds", "scan", "records", "bytes"} and all(v > 0 for v in ph.values())


# ---- allocation failures
def test_allocation_failure_leaves_the_handle_usable(monkeypatch):
    """KMX_E_NOMEM at every allocation of a first fill call in turn, host and device form: the same call then succeeds with the
    right bytes"""
    c = F.alignments(3)
    exp = expected(c)
    failed = {"host": 0, "dev": 0}
    run = {"host": run_host, "dev": run_dev}
    for nth in range(1, 22):
        for variant in ("host", "dev"):
            m = KModel(1, 1023, NH, NB)                          # fresh: every buffer is still to be allocated
            monkeypatch.setenv("KMX_FAIL_ALLOC", str(nth))
            try:
                run[variant](m, c, capacity=len(exp[0])) if variant == "host" else run[variant](m, c)
            except KmxError as e:
                assert e.code == -6, (nth, variant, e)
                failed[variant] += 1
            monkeypatch.delenv("KMX_FAIL_ALLOC")
            same(run[variant](m, c), exp, f"after allocation {nth} failed, {variant}")
    assert failed["host"] >= 15 and failed["dev"] >= 7, failed    # 12 staged buffers; the scan's two arrays, ubase, the counters, three piece arrays


# ---- the facade and the driver
def test_facade_and_driver(tmp_path):
    """tests/facade_unitig_scaffold_fill.cpp prints the stats and the two texts for the acceptance reads; the driver's -u1 -M -W -P400
    -S6 -F writes scaffolds.filled.fa and scaffolds.fill.tsv equal to the restatement's text and leaves scaffolds.fa and every other
    output as it is without -F"""
    import count_reads as CR
    a = F.acceptance()
    k, strs, plinks, reads = a["k"], a["strs"], a["plinks"], a["reads"]
    fa = str(tmp_path / "reads.fa")
    CR.write_fasta(fa, [r.encode() for r in reads])
    lines = str(tmp_path / "reads.txt")
    with open(lines, "w") as f:
        f.write("".join(r + "\n" for r in reads))

    def build(source, exe_name):
        exe = str(tmp_path / exe_name)
        subprocess.check_call(["g++", "-O3", "-m64", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                               "-L" + os.path.join(ROOT, "kmcex_amd"), "-lkmx", "-Wl,-rpath," + os.path.join(ROOT, "kmcex_amd"), "-o", exe])
        return exe

    q = a["par"]
    scf, pth, res = F.through_restatements(k, strs, a["rows"], plinks, q, a["path_par"])
    exe = build("tests/facade_unitig_scaffold_fill.cpp", "facade_unitig_scaffold_fill")
    out = subprocess.check_output([exe, fa, str(k), "1", lines, str(P.MAX_DIST), str(q["min_pairs"]), str(q["inner"]), str(q["min_n"]), str(q["max_n"]), str(k), "3"], timeout=120).decode()
    blocks = out.split("#\n")
    assert len(blocks) == 3 and blocks[0] == " ".join(str(res["stats"][f]) for f in F.STAT_FIELDS) + "\n"
    assert blocks[1] == F.fasta(res, F.srecs_of(scf)) and blocks[2] == F.fill_tsv(res, F.srecs_of(scf))
    # the driver: inner is the floor of the mean d of the pairs on one unitig (221 for every one), min_n = 10, max_n = 2 max_dist, tol = k
    par = dict(min_pairs=6, ratio=0, inner=221, min_n=10, max_n=2 * P.MAX_DIST)
    scf, pth, res = F.through_restatements(k, strs, a["rows"], plinks, par, dict(min_pairs=6, inner=221, tol=k, max_steps=8, max_visits=4096))
    exe = build("examples/kmcex_main.cpp", "kmcEx")
    base = ["-g", "-u1", "-M", "-W", f"-P{P.MAX_DIST}", f"-k{k}", "-nh3", "-nb2", "-S6"]
    texts = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix in (".fa", ".tsv", ".gaf", ".gfa", ".agp")}
    work = tmp_path / "plain"
    work.mkdir()
    subprocess.check_call([exe, *base, fa, "db", str(work)], stdout=subprocess.DEVNULL, timeout=120)
    before = texts(work / "db")
    assert before["scaffolds.fa"].decode() == S.fasta(scf) and "scaffolds.filled.fa" not in before
    for flag, kinds in (("-F", 3), ("-F0", 0)):
        work = tmp_path / f"fill{kinds}"
        work.mkdir()
        log = subprocess.check_output([exe, *base, flag, fa, "db", str(work)], timeout=120).decode()
        after = texts(work / "db")
        want = F.through_restatements(k, strs, a["rows"], plinks, par, dict(min_pairs=6, inner=221, tol=k, max_steps=8, max_visits=4096), kinds)[2]
        assert after["scaffolds.filled.fa"].decode() == F.fasta(want, F.srecs_of(scf)) and after["scaffolds.fill.tsv"].decode() == F.fill_tsv(want, F.srecs_of(scf)), flag
        assert {n: b for n, b in after.items() if n not in ("scaffolds.filled.fa", "scaffolds.fill.tsv")} == before, flag      # every existing output byte for byte
        assert f"{want['stats']['n_path']} links filled along a path" in log and f"{want['stats']['n_removed']} N removed" in log
    assert after["scaffolds.filled.fa"].decode() == S.fasta(scf).replace(" circular=", " n_fill_bases=0 circular=")             # -F0: the scaffolds as they were
    assert subprocess.call([exe, "-g", "-u1", "-M", "-W", f"-P{P.MAX_DIST}", f"-k{k}", "-F", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2    # -F without -S
    assert subprocess.call([exe, *base, "-F4", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2 and subprocess.call([exe, *base, "-Fx", fa, "db", str(tmp_path)], stdout=subprocess.DEVNULL) == 2
