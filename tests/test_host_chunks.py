"""tests/host_chunks.py against the sources it restates (the slots, the staging
budgets and the small-group rule, read out of the two files), and every batch
of the host-pointer GPU tests against the edge it is built for."""
import os
import re

import numpy as np
import pytest

import host_chunks as HC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libquic_amd",
                    "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def body(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


def test_constants_are_the_sources():
    capi, header = source("qfec_capi.cpp"), source("qfec_internal.h")
    slots = re.findall(r"constexpr\s+int\s+kSlots\s*=\s*(\d+)\s*;", capi)
    stage = re.findall(r"constexpr\s+size_t\s+kStageBytes\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", capi)
    small = re.findall(r"constexpr\s+uint64_t\s+kRaggedSmallGroupBytes\s*=\s*(\d+)\s*;", header)
    assert [int(x) for x in slots] == [HC.SLOTS], slots
    assert [int(a) << int(b) for a, b in stage] == [HC.STAGE], stage
    assert [int(x) for x in small] == [HC.SMALL_GROUP_BYTES], small
    # the slots' buffers: input kStageBytes, aux / 8, output / 4, device and pinned alike
    alloc = body(capi, "int ensure_staging(", "ctx->staging_ready = true")
    sizes = re.findall(r"hip(?:Host)?Malloc\(&s\.([dh])_(in|aux|out),\s*kStageBytes(?:\s*/\s*(\d+))?"
                       r"\s*[,)]", alloc)
    assert sorted(sizes) == sorted((m, b, d) for m in "dh"
                                   for b, d in (("in", ""), ("aux", "8"), ("out", "4"))), sizes
    assert HC.OUT_STAGE == HC.STAGE // 4 and HC.AUX_STAGE == HC.STAGE // 8
    # the ragged planner's two budgets and its cut
    ragged = body(capi, "int ragged_host(", "int ragged_mapped(")
    assert re.search(r"in_cap\s*=\s*kStageBytes\s*,\s*out_cap\s*=\s*kStageBytes\s*/\s*4\s*;", ragged)
    assert re.search(r"if\s*\(c\.n\s*>\s*0\s*&&\s*\(lay\.in_total\s*>\s*in_cap\s*\|\|\s*"
                     r"lay\.out_total\s*>\s*out_cap\)\)\s*break;", ragged)
    assert re.search(r"c\.nbytes\s*<\s*qfec::kRaggedSmallGroupBytes\s*\*\s*c\.n", ragged)
    assert re.search(r"slot\s*=\s*\(slot\s*\+\s*1\)\s*%\s*kSlots;", ragged)
    # the fixed planner's three
    fixed = body(capi, "int fixed_host(", "struct Pending")
    assert re.search(r"cg\s*=\s*kStageBytes\s*/\s*group_stride;", fixed)
    assert re.search(r"min<uint64_t>\(cg,\s*\(kStageBytes\s*/\s*4\)\s*/\s*L\);", fixed)
    assert re.search(r"if\s*\(recover\)\s*cg\s*=\s*std::min<uint64_t>\(cg,\s*\(kStageBytes\s*/\s*8\)"
                     r"\s*/\s*\(L\s*\+\s*1\)\);", fixed)
    assert re.search(r'if\s*\(cg\s*==\s*0\)\s*return\s+fail\([^;]*"staging too small"\);', fixed)


def test_layout_is_the_source():
    """RaggedLayout, line by line, against ragged_totals"""
    lay = re.sub(r"\s+", " ", body(source("qfec_capi.cpp"), "struct RaggedLayout {", "};"))
    for line in ["off = align_up(c.nbytes, 16);", "len = off + c.np * 8;",
                 "ptr = align_up(len + c.np * 2, 8);", "poff = align_up(ptr + (c.n + 1) * 4, 8);",
                 "par = align_up(poff + c.n * 8, 16);",
                 "plen = align_up(par + (recover ? c.npar : 0), 8);",
                 "miss = plen + (recover ? c.n * 2 : 0);",
                 "ooff = align_up(miss + (recover ? c.n : 0), 8);",
                 "in_total = ooff + (recover ? c.n * 8 : 0);", "out_plen = align_up(c.nout, 8);",
                 "out_total = out_plen + (recover ? 0 : c.n * 2);"]:
        assert line in lay, line
    # by hand, encode: 3 groups, 7 packets, 100 B staged, 40 B of parity
    # 112 | +56 = 168 | +14 -> 184 | +16 = 200 | +24 -> 224 = par = plen = miss = ooff
    assert HC.ragged_totals(3, 7, 100, 40, 0, False) == (224, 46)
    # recover: 6 entries, 90 B staged, 40 B of redundancy behind the tables
    # 96 | +48 = 144 | +12 -> 160 | +16 = 176 | +24 -> 208 | +40 = 248 | +6 = 254 -> +3 -> 264 | +24
    assert HC.ragged_totals(3, 6, 90, 40, 40, True) == (288, 40)


def test_planner_cuts_before_the_group_that_exceeds():
    # 50,000 groups of one full packet: the output budget (1,452 + 2 B a group) cuts
    n = 50_000
    ln = np.full(n, 1452, np.uint16)
    ptr = np.arange(n + 1, dtype=np.uint32)
    plan = HC.plan_ragged(ln, ptr)
    per = HC.OUT_STAGE // 1454
    assert [c["n"] for c in plan] == [per] * (n // per) + [n % per]
    assert [c["cut"] for c in plan] == ["out"] * (n // per) + ["end"]
    assert [c["g0"] for c in plan] == [i * per for i in range(len(plan))]
    for c in plan:
        it, ot = HC.ragged_totals(c["n"], c["npk"], c["nbytes"], c["nout"], c["npar"], False)
        assert it <= HC.STAGE and ot <= HC.OUT_STAGE
    assert HC.ragged_totals(per + 1, per + 1, (per + 1) * 1452, (per + 1) * 1452, 0, False)[1] \
        > HC.OUT_STAGE
    # tables of a sub-batch: the plan of groups 10.. is the plan of those groups alone
    assert HC.plan_ragged(ln, ptr[10:]) == HC.plan_ragged(ln[10:], ptr[:-10])


@pytest.fixture(scope="module", params=sorted(HC.LARGE))
def large(request):
    b = HC.large(request.param)
    return b, HC.plans(b)


def test_large_batches_byte_bounds(large):
    """what the GPU tests rest on, whatever the planner does: more bytes in and
    more bytes out than SLOTS slots hold, on the encode and on the recover"""
    b, _ = large
    for recover in (False, True):
        nin, nout = HC.staged_bytes(b, recover)
        assert nin > HC.SLOTS * HC.STAGE, (recover, nin)
        assert nout > HC.SLOTS * HC.OUT_STAGE, (recover, nout)
    assert b["pkt_len"].min() >= 1 and b["pkt_len"].max() <= HC.MAX_PACKET
    assert int(b["pkt_off"].max()) + HC.MAX_PACKET <= b["data"].size
    assert (b["missing"] < b["ks"]).all()
    # the lost packets' offsets are far outside the arena, the others untouched
    off = HC.recover_offsets(b)
    lost = b["grp_ptr"][:-1].astype(np.int64) + b["missing"]
    assert (off[lost] == HC.FAR_OFF).all() and HC.FAR_OFF > 1000 * b["data"].size
    keep = np.ones(off.size, bool)
    keep[lost] = False
    assert np.array_equal(off[keep], b["pkt_off"][keep])
    # the slots are a permutation from an odd base, not in group order
    poff, size = HC.slot_offsets(b["ks"].size, 3)
    assert np.array_equal(np.sort(poff), np.arange(b["ks"].size, dtype=np.uint64) * 1460 + 5)
    assert size == b["ks"].size * 1460 + 5 and (np.diff(poff.astype(np.int64)) != 1460).any()


def test_large_batches_modelled_plan(large):
    """which edge is which, in the modelled plan of the encode and of the recover"""
    b, plans = large
    for recover, plan in zip((False, True), plans):
        assert len(plan) > HC.SLOTS
        assert sum(c["n"] for c in plan) == b["ks"].size
        cuts = [c["cut"] for c in plan]
        assert "in" in cuts and "out" in cuts and cuts[-1] == "end", cuts
        small = [c["small"] for c in plan]
        assert True in small and False in small, small
        # a boundary inside a run of equal-shaped groups: same stretch, same k on both sides
        inside = [c["g0"] for c in plan[1:]
                  if b["stretch"][c["g0"] - 1] == b["stretch"][c["g0"]]
                  and b["ks"][c["g0"] - 1] == b["ks"][c["g0"]]]
        assert inside, [c["g0"] for c in plan]
        # every slot is gathered again, over a chunk that held other stretches
        for i in range(HC.SLOTS):
            held = [frozenset(b["stretch"][c["g0"]:c["g0"] + c["n"]].tolist())
                    for c in plan[i::HC.SLOTS]]
            assert len(held) > 1 and len(set(held)) > 1, (i, held)


def test_large_batches_chunk_counts():
    """seven chunks each: forward three of about 3,225 groups (3,213 on the
    recover) cut by the input budget, three of about 11,577 (11,593) cut by the
    output budget, then the rest; in reverse the tiny groups share the first
    output-budget chunk and the last chunk is what is left of the k = 15 groups"""
    for name, cuts in (("forward", ["in"] * 3 + ["out"] * 3 + ["end"]),
                       ("reverse", ["out"] * 3 + ["in"] * 3 + ["end"])):
        for plan in HC.plans(HC.large(name)):
            assert [c["cut"] for c in plan] == cuts, (name, plan)
    for plan, per_in, per_out in zip(HC.plans(HC.large("forward")), (3_225, 3_213), (11_577, 11_593)):
        assert all(abs(c["n"] - per_in) < 10 for c in plan[:3]), plan
        assert all(abs(c["n"] - per_out) < 10 for c in plan[3:6]), plan


@pytest.mark.parametrize("name", sorted(HC.FIXED_MULTI))
def test_fixed_shapes_pass_the_rotation(name):
    s = HC.fixed_multi(name)
    cg = s["cg"]
    assert cg > 0 and -(-s["n"] // cg) > HC.SLOTS and s["n"] % cg != 0
    assert cg == (5_773 if s["recover"] else 11_554)
    # strides above L everywhere, the free stride not a multiple of the rows'
    assert s["row_stride"] > s["L"] and s["parity_stride"] > s["L"] and s["out_stride"] > s["L"]
    assert (s["group_stride"] == s["k"] * s["row_stride"]) == s["way"].endswith("uniform")
    # pinned memory of one test near or below 128 MB
    if s["way"].startswith("pinned"):
        pinned = s["n"] * (s["group_stride"] + s["out_stride"]
                           + (s["parity_stride"] if s["recover"] else 0))
        assert pinned <= 128 << 20, pinned


def test_fixed_chunk_groups():
    assert HC.fixed_chunk_groups(1350, 13500, False) == 4971   # test_host_pointer_path's chunks
    assert HC.fixed_chunk_groups(1350, 5 * 1408, True) > 6000  # test_host_pointer_strided: one chunk
    assert HC.fixed_chunk_groups(16, HC.STAGE + 1, False) == 0  # the refusal
    assert HC.fixed_chunk_groups(16, HC.STAGE, False) == 1
