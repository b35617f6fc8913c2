"""The inputs of tests/test_gpu_read_phases.py, checked without a device: what keeps a case from passing for the wrong reason.  The
tiles of the count batches start the numbers of reads they are named after, every slot of a phase holds an odd read among kept and
among dropped neighbours, the oracle keeps the reads the batch means it to keep -- about half of them -- and refuses the error
batches with the intended code at the intended read."""
import numpy as np
import pytest

from midas_amd import abi
from oracle import c_oracle
from tests import helpers as H
from tests import test_gpu_read_phases as P

DEFAULT = abi.Thresholds.from_args(abi.DEFAULT_ARGS)


def test_the_slot_rule_is_a_bijection_for_every_lane_count():
    for lanes in range(1, 11):
        rpw, ph = 64 // lanes, P.phase_iters(lanes)
        assert ph * rpw <= 64 and (ph % 2 == 0 or ph == 1) and (ph == 4 or (ph + 2) * rpw > 64 or lanes == 1)
        n = 3 * ph * rpw * P.NWAVES
        seen = set()
        for v in range(n):
            (p, w), slot = P.slot_of(v, lanes)
            assert 0 <= slot < ph * rpw and P.stream_index(p, w, slot, lanes) == v
            seen.add((p, w, slot))
        assert len(seen) == n
    assert [P.phase_iters(k) for k in (1, 2, 3, 4, 5, 8, 9)] == [1, 2, 2, 4, 4, 4, 4]


@pytest.mark.parametrize("read_len", P.LENGTHS)
def test_count_batches_start_the_named_numbers_of_reads(read_len):
    table, soa, reads, starts = P.count_batch(read_len)
    assert [tuple(s) for s in starts] == [tuple(n + (1 if (c, t) == P.OUTLIER_TILE else 0) for t, n in enumerate(tiles))
                                          for c, tiles in enumerate(P.COUNT_TILES)]
    flat = [n for s in starts for n in s]
    assert set(P.PHASE_COUNTS) <= set(flat)
    pairs = set(zip(flat, flat[1:]))
    assert (0, 513) in pairs and (513, 1) in pairs and (577, 0) in pairs
    n_tiles = len(flat)
    assert n_tiles // 8 >= 1 and all(1 <= (len(t) + 3) // 4 <= 4 for t in P.COUNT_TILES)      # one-by-one tail items; 1-3 chunks
    overhang = H.direct_overhang_shape(read_len)[0]
    assert min(P.COUNT_LAST) < overhang
    assert max(len(r["seq"]) for r in reads) == read_len == min(len(r["seq"]) for r in reads)
    spans = [H.cigar_span(r["cigar"]) for r in reads]
    assert sum(1 for s in spans if s > overhang) == 1 and sorted(spans)[-2] <= overhang      # the outlier, and only it
    for k in range(len(table.length)):
        lo, hi = int(table.read_begin[k]), int(table.read_begin[k + 1])
        assert all(reads[i]["pos"] <= reads[i + 1]["pos"] for i in range(lo, hi - 1))
        assert any(reads[i]["pos"] % P.CHUNK > P.CHUNK - read_len for i in range(lo, hi))       # a read over a chunk border
    for args in ({}, P.OTHER_THRESHOLDS):
        st, er, oc, _, os_ = c_oracle.pileup(abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, **args)), table, soa)
        assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
        aligned, mapped = int(os_[:, 0].sum()), int(os_[:, 1].sum())
        assert aligned == len(reads) and 0.25 * aligned <= mapped <= 0.75 * aligned, (aligned, mapped)
        assert int(oc.sum()) > 0


@pytest.mark.parametrize("kind,read_len", [(k, 150) for k in P.SLOT_KINDS] + [(k, l) for l in (114, 152) for k in ("mapq", "del", "five_op")])
def test_slot_batches_put_an_odd_read_into_every_slot(kind, read_len):
    table, soa, reads, seen = P.slot_batch(kind, read_len)
    lanes = H.direct_lane_shape(read_len)[1]
    slots = P.phase_iters(lanes) * (64 // lanes)
    # every slot holds an odd read among kept and among dropped neighbours; for the kinds that drop a read, both a dropped and a kept one
    want = {(False, True), (True, False)} if kind in P.DROP_KINDS else {(True, True), (True, False)}
    assert sorted(seen) == list(range(slots)) and all(s == want for s in seen.values())
    kept = [r for r in reads if r["kept"]]
    assert 0.25 * len(reads) <= len(kept) <= 0.75 * len(reads)
    n_odd = sum(1 for r in reads if r["kind"] == kind)
    assert n_odd == (slots if kind in P.DROP_KINDS else 2 * slots)
    # no read reaches the next tile: a tile's stream is the reads that start in it, in order
    assert all(r["pos"] % P.TILE + H.cigar_span(r["cigar"]) < P.TILE for r in reads)
    for k in range(len(table.length)):
        lo, hi = int(table.read_begin[k]), int(table.read_begin[k + 1])
        assert all(reads[i]["pos"] <= reads[i + 1]["pos"] for i in range(lo, hi - 1))
    st, er, oc, _, os_ = c_oracle.pileup(DEFAULT, table, soa)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    assert int(os_[:, 0].sum()) == len(reads) and int(os_[:, 1].sum()) == len(kept)      # the oracle keeps exactly the reads meant to be kept
    # ... and tallies what they hold: every A/C/G/T base of a kept read at or above the threshold, less inserted and clipped ones
    assert int(oc.sum()) > 0
    for baseq in (0, 30):
        st, er, oc, _, _ = c_oracle.pileup(abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq)), table, soa)
        assert st == 0
        want_bases = 0
        for r in kept:
            q, at = np.asarray(r["qual"]), 0
            for op, n in r["cigar"]:
                if op in (0, 7, 8):
                    want_bases += int((q[at:at + n] >= baseq).sum())
                if op in (0, 1, 4, 7, 8):
                    at += n
        assert int(oc.sum()) == want_bases


@pytest.mark.parametrize("where", P.ERROR_SLOTS)
@pytest.mark.parametrize("kind", sorted(P.ERROR_CODES))
def test_error_batches_are_refused_with_the_intended_code(kind, where):
    table, soa, reads = P.error_batch((kind,), (where,))
    assert len(reads) == 601 and all(0 <= r["pos"] < P.TILE for r in reads)
    st, er, *_ = c_oracle.pileup(DEFAULT, table, soa)
    assert (st, er) == (P.ERROR_CODES[kind], where)


def test_two_refused_reads_share_a_phase_and_the_lower_index_is_reported():
    for kinds, where in ((("no_qual", "no_nm"), (3, 70)), (("overrun", "no_nm"), (16 * 4 + 2, 16 * 8 + 1)),
                         (("no_nm", "no_qual"), (257, 256 + 16 * 12)), (("no_qual", "overrun"), (599, 600))):
        assert P.slot_of(where[0], 4)[0] == P.slot_of(where[1], 4)[0]
        table, soa, _ = P.error_batch(kinds, where)
        st, er, *_ = c_oracle.pileup(DEFAULT, table, soa)
        assert (st, er) == (P.ERROR_CODES[kinds[0]], where[0])
