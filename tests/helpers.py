"""Shared test helpers: build C-ABI inputs from readable case descriptions."""
import json
import os
import re

import numpy as np

from midas_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIGAR_CHARS = "MIDNSHP=XB"
NT16 = "=ACMGRSVTWYHKDBN"


def parse_cigar(s):
    return [(CIGAR_CHARS.index(op), int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=XB])", s)]


def encode_seq4(seq):
    codes = [NT16.index(c) if c in NT16 else 15 for c in seq.upper()]
    if len(codes) & 1:
        codes.append(0)
    return [(codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2)]


def reads_from_dicts(reads):
    """[{pos,cigar(str or [(op,len)]),seq,qual(list|'absent'),nm(int|None),mapq,flag}] -> ReadsSoA"""
    pos, mapq, flag, nm, l_seq = [], [], [], [], []
    seq4, qual, cigar = [], [], []
    seq_off, qual_off, cigar_off = [0], [0], [0]
    for r in reads:
        cg = parse_cigar(r["cigar"]) if isinstance(r["cigar"], str) else r["cigar"]
        s = r["seq"]
        q = r.get("qual")
        if q is None:
            q = [40] * len(s)
        elif isinstance(q, str) and q == "absent":
            q = [0xFF] * len(s)
        assert len(q) == len(s)
        pos.append(r["pos"]); mapq.append(r.get("mapq", 42)); flag.append(r.get("flag", 0))
        nm.append(-1 if r.get("nm", 0) is None else r.get("nm", 0)); l_seq.append(len(s))
        seq4 += encode_seq4(s); qual += list(q); cigar += [(ln << 4) | op for op, ln in cg]
        seq_off.append(len(seq4)); qual_off.append(len(qual)); cigar_off.append(len(cigar))
    return abi.ReadsSoA(pos=np.array(pos, dtype=np.int32), mapq=np.array(mapq, dtype=np.uint8),
                        flag=np.array(flag, dtype=np.uint16), nm=np.array(nm, dtype=np.int32),
                        l_seq=np.array(l_seq, dtype=np.int32), seq_off=np.array(seq_off, dtype=np.int64),
                        qual_off=np.array(qual_off, dtype=np.int64), cigar_off=np.array(cigar_off, dtype=np.int64),
                        seq4=np.array(seq4, dtype=np.uint8), qual=np.array(qual, dtype=np.uint8),
                        cigar=np.array(cigar, dtype=np.uint32))


def single_contig(length, n_reads, ref=None):
    ref = np.frombuffer((ref or "A" * length).encode(), dtype=np.uint8)
    return abi.ContigTable(length=[length], species=[0], read_begin=[0, n_reads], ref=ref, n_species=1,
                           ids=["contig_1"], species_ids=["sp"])


def load_kat_cases():
    with open(os.path.join(GOLDEN, "kat_cases.json")) as f:
        return json.load(f)["cases"]


def kat_inputs(case):
    reads = reads_from_dicts(case["reads"])
    contigs = single_contig(case["contig_len"], reads.n_reads, case.get("ref"))
    args = dict(abi.DEFAULT_ARGS)
    args.update(case.get("args", {}))
    return contigs, reads, abi.Thresholds.from_args(args), args


def kat_pysam_pad_rule(case):
    """True when the case states what the path does under MIDAS_SNPS_PAD_PYSAM (the CIGAR op P advances the query)."""
    return case.get("pad_rule", "spec") == "pysam"


def kat_expected_counts(case):
    exp = np.zeros((case["contig_len"], 4), dtype=np.uint32)
    for k, v in case.get("counts", {}).items():
        exp[int(k)] = v
    return exp


def kat_expected_stats(case):
    return np.array([[case["aligned_reads"], case["mapped_reads"], case["covered_bases"], case["total_depth"]]],
                    dtype=np.int64)


# ---- the direct kernel's lane shapes (pileup_direct.hip) and batches aimed at their borders ------------------------------------
TILE = 2048
CHUNK = 4 * TILE
OVERHANG, OVERHANG_LONG = 160, 288
BORDER_QUALS = (0, 12, 29, 30, 31, 40, 41, 50, 51, 60)
SHORT_READ = 12                 # the single-lane read among the long ones


def direct_lane_shape(max_len):
    """(lane_bases, lanes_per_read) of the direct path for a batch's longest read: the rule of direct_lane_bases."""
    lanes = lambda lb: (max_len + lb - 1) // lb
    lb = 32 if lanes(32) < lanes(30) else 30
    if lb == 30 and 96 < max_len <= 160 and lanes(38) < lanes(32):
        lb = 38
    return lb, lanes(lb)


def direct_overhang_shape(max_len):
    """(direct_overhang, direct_chunk_tiles) a position-sorted batch reports for its longest read: chunks of four tiles carry the
    common overhang up to 160 bases, the long one up to 288; a longer read switches the chunks off (tile by tile, common overhang)."""
    if max_len <= OVERHANG:
        return OVERHANG, 4
    return (OVERHANG_LONG, 4) if max_len <= OVERHANG_LONG else (OVERHANG, 1)


def border_offsets(lane_bases, max_len):
    """Query offsets on both sides of every lane border inside a read of max_len bases."""
    return [k * lane_bases + d for k in range(1, (max_len - 1) // lane_bases + 1) for d in (-1, 0, 1)]


def border_contigs(overhang):
    return [2 * CHUNK + 5, TILE, 3 * TILE - 1, CHUNK + overhang, 700, 5 * TILE + overhang + 1]


def cigar_span(cigar):
    return sum(n for op, n in cigar if op in (0, 2, 3, 7, 8))


def border_reads(rng, length, lane_bases, max_len, overhang, n, turn):
    """n reads on a contig of `length` sites whose clips, insertions and deletions start or end on and around the lane borders.
    A read's "events" are the (kind, query offset) pairs it puts exactly on an offset of border_offsets: kind "clip" (the first
    aligned base, or the first base of a trailing clip), "ins" (the first inserted base, or the first base behind the
    insertion), "del" (the first base behind the deletion).  The offsets are dealt round-robin per kind of read (`turn`), and a read
    with events is built to pass the read filter at mapid 50, aln_cov 0.2, mapq 20 -- so every border offset gets tallied
    reads of every kind (border_conditions asserts it).  No read spans more than the overhang where the batch runs in chunks.  The "edge"
    reads sit on either side of the filter's two thresholds: an aligned part of ceil(l / 5) bases or one less, and l // 2 or
    l // 2 + 1 mismatches."""
    lb = lane_bases
    borders = border_offsets(lb, max_len)
    assert all(1 <= o <= max_len - 2 for o in borders), (lb, max_len)
    cap = overhang if max_len <= overhang else max_len + 8          # the longest reference span (no chunks: nothing to stay within)
    whole = [m for k in range(1, max_len // lb + 1) for m in (k * lb, k * lb + 1) if SHORT_READ < m <= max_len]
    tile_borders = list(range(TILE, length, TILE))
    chunk_borders = list(range(CHUNK, length, CHUNK))

    def offset(kind, l_max):
        """The kind's next border offset with room for two bases behind it in a read of at most l_max bases (None: no border)."""
        fit = [o for o in borders if o <= l_max - 2]
        if not fit:
            return None
        turn[kind] = turn.get(kind, 0) + 1
        return fit[turn[kind] % len(fit)]

    out = []
    for _ in range(n):
        u = rng.random()
        l = max_len if u < 0.45 else (max_len - 1 if u < 0.55 else (rng.choice(whole) if u < 0.85 and whole else rng.randint(min(SHORT_READ + 1, max_len), max_len)))
        mapq = 19 if rng.random() < 0.04 else rng.choice([42, 42, 30, 20])
        events = []
        kind = rng.random()
        if kind < 0.08:
            name, cigar = "plain", [(0, l)]
        elif kind < 0.12:                    # on either side of the read filter's thresholds (aln_cov 0.2, mapid 50): kept, dropped
            name, edge_nm = "edge", None
            if rng.random() < 0.5:
                alen = max(1, (l + 4) // 5 - rng.choice([0, 1]))
                cigar = [(4, l - alen), (0, alen)] if rng.random() < 0.5 else [(0, alen), (4, l - alen)]
            else:
                cigar, edge_nm = [(0, l)], l // 2 + rng.choice([0, 1])
        elif kind < 0.30:                    # a leading / trailing / both-sided soft clip ending on a border
            name = "clip"
            o = offset("clip", max_len)
            if o is None:
                o = l // 2
            else:
                l = max(l, o + 2)
                events.append(("clip", o))
            mode = rng.choice(["lead", "trail", "both"])
            if mode != "trail" and 4 * (l - o) < l + 4:
                mode = "trail"                                      # (a leading clip this long fails aln_cov: the trailing one)
            elif mode == "trail" and 4 * o < l + 4:
                mode = "lead"
            if mode == "lead":
                cigar = [(4, o), (0, l - o)]
            elif mode == "trail":
                cigar = [(0, o), (4, l - o)]
            else:
                o2s = [x for x in borders if o < x <= l - 2 and 4 * (x - o) >= l + 4]
                o2 = rng.choice(o2s) if o2s else l - 1
                if o2s and events:
                    events.append(("clip", o2))
                cigar = [(4, o), (0, o2 - o), (4, l - o2)] if 4 * (o2 - o) >= l + 4 else [(4, o), (0, l - o)]
        elif kind < 0.52:                    # an insertion that starts or ends on a border
            name = "ins"
            o = offset("ins", max_len)
            if o is None:
                o = l // 2
            else:
                l = max(l, o + 2)
                events.append(("ins", o))
            i = rng.randint(1, 4)
            a = o - i if rng.random() < 0.5 and o - i >= 1 else o
            i = min(i, l - 1 - a)
            cigar = [(0, a), (1, i), (0, l - a - i)]
        elif kind < 0.76:                    # a deletion at a border (the span stays within the overhang)
            name = "del"
            l = min(l, cap - 1)
            o = offset("del", cap - 1)
            if o is None:
                o = l // 2
            else:
                l = max(l, o + 2)
                events.append(("del", o))
            cigar = [(0, o), (2, rng.randint(1, cap - l)), (0, l - o)]
        elif kind < 0.84:                    # clip + indel: four ops, still settled in registers
            name = "clip+indel"
            l = min(l, cap - 3)
            o = offset("clip4", min(l - 12, (3 * l - 4) // 4 + 2)) if l > 14 else None      # (the aligned part keeps aln_cov)
            s = o if o is not None else 1
            o2s = [x for x in borders if s + 1 < x <= l - 2]
            g = rng.randint(1, 3)
            if o2s and rng.random() < 0.5:   # the gap on a border as well
                o2 = rng.choice(o2s)
                gk = rng.choice(["ins", "del"])
                a = o2 - s
                if gk == "ins":
                    g = min(g, l - 1 - o2)
                events.append((gk, o2))
            else:
                gk, a = "ins", rng.randint(1, l - s - 6)
            if o is not None:
                events.append(("clip", s))
            cigar = [(4, s), (0, a), (1 if gk == "ins" else 2, g), (0, l - s - a - (g if gk == "ins" else 0))]
        elif kind < 0.88:                    # five ops with N, = and X: walked op by op
            name = "five"
            l = min(l, cap - 3)
            o = offset("five", l - 8) if l > 10 else None
            a = o if o is not None else min(5, l - 9)
            cigar = [(0, a), (3, 3), (7, 6), (8, 2), (0, l - a - 8)]
        elif kind < 0.91:                    # a hard clip in front of the soft clip (walked op by op as well)
            name = "hard"
            o = offset("hard", max_len)
            if o is None:
                o = l // 2
            else:
                l = max(l, o + 2)
            if 4 * (l - o) < l + 4:
                cigar = [(5, rng.randint(1, 20)), (4, 1), (0, o - 1), (4, l - o), (5, rng.randint(1, 9))]
            else:
                cigar = [(5, rng.randint(1, 20)), (4, o), (0, l - o)]
            if o in borders:
                events.append(("clip", o))
        elif kind < 0.94:                    # the batch's shortest read, on a single lane among the long ones
            name, l = "short", min(SHORT_READ, max_len)
            cigar = [(0, l)] if rng.random() < 0.5 else [(4, 2), (0, l - 2)]
        else:                                # a whole number of lanes, and one base more (the last lane holds one base)
            name = "whole"
            l = rng.choice(whole[-2:]) if whole else l
            cigar = [(0, l)]
        assert sum(c for op, c in cigar if op in (0, 1, 4, 7, 8)) == l and all(c >= 1 for _, c in cigar), (name, l, cigar)
        span = cigar_span(cigar)
        assert span <= cap
        alen = sum(c for op, c in cigar if op in (0, 1, 7, 8))
        where = rng.random()
        if tile_borders and where < 0.5:     # over a tile border, a chunk border among them
            b = rng.choice(chunk_borders) if chunk_borders and rng.random() < 0.35 else rng.choice(tile_borders)
            pos = b - rng.randint(0, span + 2) + rng.choice([0, 0, 1, -1])
        elif where < 0.53:
            pos = rng.randint(-2, 0)
        elif where < 0.56:                   # hangs over the contig's end
            pos = length - rng.randint(1, span)
        else:
            pos = rng.randint(0, length - 1)
        pos = max(-2, min(length - 1, pos))
        if mapq < 20:
            events = []
        out.append(dict(pos=pos, cigar=cigar, seq="".join(rng.choices("ACGTACGTACGTN", k=l)), qual=rng.choices(BORDER_QUALS, k=l),
                        nm=min(rng.choice([0, 1, 2, 3]), alen // 2) if name != "edge" or edge_nm is None else edge_nm, mapq=mapq,
                        kind=name, events=events))
    return out


_NT16_CODE = np.full(256, 15, dtype=np.uint8)
for _k, _ch in enumerate(NT16):
    _NT16_CODE[ord(_ch)] = _k


def reads_from_border_dicts(reads):
    """reads_from_dicts for the thousands of reads of a border batch: the same arrays, built with numpy."""
    seq4, cigar = [], []
    for r in reads:
        codes = _NT16_CODE[np.frombuffer(r["seq"].encode(), np.uint8)]
        if codes.size & 1:
            codes = np.append(codes, np.uint8(0))
        seq4.append((codes[0::2] << 4) | codes[1::2])
        cigar += [(ln << 4) | op for op, ln in r["cigar"]]
    l_seq = np.array([len(r["seq"]) for r in reads], dtype=np.int32)
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    return abi.ReadsSoA(pos=np.array([r["pos"] for r in reads], dtype=np.int32), mapq=np.array([r["mapq"] for r in reads], dtype=np.uint8),
                        flag=np.zeros(len(reads), dtype=np.uint16), nm=np.array([r["nm"] for r in reads], dtype=np.int32), l_seq=l_seq,
                        seq_off=off([s.size for s in seq4]), qual_off=off(l_seq), cigar_off=off([len(r["cigar"]) for r in reads]),
                        seq4=np.concatenate(seq4).astype(np.uint8), qual=np.concatenate([np.asarray(r["qual"], dtype=np.uint8) for r in reads]),
                        cigar=np.array(cigar, dtype=np.uint32))


def border_batch(lane_bases, max_len, overhang, seed, lengths=None, extra=None):
    """-> (ContigTable, ReadsSoA, reads as dicts): border_reads on the contigs of border_contigs(overhang), position-sorted per
    contig, over a reference with lower case and N.  extra(k, n, rng): further reads for contig k of n sites."""
    import random
    assert direct_lane_shape(max_len)[0] == lane_bases, (lane_bases, max_len)
    rng = random.Random(seed)
    lengths = list(lengths or border_contigs(overhang))
    reads, begin, ref, turn = [], [0], [], {}
    for k, n in enumerate(lengths):
        rs = border_reads(rng, n, lane_bases, max_len, overhang, max(60, n // 10), turn)
        if extra:
            rs += extra(k, n, rng)
        rs.sort(key=lambda r: r["pos"])
        reads += rs
        begin.append(len(reads))
        ref.append("".join(rng.choices("ACGTacgtN", k=n)))
    assert max(len(r["seq"]) for r in reads) == max_len
    table = abi.ContigTable(length=lengths, species=[k % 2 for k in range(len(lengths))], read_begin=begin,
                            ref=np.frombuffer("".join(ref).encode(), np.uint8), n_species=2,
                            ids=["c%d" % k for k in range(len(lengths))], species_ids=["s0", "s1"])
    return table, reads_from_border_dicts(reads), reads


def border_conditions(reads, lane_bases, max_len, oracle_counts, oracle_stats):
    """What keeps a border batch from passing for the wrong reason, from the batch and the oracle's result alone (no device):
    every border offset has a clip, an insertion and a deletion exactly on it; the lengths of a whole number of lanes, of one
    base more and of the single-lane read occur; the oracle tallied something and kept at least 90 % of the reads."""
    have = set(e for r in reads for e in r["events"])
    missing = [(k, o) for o in border_offsets(lane_bases, max_len) for k in ("clip", "ins", "del") if (k, o) not in have]
    assert not missing, "no read puts its event on %s" % missing[:8]
    lens = set(len(r["seq"]) for r in reads)
    top = max_len // lane_bases * lane_bases
    assert min(lens) == min(SHORT_READ, max_len) and max(lens) == max_len
    if top > SHORT_READ:
        assert top in lens and (top + 1 in lens or top + 1 > max_len), (top, sorted(lens))
    kinds = set(r["kind"] for r in reads)
    assert kinds >= {"plain", "edge", "clip", "ins", "del", "clip+indel", "five", "hard", "short", "whole"}, kinds
    assert int(oracle_counts.sum()) > 0
    aligned, mapped = int(oracle_stats[:, 0].sum()), int(oracle_stats[:, 1].sum())
    assert aligned == len(reads) and 10 * mapped >= 9 * aligned, (aligned, mapped)


LONG_HEADER_BYTES = 276265


def long_header_bam(path):
    """A BAM whose header is longer than one BGZF block: 4 contigs with 4 000 reads, and 4 000 read-less references behind them --
    276 265 bytes of header, five blocks, so that a reader that takes twice as many blocks every round goes round four times.
    -> (names, lengths) as written."""
    from midas_amd import synth
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=4, n_reads=4000, seed=11)
    refid = np.repeat(np.arange(4, dtype=np.int32), np.diff(contigs.read_begin))
    names = list(contigs.ids) + ["empty_reference_%05d" % k for k in range(4000)]
    lens = [int(x) for x in contigs.length] + [99996 + k for k in range(4000)]
    abi.write_bam(path, names, lens, refid, reads)
    return names, lens
