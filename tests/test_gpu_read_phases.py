"""The direct kernel's per-read work (pileup_direct.hip: CIGAR shape, the filter tables, keep_read, the read counters and the
error report), held to the C oracle where a scheme that does it once per read for a PHASE of a wave's iterations -- up to 64 reads,
one lane each, handed to the lanes that hold the read's bases -- can go wrong.  Three kinds of batch:

  counts   tiles that start exactly N reads for every N at which a wave's number of iterations, and so of phases, changes
           (150-base reads: 16 reads an iteration, 4 waves), unlike neighbours side by side, a contig's last tile shorter than the
           overhang, chunk borders, one-by-one tail items and a chunk with an outlier deletion; the same tiles with reads of 114,
           152, 250, 260, 60 and 30 bases (three lanes of 38, five of 32, eight of 32 and nine of 30 with the long overhang, two
           lanes and one lane of 30: phases of two iterations and of one);
  slots    one odd read -- dropped by one of keep_read's tests, or with an indel, a clip or a walked CIGAR -- per phase, in slot
           k mod (slots of a phase) of the k-th phase, among plain neighbours: every slot gets one, in a first half among kept
           neighbours and in a second half among neighbours that mapq drops;
  errors   a read the oracle refuses in a chosen slot: status and read index are the oracle's, the lower index wins.

Every batch runs on the direct path twice, the second time with other thresholds, bit-exact against oracle/c_oracle.pileup.
tests/test_read_phases_host.py checks without a device that the batches are what they claim to be."""
import functools
import random

import numpy as np
import pytest

from midas_amd import abi
from oracle import c_oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu
TILE = H.TILE
CHUNK = H.CHUNK
NWAVES = 4                                   # waves of the kernel's workgroup
# reads that START in consecutive tiles: a wave gets 0, 1, 2, 3, 4, 5, 8 and 9 iterations of 16 reads
PHASE_COUNTS = (0, 1, 16, 17, 63, 64, 65, 128, 129, 256, 257, 272, 273, 320, 321, 512, 513, 577)
# per contig: the reads that start in each of its tiles; unlike neighbours side by side (0 then 513 then 1), every contig one to
# three chunks long, the first one's last tile 100 sites (shorter than either overhang), 29 tiles in all: the last three one by one
COUNT_TILES = (
    (0, 513, 1, 577, 16, 0, 17, 512, 63, 64, 65, 320, 7),              # 12 tiles + 100 sites
    (257, 0, 0, 129, 128, 1, 273, 272),                                 # two chunks
    (321, 256, 0, 513, 1, 16, 577, 0, 64),                              # two chunks + a tile
)
COUNT_LAST = (100, TILE, TILE - 3)                                    # sites of each contig's last tile
OUTLIER_TILE = (1, 1)                                                  # (contig, tile): holds a deletion longer than the overhang
LENGTHS = (150, 114, 152, 250, 260, 60, 30)
QUALS = (60, 50, 41, 40, 31, 30, 29, 25)

SLOT_KINDS = ("mapq", "readq", "mapid", "aln_cov", "del", "ins", "lead_clip", "trail_clip", "five_op")
DROP_KINDS = SLOT_KINDS[:4]


def phase_iters(lanes):
    """Iterations of a phase: the largest even number (four at most) whose reads fit one lane each into a wave, else one."""
    rpw = 64 // lanes
    n = min(4, 64 // rpw)
    return n - (n & 1) if n >= 2 else 1


def slot_of(v, lanes):
    """Stream index v of a read in its tile -> (phase of the tile, slot in the phase): iteration v // rpw goes to wave it % 4
    as its (it // 4)-th, a phase holds phase_iters of a wave's iterations, the slot is (iteration of the phase, read of it)."""
    rpw, ph = 64 // lanes, phase_iters(lanes)
    it, g = divmod(v, rpw)
    k_it, wave = divmod(it, NWAVES)
    p, j = divmod(k_it, ph)
    return (p, wave), j * rpw + g


def stream_index(p, wave, slot, lanes):
    rpw, ph = 64 // lanes, phase_iters(lanes)
    j, g = divmod(slot, rpw)
    return ((p * ph + j) * NWAVES + wave) * rpw + g


def _seqs(rng, n, l):
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, l))]
    return [row.tobytes().decode() for row in a]


def _plain(pos, seq, qual, mapq=42):
    return dict(pos=pos, cigar=[(0, len(seq))], seq=seq, qual=qual, nm=0, mapq=mapq, kind="plain")


def odd_read(kind, pos, seq, qual, rng):
    """A read of the kind at the default thresholds: the first four are dropped by exactly one test of keep_read, the others kept."""
    l = len(seq)
    r = dict(pos=pos, cigar=[(0, l)], seq=seq, qual=qual, nm=0, mapq=42, kind=kind)
    if kind == "mapq":
        r["mapq"] = 19
    elif kind == "readq":
        r["qual"] = [19] * (l - 1) + [30]                      # mean below 20; one base that a kept read would tally
    elif kind == "mapid":
        r["nm"] = l // 16 + 1                                  # (l - nm) / l below 94 %
    elif kind == "aln_cov":
        r["cigar"] = [(4, l // 4 + 1), (0, l - l // 4 - 1)]    # the aligned part below 75 %
    elif kind == "del":
        a, d = rng.randint(1, l - 1), rng.randint(1, 7)
        r["cigar"], r["nm"] = [(0, a), (2, d), (0, l - a)], min(d, l // 20)
    elif kind == "ins":
        i = rng.randint(1, 4)
        a = rng.randint(1, l - i - 1)
        r["cigar"], r["nm"] = [(0, a), (1, i), (0, l - a - i)], i
    elif kind == "lead_clip":
        s = rng.randint(1, l // 5)
        r["cigar"] = [(4, s), (0, l - s)]
    elif kind == "trail_clip":
        s = rng.randint(1, l // 5)
        r["cigar"] = [(0, l - s), (4, s)]
    elif kind == "five_op":
        a = rng.randint(1, l - 10)
        r["cigar"], r["nm"] = [(0, a), (3, 3), (7, 6), (8, 2), (0, l - a - 8)], 2
    else:
        raise ValueError(kind)
    return r


def _table(lengths, begin, rng):
    ref = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, size=int(sum(lengths)))]
    return abi.ContigTable(length=list(lengths), species=[k % 2 for k in range(len(lengths))], read_begin=begin, ref=ref,
                           n_species=2, ids=["c%d" % k for k in range(len(lengths))], species_ids=["s0", "s1"])


@functools.lru_cache(maxsize=None)
def count_batch(read_len):
    """-> (ContigTable, ReadsSoA, reads as dicts, [per contig: reads that start in each tile]).  Nine reads in ten are one match,
    the others carry a clip, an indel or five ops; a read may hang over its tile's end, a chunk's and the contig's."""
    rng, nrng = random.Random(4100 + read_len), np.random.default_rng(4100 + read_len)
    reads, begin, lengths = [], [0], []
    for c, tiles in enumerate(COUNT_TILES):
        length = (len(tiles) - 1) * TILE + COUNT_LAST[c]
        rs = []
        for t, n in enumerate(tiles):
            lo, hi = t * TILE, min(length, (t + 1) * TILE)
            pos = sorted(rng.randrange(lo, hi) for _ in range(n))
            if n >= 2:
                pos[0], pos[-1] = lo, hi - 1                   # the tile's first and last site start a read
            seqs = _seqs(nrng, n, read_len)
            for k in range(n):
                qual = rng.choices(QUALS, k=read_len)
                u = rng.random()
                if u < 0.9:
                    r = _plain(pos[k], seqs[k], qual, mapq=rng.choice([42, 42, 42, 30, 19]))
                    r["nm"] = rng.choice([0, 0, 1, 2, read_len // 16 + 1])
                else:
                    r = odd_read(rng.choice(SLOT_KINDS[4:]), pos[k], seqs[k], qual, rng)
                rs.append(r)
            if (c, t) == OUTLIER_TILE:      # spans more than either overhang: its chunk is piled up tile by tile
                rs.append(dict(pos=lo + 900, cigar=[(0, read_len // 3), (2, 700), (0, read_len - read_len // 3)], seq=_seqs(nrng, 1, read_len)[0],
                               qual=[40] * read_len, nm=0, mapq=42, kind="outlier"))
        rs.sort(key=lambda r: r["pos"])
        reads += rs
        begin.append(len(reads))
        lengths.append(length)
    starts = [[sum(1 for r in reads[begin[c]:begin[c + 1]] if r["pos"] // TILE == t)
               for t in range(len(tiles))] for c, tiles in enumerate(COUNT_TILES)]
    return _table(lengths, begin, nrng), H.reads_from_border_dicts(reads), reads, starts


@functools.lru_cache(maxsize=None)
def slot_batch(kind, read_len):
    """-> (ContigTable, ReadsSoA, reads as dicts, {slot: set of (odd read kept?, neighbours kept?)}).  Contig 0: one chunk, contig 1:
    up to three; every tile starts a whole number of phases for each of its four waves, and no read reaches the
    next tile, so a tile's stream is its own reads in order and slot_of holds.  The k-th phase's odd read sits in slot k mod
    (slots of a phase); the second half of the phases has plain neighbours that mapq drops (and, for the kinds that drop the odd
    read, a KEPT plain read in its place): the odd slot is the one that differs from its neighbours either way."""
    lb, lanes = H.direct_lane_shape(read_len)
    rpw, ph = 64 // lanes, phase_iters(lanes)
    slots = ph * rpw
    block = slots * NWAVES                               # reads of one phase of every wave
    seed = SLOT_KINDS.index(kind) * 1000 + read_len
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    n_phases = 2 * slots                                 # every slot once per half
    n_blocks = n_phases // NWAVES
    per_tile = [4 * block] * 2 + [2 * block] * ((n_blocks - 8) // 2) + [block] * (n_blocks & 1)
    assert sum(per_tile) == n_phases * slots
    tiles_of = (per_tile[:4], per_tile[4:])
    assert len(tiles_of[0]) == 4 and 5 <= len(tiles_of[1]) <= 12, per_tile
    reach = read_len + 8
    reads, begin, lengths, k, seen = [], [0], [], 0, {}
    for tiles in tiles_of:
        rs = []
        for t, n in enumerate(tiles):
            pos = sorted(rng.randrange(t * TILE, (t + 1) * TILE - reach - 1) for _ in range(n))
            seqs = _seqs(nrng, n, read_len)
            inverse = {}                                 # stream index of the tile -> its phase's half
            odd = {}
            for p in range(n // block):
                for w in range(NWAVES):
                    second = k >= n_phases // 2
                    v = stream_index(p, w, k % slots, lanes)
                    odd[v] = second
                    inverse[(p, w)] = second
                    k += 1
            for v in range(n):
                phase, slot = slot_of(v, lanes)
                second = inverse[phase]
                qual = rng.choices(QUALS, k=read_len)
                if v in odd:
                    if second and kind in DROP_KINDS:
                        r = _plain(pos[v], seqs[v], qual)
                    else:
                        r = odd_read(kind, pos[v], seqs[v], qual, rng)
                    kept = second or kind not in DROP_KINDS
                    seen.setdefault(slot, set()).add((kept, not second))
                else:
                    r = _plain(pos[v], seqs[v], qual, mapq=19 if second else 42)
                r["kept"] = (v in odd and kept) or (v not in odd and not second)
                rs.append(r)
        reads += rs
        begin.append(len(reads))
        lengths.append(len(tiles) * TILE)
    assert k == n_phases
    return _table(lengths, begin, nrng), H.reads_from_border_dicts(reads), reads, seen


ERROR_SLOTS = (0, 1, 17, 63, 64, 255, 256 + 3 * 16 + 5, 600)        # stream indices of the one tile: first / last slots, a tail phase


@functools.lru_cache(maxsize=None)
def error_batch(kinds, where):
    """601 reads of 150 bases that start in one tile (wave 0: ten iterations, three phases) on a contig of two tiles; read where[i]
    is of kinds[i]: "no_nm", "no_qual" (on a read that passes mapid) or "overrun" (a match op runs past the read's end)."""
    rng, nrng = random.Random(77 + sum(where)), np.random.default_rng(77 + sum(where))
    n, l = 601, 150
    pos = sorted(rng.randrange(0, TILE - 200) for _ in range(n))
    seqs = _seqs(nrng, n, l)
    reads = [_plain(pos[v], seqs[v], rng.choices(QUALS, k=l)) for v in range(n)]
    for kind, v in zip(kinds, where):
        if kind == "no_nm":
            reads[v]["nm"] = None
        elif kind == "no_qual":
            reads[v]["qual"] = [0xFF] * l
        elif kind == "overrun":
            reads[v]["cigar"] = [(0, l + 2)]
        else:
            raise ValueError(kind)
    return _table([2 * TILE], [0, n], nrng), H.reads_from_dicts(reads), reads


ERROR_CODES = {"no_nm": abi.ERR_READ_NO_NM, "no_qual": abi.ERR_READ_NO_QUAL, "overrun": abi.ERR_READ_CIGAR_OVERRUN}
OTHER_THRESHOLDS = dict(mapid=90.0, mapq=31, baseq=41, readq=33, aln_cov=0.5)


def _exact_on_the_direct_path(ctx, table, soa, max_len, thresholds, packed=True):
    """The batch on the direct path, run once per entry of `thresholds` (nothing may stay from the run before), each time equal
    to the oracle's counts, reference alleles and counters; then once on the packed path."""
    b = ctx.batch(table, soa)
    try:
        b.select_path(abi.PATH_DIRECT)
        info = b.info()
        assert (info.lane_bases, info.lanes_per_read) == H.direct_lane_shape(max_len)
        for args in thresholds:
            thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, **args))
            st, er, oc, oa, os_ = c_oracle.pileup(thr, table, soa)
            assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
            b.run(thr)
            counts, allele, stats = b.fetch()
            bad = np.nonzero((counts != oc).any(axis=1))[0]
            assert bad.size == 0, "direct: counts differ at %d sites, first %s: hip %s oracle %s" % (
                bad.size, bad[:5], counts[bad[:5]].tolist(), oc[bad[:5]].tolist())
            assert np.array_equal(allele, oa)
            assert np.array_equal(stats, os_), "counters: hip %s oracle %s" % (stats.tolist(), os_.tolist())
        if packed:
            b.select_path(abi.PATH_PACKED)
            b.run(thr)
            c2, a2, s2 = b.fetch()
            assert np.array_equal(c2, counts) and np.array_equal(a2, allele) and np.array_equal(s2, stats)
    finally:
        b.close()
    return info


@pytest.mark.parametrize("read_len", LENGTHS)
def test_tiles_of_every_phase_count(hip_ctx, read_len):
    table, soa, _, _ = count_batch(read_len)
    info = _exact_on_the_direct_path(hip_ctx, table, soa, read_len, [{}, OTHER_THRESHOLDS])
    want = {150: (38, 4), 114: (38, 3), 152: (32, 5), 250: (32, 8), 260: (30, 9), 60: (30, 2), 30: (30, 1)}[read_len]
    assert (info.lane_bases, info.lanes_per_read) == want
    assert info.direct_chunk_tiles == 4 and info.direct_overhang == (160 if read_len <= 160 else 288)


@pytest.mark.parametrize("baseq", [0, 30])
@pytest.mark.parametrize("kind", SLOT_KINDS)
def test_an_odd_read_in_every_slot(hip_ctx, kind, baseq):
    table, soa, _, _ = slot_batch(kind, 150)
    info = _exact_on_the_direct_path(hip_ctx, table, soa, 150, [dict(baseq=baseq), dict(OTHER_THRESHOLDS, baseq=30 - baseq)],
                                     packed=False)
    assert (info.lane_bases, info.lanes_per_read) == (38, 4)


@pytest.mark.parametrize("read_len", [114, 152])
@pytest.mark.parametrize("kind", ["mapq", "del", "five_op"])
def test_an_odd_read_in_every_slot_of_other_lane_counts(hip_ctx, kind, read_len):
    table, soa, _, _ = slot_batch(kind, read_len)
    info = _exact_on_the_direct_path(hip_ctx, table, soa, read_len, [{}, OTHER_THRESHOLDS], packed=False)
    assert (info.lane_bases, info.lanes_per_read) == {114: (38, 3), 152: (32, 5)}[read_len]


def _refused_as_the_oracle_refuses(ctx, kinds, where):
    table, soa, _ = error_batch(kinds, where)
    thr = abi.Thresholds.from_args(abi.DEFAULT_ARGS)
    st, er, *_ = c_oracle.pileup(thr, table, soa)
    assert st != 0
    b = ctx.batch(table, soa)
    try:
        b.select_path(abi.PATH_DIRECT)
        info = b.info()
        assert (info.lane_bases, info.lanes_per_read) == (38, 4)
        with pytest.raises(abi.MidasSnpsError) as ei:
            b.run(thr)
            b.fetch()
        assert (ei.value.status, ei.value.read_index) == (st, er)
    finally:
        b.close()
    return st, er


@pytest.mark.parametrize("where", ERROR_SLOTS)
@pytest.mark.parametrize("kind", sorted(ERROR_CODES))
def test_a_refused_read_in_a_chosen_slot(hip_ctx, kind, where):
    assert _refused_as_the_oracle_refuses(hip_ctx, (kind,), (where,)) == (ERROR_CODES[kind], where)


@pytest.mark.parametrize("kinds,where", [(("no_qual", "no_nm"), (3, 70)), (("overrun", "no_nm"), (16 * 4 + 2, 16 * 8 + 1)),
                                         (("no_nm", "no_qual"), (257, 256 + 16 * 12)), (("no_qual", "overrun"), (599, 600))])
def test_of_two_refused_reads_in_a_phase_the_lower_index_wins(hip_ctx, kinds, where):
    assert slot_of(where[0], 4)[0] == slot_of(where[1], 4)[0]                  # one phase of one wave
    assert _refused_as_the_oracle_refuses(hip_ctx, kinds, where) == (ERROR_CODES[kinds[0]], where[0])
