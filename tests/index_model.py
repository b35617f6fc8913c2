"""A plain model of the direct path's index pass (index_direct.hip + the host logic of batch_direct.hip), from its definitions
alone: the contig table (length, read_begin) and the reads' pos, l_seq, CIGAR ops, nm and mapq go in; the batch's facts, the
outlier list, the tile flags, chunk_ok and every tile's read range [tbegin, tend) come out.  None of the library's code is used:
tests/test_index_model_host.py holds the model to brute force, tests/test_gpu_index.py holds the device to the model.

  span     sum of the lengths of M, =, X, D, N (capped at 0x3FFFFFFF); pc = pos clamped to the contig; tile of a site =
           tile_base[contig] + (site >> 11)
  facts    unsorted: some read other than its contig's first starts (clamped) in front of the read before it; the overhang H is
           160, or 288 for a sorted batch whose longest read is 161..288 bases; a read is an OUTLIER iff span > H
  ranges   sorted:   tend[t] = the first read that starts behind tile t, tbegin[t] = the first read whose start + reach gets to t
           unsorted: the lowest / highest read + 1 among those whose [tile(pc), tile(pc + reach)] holds t
           listed outliers lower tbegin over the tiles behind their own that they reach
"""
import numpy as np

TILE_SHIFT = 11
TILE = 1 << TILE_SHIFT
OVERHANG, OVERHANG_LONG = 160, 288
CHUNK_TILES, TAIL_DIV = 4, 8
NONE = 0xFFFFFFFF
MAX_SPAN = 0x3FFFFFFF
MAX_L_SEQ, MAX_FIELD16 = 1024, 65534          # beyond them a read sends its batch to the long path (not modelled: no ranges)
MAX_FAST_GAP = 65535
_M, _I, _D, _N, _S, _EQ, _X = 0, 1, 2, 3, 4, 7, 8
_MATCH = (_M, _EQ, _X)


def cigar_span(cigar):
    return min(sum(n for op, n in cigar if op in (_M, _EQ, _X, _D, _N)), MAX_SPAN)


def _op_class(op):
    return 0 if op in _MATCH else 1 if op == _S else 2 if op in (_I, _D, _N) else 3


def fast_shape(cigar, l_seq):
    """The CIGARs the pileup kernel settles in registers: `S? (M|=|X) ((I|D|N) (M|=|X))? S?` in at most four ops, one op per
    match run, the lengths of S / M / I adding up to l_seq, at least one aligned base, a deletion or skip of at most 65 535."""
    nc = len(cigar)
    if not 1 <= nc <= 4:
        return False
    lead = cigar[0][1] if _op_class(cigar[0][0]) == 1 else 0
    rest = cigar[1:] if _op_class(cigar[0][0]) == 1 else cigar
    want = {1: [0], 2: [0, 1], 3: [0, 2, 0], 4: [0, 2, 0, 1]}
    if len(rest) not in want or [_op_class(op) for op, _ in rest] != want[len(rest)] or len(cigar) > 4:
        return False
    m1 = rest[0][1]
    gap_op, gap = rest[1] if len(rest) >= 3 else (None, 0)
    ins = gap if gap_op == _I else 0
    m2 = rest[2][1] if len(rest) >= 3 else 0
    trail = rest[1][1] if len(rest) == 2 else rest[3][1] if len(rest) == 4 else 0
    alen = m1 + ins + m2
    return lead + alen + trail == l_seq and alen >= 1 and gap - ins <= MAX_FAST_GAP


def cigars_of(cigar, cigar_off):
    """[(op, len)] per read from BAM's packed column and its CSR offsets."""
    return [[(int(v) & 15, int(v) >> 4) for v in cigar[int(cigar_off[i]):int(cigar_off[i + 1])]] for i in range(len(cigar_off) - 1)]


def index_model(length, read_begin, pos, l_seq, cigars, nm, mapq=None):
    """-> dict: facts (the names of abi.INDEX_FACTS), outliers (sorted (read, t_first, t_last)), tile_flag, chunk_ok, tbegin, tend,
    stream_reads, max_tile_reads, chunk_tiles, info_overhang.  mapq takes no part in the index pass (accepted for symmetry)."""
    length = [int(x) for x in length]
    read_begin = [int(x) for x in read_begin]
    n_contigs, n_reads = len(length), len(pos)
    assert len(read_begin) == n_contigs + 1 and read_begin[0] == 0 and read_begin[-1] == n_reads
    tile_base = [0]
    for ln in length:
        tile_base.append(tile_base[-1] + (ln + TILE - 1) // TILE)
    n_tiles = tile_base[-1]
    contig = [0] * n_reads
    for c in range(n_contigs):
        for i in range(read_begin[c], read_begin[c + 1]):
            contig[i] = c
    pos = [int(x) for x in pos]
    l_seq = [int(x) for x in l_seq]
    nm = [int(x) for x in nm]
    last = [length[contig[i]] - 1 for i in range(n_reads)]
    pc = [min(max(pos[i], 0), last[i]) for i in range(n_reads)]
    span = [cigar_span(cg) for cg in cigars]
    tile = lambda i, site: tile_base[contig[i]] + (site >> TILE_SHIFT)
    assert all(l <= MAX_L_SEQ for l in l_seq) and all(len(cg) <= MAX_FIELD16 for cg in cigars) and all(x <= MAX_FIELD16 for x in nm)

    # ---- the facts ------------------------------------------------------------------------------------------------------------
    unsorted = int(any(i != read_begin[contig[i]] and pc[i - 1] > pc[i] for i in range(n_reads)))
    max_l = max(l_seq, default=0)
    H = OVERHANG_LONG if not unsorted and OVERHANG < max_l <= OVERHANG_LONG else OVERHANG
    outlier = [s > H for s in span]
    max_span = max(span, default=0)
    max_common = max((s for s, o in zip(span, outlier) if not o), default=0)
    reach = max(1, max_l, max_span)
    listed, tile_flag = [], np.zeros(n_tiles, np.uint8)
    for i in range(n_reads):
        if not outlier[i]:
            continue
        e = min(pos[i] + span[i] - 1, last[i])
        if e < pc[i]:
            continue
        if tile(i, e) > tile(i, pc[i]):
            listed.append((i, tile(i, pc[i]) + 1, tile(i, e)))
        if e - (pc[i] >> TILE_SHIFT << TILE_SHIFT) >= TILE + H:
            tile_flag[tile(i, pc[i]):tile(i, e) + 1] = 1
    cap = max(4096, n_reads // 64)
    chunks = not unsorted and max_l <= H and len(listed) <= cap
    n_out = sum(outlier)
    reach_ranges = max(1, max_l, max_common) if chunks and n_out > 0 else reach
    chunk_ok = np.zeros(0, np.uint8)
    if chunks and n_out > 0:
        n_chunked = (n_tiles - n_tiles // TAIL_DIV) // CHUNK_TILES * CHUNK_TILES
        chunk_ok = np.ones(max(1, n_chunked // CHUNK_TILES), np.uint8)
        for t in range(n_chunked):
            if tile_flag[t]:
                chunk_ok[t // CHUNK_TILES] = 0
    alg = sum((l + 1) // 2 + l + 4 * len(cg) + 16 for l, cg in zip(l_seq, cigars))
    n_general = sum(1 for i in range(n_reads)
                    if not (fast_shape(cigars[i], l_seq[i]) and nm[i] >= 0 and 0 <= pos[i] < length[contig[i]]))
    facts = dict(status=-1, alg=alg, n_general=n_general, n_long=0, n_outliers=n_out, max_l=max_l, max_span=max_span,
                 max_common=max_common, unsorted=unsorted, direct_reach=reach, direct_reach_ranges=reach_ranges, direct_overhang=H,
                 direct_chunks=int(chunks), n_outliers_listed=len(listed) if chunks else 0, outlier_cap=cap)

    # ---- the ranges -----------------------------------------------------------------------------------------------------------
    tbegin, tend = np.full(n_tiles, NONE, np.uint32), np.zeros(n_tiles, np.uint32)
    ka = [tile(i, pc[i]) for i in range(n_reads)]
    kb = [tile(i, min(pc[i] + reach_ranges, last[i])) for i in range(n_reads)]
    if not unsorted:
        for c in range(n_contigs):
            lo, hi = read_begin[c], read_begin[c + 1]
            if lo == hi:
                continue
            i = j = lo
            for t in range(tile_base[c], tile_base[c + 1]):
                while i < hi and ka[i] <= t:         # i: the first read that starts behind t
                    i += 1
                tend[t] = i
                while j < hi and kb[j] < t:          # j: the first read that gets to t
                    j += 1
                if j < hi:
                    tbegin[t] = j
    else:
        for i in range(n_reads):
            for t in range(ka[i], kb[i] + 1):
                tbegin[t] = min(int(tbegin[t]), i)
                tend[t] = max(int(tend[t]), i + 1)
    if reach_ranges != reach:
        for i, t0, t1 in listed:
            for t in range(t0, t1 + 1):
                tbegin[t] = min(int(tbegin[t]), i)
    streams = np.maximum(tend.astype(np.int64) - tbegin.astype(np.int64), 0)
    return dict(facts=facts, outliers=sorted(listed) if chunks else [], tile_flag=tile_flag, chunk_ok=chunk_ok, tbegin=tbegin, tend=tend,
                stream_reads=int(streams.sum()), max_tile_reads=int(streams.max()) if n_tiles else 0,
                chunk_tiles=CHUNK_TILES if chunks else 1, info_overhang=H if chunks else OVERHANG,
                n_tiles=n_tiles, tile_base=tile_base, reach_ranges=reach_ranges, ka=ka, kb=kb, pc=pc, span=span, contig=contig)
