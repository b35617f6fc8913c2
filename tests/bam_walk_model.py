"""A plain sequential model of the device BAM record walk (bam_walk.hip, decode_plan.h) and the BAM files that make its guesses
wrong.  Pure Python and numpy, no device.

The device cuts the inflated stream into chunks of at most 32 KiB.  One thread per chunk GUESSES a record boundary (the first
offset from which four records in a row pass plausible(), or fewer if the chain reaches the end of the segment) and follows
block_size from there to the end of its chunk.  The host stitches the chunks in order; a chunk whose guess the true chain does not
hit is walked a second time from where the chain stands.  Here the same steps are written out one after the other:

  records(stream)      the serial walk from the header's end: the truth
  plausible(...)       bam_walk.hip's test, field for field
  guess(...)           the kernel's scan of one chunk
  walk(...)            a chunk's kept / unmapped / first unmapped / end / bad from a given start
  grid(...)            decode_plan.h ChunkWalk::add_segment
  stitch(...)          decode_plan.h stitch_chunks, with the count of second walks
  whole_file / streamed / slice_walk   the grids the routes of the decode lay over a stream

and the fixture builders write well-formed BAMs (midas_amd.bam.write_bam) whose QUAL bytes spell tiny records, whose names the
plausibility test refuses, or whose records start at chosen distances from a chunk border.  Every builder returns a Fixture: the
path, the inflated stream, what was written and what the model predicts for a walk of the whole file from the header's end."""
import gzip
import struct

import numpy as np

from midas_amd import abi, bam, synth

CHUNK = 32768                 # decode_plan.h kWalkChunk
CHAIN = 4                     # bam_walk.hip kChain
TAIL_BLOCKS = 8               # bam_device.hip kTail: blocks a streamed group keeps behind its last
NONE = -1                     # "no offset" (the kernels' ~0ull)
DECOY_BYTES = 37              # 4 + 33: block_size and a record of nothing but its fixed fields and an empty name


# ---- the stream -------------------------------------------------------------------------------------------------------------------

def inflate(path):
    return gzip.open(path, "rb").read()


def header(stream):
    """-> (the header's end = the first record's offset, the reference lengths)"""
    p = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref, = struct.unpack_from("<i", stream, p)
    p += 4
    ref_lens = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, p)
        ref_lens.append(struct.unpack_from("<i", stream, p + 4 + l_name)[0])
        p += 8 + l_name
    return p, ref_lens


def _nm(aux):
    """NM of an aux block, any integer width; -1: none"""
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    p = 0
    while p + 3 <= len(aux):
        tag, ty = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if ty in sizes:
            sz = sizes[ty]
        elif ty in "ZH":
            sz = aux.index(b"\0", p) - p + 1
        elif ty == "B":
            sz = 5 + struct.unpack_from("<I", aux, p + 1)[0] * {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(aux[p]), 4)
        else:
            return -1
        if tag == b"NM":
            return struct.unpack_from("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], aux, p)[0] if ty in "cCsSiI" else -1
        p += sz
    return -1


def records(stream):
    """The serial walk from the header's end: every record's offset, refID, pos, mapq, flag, l_seq, n_cigar and NM (int64 arrays),
    and l_read_name (for the builders)."""
    p, _ = header(stream)
    total = len(stream)
    cols = {k: [] for k in ("offset", "refid", "pos", "mapq", "flag", "l_seq", "n_cigar", "nm", "l_name", "size")}
    while p < total:
        bs, refid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHI", stream, p)
        assert bs >= 32 and p + 4 + bs <= total, "the fixtures hold no malformed record"
        body = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        for k, v in zip(cols, (p, refid, pos, mapq, flag, l_seq, n_cig, _nm(stream[p + 4 + body:p + 4 + bs]), l_name, 4 + bs)):
            cols[k].append(v)
        p += 4 + bs
    assert p == total
    return {k: np.array(v, np.int64) for k, v in cols.items()}


def qual_begin(rec, i):
    """where record i's QUAL bytes start in the stream"""
    return int(rec["offset"][i] + 36 + rec["l_name"][i] + 4 * rec["n_cigar"][i] + (rec["l_seq"][i] + 1) // 2)


# ---- bam_walk.hip -----------------------------------------------------------------------------------------------------------------

def plausible(stream, u, total, ref_lens):
    """Could an alignment record start at u?  -> its block_size, or None."""
    if u + 36 > total:
        return None
    bs, refid, pos, lrn, _mapq, _bin, n_cig, _flag, l, nref, npos = struct.unpack_from("<IiiBBHHHIii", stream, u)
    if bs < 32 or bs > (1 << 26):
        return None
    n_ref = len(ref_lens)
    if refid < -1 or refid >= n_ref or nref < -1 or nref >= n_ref or pos < -1 or npos < -1:
        return None
    if refid >= 0 and pos > ref_lens[refid]:
        return None
    if lrn < 1 or l > (1 << 26):
        return None
    if 32 + lrn + 4 * n_cig + (l + 1) // 2 + l > bs:
        return None
    if u + 4 + 32 + lrn + 4 * n_cig > total:
        return None
    name = u + 36
    if stream[name + lrn - 1] != 0:
        return None
    for k in range(lrn - 1):
        if stream[name + k] < 33 or stream[name + k] > 126:
            return None
    cg = name + lrn
    for k in range(min(n_cig, 64)):
        if (struct.unpack_from("<I", stream, cg + 4 * k)[0] & 15) > 8:
            return None
    return bs


def guess(stream, lo, hi, total, ref_lens, chain=CHAIN):
    """The kernel's scan of chunk [lo, hi) of a segment that ends at `total`: the first offset from which `chain` plausible
    records follow one another, or fewer when the chain arrives exactly at `total`.  NONE: no such offset."""
    u = lo
    while u < hi and u + 36 <= total:
        v, ok = u, 0
        while ok < chain:
            if v == total:                 # the segment ends on a record boundary: as good as a full chain
                break
            bs = plausible(stream, v, total, ref_lens)
            if bs is None:
                ok = -1
                break
            v += 4 + bs
            if v > total:
                ok = -1
                break
            ok += 1
        if ok >= 0:
            return u
        u += 1
    return NONE


def walk(stream, start, hi, stop, total, offsets=None):
    """A chunk's walk from `start`: -> (kept, unmapped, first_unmapped, end, bad).  offsets (a list): the kept records' are appended
    (bam_offsets_kernel)."""
    stop = min(stop, hi)
    kept = unmapped = bad = 0
    first_unmapped = NONE
    q = start
    if start != NONE:
        while q + 4 <= total and q < stop:
            bs, refid = struct.unpack_from("<Ii", stream, q)
            if bs < 32 or q + 4 + bs > total:
                bad = 1
                break
            if refid >= 0:
                kept += 1
                if offsets is not None:
                    offsets.append(q)
            else:
                if not unmapped:
                    first_unmapped = q
                unmapped += 1
            q += 4 + bs
    return kept, unmapped, first_unmapped, q, bad


# ---- decode_plan.h ----------------------------------------------------------------------------------------------------------------

def grid(frm, seg_stop, limit, exact):
    """ChunkWalk::add_segment: the chunks over [frm, seg_stop) of a segment that ends at `limit`."""
    out = []
    at = frm
    while at < seg_stop:
        first = at == frm
        out.append(dict(lo=at, hi=min(at + CHUNK, seg_stop), stop=seg_stop, limit=limit, forced=first and exact,
                        start=frm if first and exact else NONE))
        at += CHUNK
    return out


def first_walk(stream, chunks, ref_lens, chain=CHAIN):
    """The kernel's first launch: every chunk's guess (or its forced start) and the walk from it."""
    for c in chunks:
        if not c["forced"]:
            c["start"] = guess(stream, c["lo"], c["hi"], c["limit"], ref_lens, chain)
        c["guess"] = c["start"]
        c["kept"], c["unmapped"], c["first_unmapped"], c["end"], c["bad"] = walk(stream, c["start"], c["hi"], c["stop"], c["limit"])
        c["again"] = False
    return chunks


def stitch(stream, chunks, cur):
    """stitch_chunks over chunks that first_walk filled; cur: where the chain starts (NONE: at the first guessed boundary).
    -> dict(what, first, end, first_unmapped, n_records, n_unmapped, again: the second walks).  A chunk walked again has
    c['again'] set and its results replaced; a chunk in which no record of the chain starts is emptied."""
    r = dict(what="settled", first=NONE, end=NONE, first_unmapped=NONE, n_records=0, n_unmapped=0, again=0)
    i = 0
    while i < len(chunks):
        c = chunks[i]
        if cur == NONE:
            if c["start"] == NONE:
                c["kept"] = c["unmapped"] = 0
                i += 1
                continue
            cur = c["start"]
        if cur >= c["hi"] or cur + 4 > c["limit"]:
            c["kept"] = c["unmapped"] = 0
            c["start"] = NONE
            i += 1
            continue
        if c["start"] == cur:
            if c["bad"]:
                r["what"] = "bad_chunk"
                return r
            if r["first"] == NONE:
                r["first"] = cur
            r["n_records"] += c["kept"]
            if c["unmapped"] and r["first_unmapped"] == NONE:
                r["first_unmapped"] = c["first_unmapped"]
            r["n_unmapped"] += c["unmapped"]
            cur = c["end"]
            i += 1
            continue
        r["again"] += 1
        c["again"] = True
        c["start"] = cur
        c["kept"], c["unmapped"], c["first_unmapped"], c["end"], c["bad"] = walk(stream, cur, c["hi"], c["stop"], c["limit"])
    r["end"] = cur
    return r


def kept_offsets(stream, chunks):
    """bam_offsets_kernel over settled chunks: the offset of every kept record, in order"""
    out = []
    for c in chunks:
        if c["kept"]:
            walk(stream, c["start"], c["hi"], c["stop"], c["limit"], out)
    return out


# ---- the grids of the routes ------------------------------------------------------------------------------------------------------

def whole_file(stream):
    """One segment from the header's end to the stream's (read_bam(resident=True) in one arena, midas_genes_count_bam).
    -> (chunks, result of the stitching, kept offsets)"""
    rec_begin, ref_lens = header(stream)
    total = len(stream)
    chunks = first_walk(stream, grid(rec_begin, total, total, True), ref_lens)
    r = stitch(stream, chunks, rec_begin)
    return chunks, r, kept_offsets(stream, chunks)


def streamed(path, stream, group_blocks, tail=TAIL_BLOCKS):
    """The streamed decode (bam_device.hip): groups of whole BGZF blocks (the file's table, its empty last block included), each
    walked over a grid that starts exactly where the chain of the group before ended and sees the group's blocks and `tail` more.
    group_blocks: what MIDAS_SNPS_DECODE_GROUP_BLOCKS says.
    -> (groups the plan holds, second walks, kept offsets); None: the decode is not streamed or gives up."""
    rec_begin, ref_lens = header(stream)
    total = len(stream)
    upos = [u for _, u in bgzf_blocks(path)[0]] + [total]
    nb = len(upos) - 1
    if nb <= group_blocks + group_blocks // 4:
        return None
    k = (nb + group_blocks - 1) // group_blocks
    group = (nb + k - 1) // k
    cur, again, offs, groups = rec_begin, 0, [], (nb + group - 1) // group
    for g in range(groups):
        b_lo, b_hi = g * group, min(nb, (g + 1) * group)
        stop = total if b_hi == nb else min(total, upos[b_hi])
        limit = upos[min(nb, b_hi + tail)]
        chunks = first_walk(stream, grid(cur, stop, limit, True), ref_lens)
        r = stitch(stream, chunks, cur)
        if r["what"] != "settled":
            return None
        again += r["again"]
        offs += kept_offsets(stream, chunks)
        if r["end"] != NONE:
            cur = r["end"]
        if cur >= total:
            break
    return groups, again, offs


def bgzf_blocks(path):
    """[(file offset, inflated offset)] of every block of the file, and the file's size"""
    blob = open(path, "rb").read()
    out, p, u = [], 0, 0
    while p < len(blob):
        size = int.from_bytes(blob[p + 16:p + 18], "little") + 1
        isize, = struct.unpack_from("<I", blob, p + size - 4)
        out.append((p, u))
        u += isize
        p += size
    return out, len(blob)


def slice_bytes(path, k, n, stream):
    """[u_lo, u_hi): the inflated bytes of slice k of n (the blocks whose file offset falls into its share of the file's bytes)"""
    blocks, size = bgzf_blocks(path)
    rec_begin, _ = header(stream)

    def first_at(fpos):
        return next((u for f, u in blocks if f >= fpos), len(stream))
    lo = blocks[0][1] if k == 0 else first_at(size * k // n)
    hi = len(stream) if k + 1 == n else first_at(size * (k + 1) // n)
    return max(lo, rec_begin), max(hi, rec_begin)


def slice_walk(path, k, n, stream):
    """A rank's slice walked on the device (midas_bam_open_slice_device): a grid from the slice's first byte, which only slice 0
    knows to be a record's.  -> (u_lo, u_hi, result of the stitching; None for an empty slice)"""
    rec_begin, ref_lens = header(stream)
    u_lo, u_hi = slice_bytes(path, k, n, stream)
    if u_lo >= u_hi:
        return u_lo, u_hi, None
    exact = u_lo == rec_begin
    chunks = first_walk(stream, grid(u_lo, u_hi, len(stream), exact), ref_lens)
    return u_lo, u_hi, stitch(stream, chunks, u_lo if exact else NONE)


# ---- decoys -----------------------------------------------------------------------------------------------------------------------

def decoy_record(refid=0, pos=5, block_size=33):
    """4 + 33 bytes that pass for an alignment record: refID 0 or -1, a position in range, l_read_name 1 whose one byte is NUL, mapq
    30, no CIGAR, no bases, next refID / next pos -1.  block_size: 33, its own size, unless the record is to reach further."""
    rec = bytearray(33)
    rec[0:4] = np.int32(refid).tobytes(); rec[4:8] = np.int32(pos).tobytes()
    rec[8] = 1; rec[9] = 30
    rec[20:24] = np.int32(-1).tobytes(); rec[24:28] = np.int32(-1).tobytes()
    return np.int32(block_size).tobytes() + bytes(rec)


def decoy_records(n, unmapped=()):
    """n decoy records one behind the other, at positions 5, 6, ...; unmapped: which of them carry refID -1"""
    return b"".join(decoy_record(-1 if k in unmapped else 0, 5 + k) for k in range(n))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

class Fixture:
    """A BAM on disk, its inflated stream, what was written, and the model's verdict on a walk of the whole file."""

    def __init__(self, name, path, contigs, refid, reads, names, **facts):
        self.name, self.path, self.contigs = name, path, contigs
        self.ref_names, self.ref_lens = list(contigs.ids), [int(x) for x in contigs.length]
        bam.write_bam(path, self.ref_names, self.ref_lens, refid, reads, read_names=names)
        self.stream = inflate(path)
        self.rec_begin, _ = header(self.stream)
        self.total = len(self.stream)
        self.written_refid, self.written = np.asarray(refid, np.int32), reads
        kept = np.flatnonzero(self.written_refid >= 0)
        # what a decode returns: the records with a reference, in file order
        self.refid = self.written_refid[kept]
        self.reads = reads if kept.size == reads.n_reads else synth.take_reads(reads, kept)
        self.dropped = int(reads.n_reads - kept.size)
        self.truth = records(self.stream)
        self.chunks, self.result, self.offsets = whole_file(self.stream)
        self.again = self.result["again"]
        self.facts = facts

    def border(self, c):
        return self.rec_begin + c * CHUNK

    def true_starts(self):
        return set(int(x) for x in self.truth["offset"])


def plain_dataset():
    """3000 reads of 320 bases over three references, fixed length"""
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=3, contig_len=60000, n_reads=3000, read_len=320, seed=22,
                                        var_len=False)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    return contigs, refid, reads


def plain_names(n):
    return ["r%d" % i for i in range(n)]


_PLAIN = {}


def _plain(tmp):
    """the plain file, written once: its dataset and the layout the placements are derived from"""
    if "rec" not in _PLAIN:
        contigs, refid, reads = plain_dataset()
        path = str(tmp / "plain_layout.bam")
        bam.write_bam(path, list(contigs.ids), [int(x) for x in contigs.length], refid, reads)
        stream = inflate(path)
        _PLAIN.update(contigs=contigs, refid=refid, reads=reads, rec=records(stream), rec_begin=header(stream)[0], total=len(stream))
    return _PLAIN


def _with_qual(reads, qual):
    return abi.ReadsSoA(**{**reads.as_dict(), "qual": qual})


def _put(qual, reads, rec, i, stream_at, data):
    """data into read i's QUAL, at the place that lies at stream_at of the inflated stream"""
    q0 = int(reads.qual_off[i]) + stream_at - qual_begin(rec, i)
    assert int(reads.qual_off[i]) <= q0 and q0 + len(data) <= int(reads.qual_off[i + 1])
    qual[q0:q0 + len(data)] = np.frombuffer(data, np.uint8)


def plain(tmp):
    p = _plain(tmp)
    return Fixture("plain", str(tmp / "plain.bam"), p["contigs"], p["refid"], p["reads"], None)


def _decoys_at_borders(tmp, name, n_decoys):
    p = _plain(tmp)
    rec, reads = p["rec"], p["reads"]
    fake = decoy_records(n_decoys, unmapped=(1,))
    qual = reads.qual.copy()
    placed = []
    c = 1
    while p["rec_begin"] + c * CHUNK < p["total"]:
        b = p["rec_begin"] + c * CHUNK
        i = int(np.searchsorted(rec["offset"], b, side="right")) - 1           # the read that holds this border
        at = max(b, qual_begin(rec, i))
        if at + CHAIN * DECOY_BYTES <= qual_begin(rec, i) + int(rec["l_seq"][i]):      # (room for four, whichever count is written)
            _put(qual, reads, rec, i, at, fake)
            placed.append((c, at))
        c += 1
    return Fixture(name, str(tmp / (name + ".bam")), p["contigs"], p["refid"], _with_qual(reads, qual), None, placed=placed)


def decoy4(tmp):
    """four decoy records in the QUAL bytes behind a chunk border: the guess falls in front of the true boundary"""
    return _decoys_at_borders(tmp, "decoy4", 4)


def decoy3(tmp):
    """three decoys, then the read's own qualities: one short of kChain, no guess is fooled"""
    return _decoys_at_borders(tmp, "decoy3", 3)


def refused_names(tmp):
    """The first true record behind every border has a name the plausibility test refuses (a space, or bytes at or above 0x80), of
    the byte length it had: the guess falls BEHIND the true boundary."""
    p = _plain(tmp)
    rec = p["rec"]
    names = plain_names(p["reads"].n_reads)
    changed = []
    c = 1
    while p["rec_begin"] + c * CHUNK < p["total"]:
        i = int(np.searchsorted(rec["offset"], p["rec_begin"] + c * CHUNK, side="left"))
        if i < len(names):
            # (two bytes in UTF-8, both above 0x80, in place of two ASCII characters; or a space in place of one)
            names[i] = ("é" + names[i][2:]) if c % 2 else (names[i][:1] + " " + names[i][2:])
            assert len(names[i].encode()) == len(("r%d" % i).encode())
            changed.append((c, i))
        c += 1
    return Fixture("refused_names", str(tmp / "refused_names.bam"), p["contigs"], p["refid"], p["reads"], names, changed=changed)


def _tuned_names(n, shift):
    """names of which the first few are longer than the plain ones by `shift` bytes in all (an l_read_name is at most 255)"""
    names = plain_names(n)
    i = 0
    while shift > 0:
        add = min(shift, 254 - len(names[i]))
        names[i] += "x" * add
        shift -= add
        i += 1
    return names, i


BORDER_DISTANCES = (0, 1, 32767, 32765, 32768 - 35, 32768 - 36)
TUNED_RECORD = 1500


def borders(tmp, d):
    """record TUNED_RECORD starts at lo + d of some chunk; d == 'end': the LAST record ends exactly on a border, so the grid's last
    chunk is a whole one"""
    p = _plain(tmp)
    rec, n = p["rec"], p["reads"].n_reads
    if d == "end":
        shift, j = (p["rec_begin"] - p["total"]) % CHUNK, n
    else:
        j = TUNED_RECORD
        shift = (p["rec_begin"] + d - int(rec["offset"][j])) % CHUNK
    names, used = _tuned_names(n, shift)
    assert used < TUNED_RECORD
    return Fixture("borders_%s" % d, str(tmp / ("borders_%s.bam" % d)), p["contigs"], p["refid"], p["reads"], names, record=j, d=d)


SHORT_TAILS = ("under36", 1, 2, 3)


def short_tail(tmp, k):
    """'under36': the last chunk holds 35 bytes; 1, 2, 3: exactly that many whole records, so the chain reaches the stream's end
    before four records"""
    p = _plain(tmp)
    rec, n = p["rec"], p["reads"].n_reads
    if k == "under36":
        shift = (p["rec_begin"] + 35 - p["total"]) % CHUNK
    else:
        shift = (p["rec_begin"] - int(rec["offset"][n - k])) % CHUNK
    names, used = _tuned_names(n, shift)
    assert used < n - 4
    return Fixture("short_tail_%s" % k, str(tmp / ("short_tail_%s.bam" % k)), p["contigs"], p["refid"], p["reads"], names, k=k)


def end_decoy(tmp):
    """The last record straddles the last border, which falls 50 bytes into its QUAL; the decoy written there has a block_size that
    reaches the end of the stream, so the scan of the last chunk takes it as a boundary (the `v == total` rule)."""
    p = _plain(tmp)
    rec, reads, n = p["rec"], p["reads"], p["reads"].n_reads
    at = qual_begin(rec, n - 1) + 50
    shift = (p["rec_begin"] - at) % CHUNK
    names, used = _tuned_names(n, shift)
    assert used < n - 4
    at += shift
    total = p["total"] + shift
    qual = reads.qual.copy()
    rec_shifted = dict(rec, offset=rec["offset"] + shift)
    _put(qual, reads, rec_shifted, n - 1, at, decoy_record(0, 5, total - at - 4))
    return Fixture("end_decoy", str(tmp / "end_decoy.bam"), p["contigs"], p["refid"], _with_qual(reads, qual), names, decoy=at)


LONG_AT = 1500
LONG_BASES = 100000


def long_record(tmp):
    """Among the short reads one of 100 000 bases: its record spans more than three chunks.  Four decoys stand behind every border
    its QUAL bytes cross: in the chunks that hold no record start, and in the one in which the record ends."""
    p = _plain(tmp)
    reads, refid = p["reads"], p["refid"]
    rng = np.random.default_rng(23)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, LONG_BASES)]
    z = lambda dt, v: np.array(v, dtype=dt)
    one = abi.ReadsSoA(pos=z(np.int32, [0]), mapq=z(np.uint8, [40]), flag=z(np.uint16, [0]), nm=z(np.int32, [3]), l_seq=z(np.int32, [LONG_BASES]),
                       seq_off=z(np.int64, [0, LONG_BASES // 2]), qual_off=z(np.int64, [0, LONG_BASES]), cigar_off=z(np.int64, [0, 1]),
                       seq4=(codes[0::2] << 4 | codes[1::2]).astype(np.uint8), qual=rng.integers(2, 42, LONG_BASES).astype(np.uint8),
                       cigar=z(np.uint32, [LONG_BASES << 4]))
    n = reads.n_reads
    merged = synth.concat_reads([synth.take_reads(reads, np.arange(LONG_AT)), one, synth.take_reads(reads, np.arange(LONG_AT, n))])
    refid = np.concatenate([refid[:LONG_AT], refid[LONG_AT:LONG_AT + 1], refid[LONG_AT:]])
    path = str(tmp / "long_layout.bam")
    bam.write_bam(path, list(p["contigs"].ids), [int(x) for x in p["contigs"].length], refid, merged)
    stream = inflate(path)
    rec, rec_begin = records(stream), header(stream)[0]
    q0, q1 = qual_begin(rec, LONG_AT), qual_begin(rec, LONG_AT) + int(rec["l_seq"][LONG_AT])
    qual = merged.qual.copy()
    placed = []
    c = (q0 - rec_begin) // CHUNK + 1
    while rec_begin + c * CHUNK + CHAIN * DECOY_BYTES <= q1:
        _put(qual, merged, rec, LONG_AT, rec_begin + c * CHUNK, decoy_records(CHAIN, unmapped=(2,)))
        placed.append((c, rec_begin + c * CHUNK))
        c += 1
    return Fixture("long_record", str(tmp / "long_record.bam"), p["contigs"], refid, _with_qual(merged, qual), None, placed=placed)


def everywhere(tmp):
    """Every read carries four decoys at QUAL offsets 0 and 160; names of differing lengths; about 1 % of the records unmapped.
    Whatever grid a route lays over the stream, many of its guesses are wrong."""
    contigs, refid, reads = plain_dataset()
    rng = np.random.default_rng(31)
    refid = refid.copy()
    refid[rng.choice(reads.n_reads, 30, replace=False)] = -1
    names = ["r%d%s" % (i, "x" * (i % 19)) for i in range(reads.n_reads)]
    qual = reads.qual.copy()
    fakes = [np.frombuffer(decoy_records(CHAIN, unmapped=u), np.uint8) for u in ((), (0,), (3,))]
    for i in range(reads.n_reads):
        q0 = int(reads.qual_off[i])
        for k, at in enumerate((0, 160)):
            f = fakes[(i + k) % 3]
            qual[q0 + at:q0 + at + f.size] = f
    return Fixture("everywhere", str(tmp / "everywhere.bam"), contigs, refid, _with_qual(reads, qual), names)
