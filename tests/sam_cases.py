"""Chosen lines for the device SAM decode (midas_amd/csrc/sam_scan.hip): every case puts one line, or a few, ON a rule of
sam_fields_kernel (pass 1) or a border of sam_payload_kernel (pass 2), the sort or the chunk loop, where synthetic samples never
land.  Plain data -- nothing here knows the decoder or tests/sam_model.py.  The expectations are literals, derived by hand from the
field rules of include/midas_snps.h (midas_sam_load_device) and DESIGN.md section 14, so that the model is a checked party too:
tests/test_sam_cases_host.py holds the model to them, tests/test_gpu_sam_lines.py holds the device to both.

A case is (name, head, lines, expect, refused): the '@' lines, the body lines as bytes WITH their line ends, and either `expect`
-- columns of the coordinate-sorted decode (sam_model.COLUMNS; the ones a case leaves out are the model's to judge) -- or
`refused` = (1-based file line, reason word).  The reason words are the keys of REASON_TEXT; its values are the texts of
sam_reason() in sam_scan.hip.

The groups, by the name's prefix, and the code each aims at:
  num/     sam_uint's clamp and its callers' bounds: FLAG / POS / MAPQ at their top and one beyond, 2^32 + k, 2^64 + k (a parser that
           wraps gives 0 or 1), forty leading zeros, signs, a blank, the empty field
  cigar/   pass 1's length loop (clamp at 2^28) and op walk; pass 2's backward digit loop, whose 32-bit multiplier wraps to 0 behind
           thirty leading zeros; 65535 ops against 65536
  stride/  pass 2's 64-byte strides over the CIGAR text: op letters at lanes 63 and 0, digit runs across 63|64 and 127|128 (a
           nine-digit one too), texts of 63 / 64 / 65 / 128 / 129 bytes, each of the nine letters at a stride's first and last lane
  rname/   the binary search over the sorted FNV-1a hashes and the byte compare down a run of EQUAL hashes (two pairs of colliding
           names, one of them at different lengths); names that are a prefix of, longer than, or one byte off an @SQ name
  nref/    the second radix sort's bits = ceil(log2(n_ref)) at 1, 2, 3, 256, 257, 65536, 65537 references (reference_count_case)
  ties/    equal (refID, POS) keys far apart in the file keep file order; POS 0, 1 and 2^31 - 1
  seq/     seq_code's two 64-bit constants over every byte value; the signed-char QUAL compare at 0x20, 0x7F, 0x80, 0xFF; l_seq
           around a wave's 64 lanes, odd ones with the pad nibble; '*' in SEQ and QUAL
  nm/      the NM loop: its exit behind a first value of -1, signs, saturation at both ends of int32, what is no integer, what is
           no NM:i: at all (a short last field, a trailing tab, nothing behind QUAL)
  shape/   ten and eleven fields, \\r\\n, the empty QNAME, the empty line, no '\\n' at the end of the file
  first/   the first reason of a line, the first bad line of a file
"""
import collections
import random

import numpy as np

Case = collections.namedtuple("Case", "name head lines expect refused")

# reason word -> what sam_reason() says (test_sam_cases_host.py compares the values with the source, one for one)
REASON_TEXT = {
    "short line": "fewer than 11 fields",
    "FLAG": "FLAG is not a decimal number in 0..65535",
    "RNAME": "RNAME is not among the @SQ lines",
    "POS": "POS is not a decimal number in 0..2147483647",
    "MAPQ": "MAPQ is not a decimal number in 0..255",
    "CIGAR op": "CIGAR holds an op that is not one of MIDNSHP=X",
    "CIGAR length": "a CIGAR op has no length, or one of 2^28 or more",
    "CIGAR ops": "CIGAR has more than 65535 ops",
    "QUAL length": "QUAL and SEQ differ in length",
    "QUAL character": "QUAL holds a character outside '!'..'~'",
    "NM": "NM:i: is not followed by an integer",
}

OPS = "MIDNSHP=X"


def fnv1a(name):
    """32-bit FNV-1a of a bytes object, as sam_scan.hip hashes an RNAME."""
    h = 2166136261
    for c in name:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


# ---- the header: sixteen references; two pairs of names whose hashes are equal among them -----------------------------------------
COLLIDING = ((b"bgatfnme", b"rhvmkwni"), (b"uwdrhfdq", b"gxtalwr"))      # 0x016c7abd twice; 0x009d3086 at lengths 8 and 7
NAMES = [b"c", b"d e", b"bgatfnme", b"contig_3", b"uwdrhfdq", b"NC_000913.3", b"rhvmkwni", b"scaffold|7", b"gxtalwr", b"k9",
         b"k10", b"ctg.11", b"ctg.12", b"Z", b"bgatfnmeY", b"k15"]
LENS = [200000, 5000] + [1000 + k for k in range(2, 16)]
HEAD = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(NAMES, LENS))
FIRST = 18                                                               # the file line of the first body line under HEAD


def line(qname=b"q", flag=b"0", rname=b"c", pos=b"7", mapq=b"40", cigar=b"4M", seq=b"ACGT", qual=b"IIII", tags=b"\tNM:i:0", end=b"\n"):
    """One record line; every field as the bytes that go into the file, `tags` with the tab in front of each."""
    return b"\t".join([qname, flag, rname, pos, mapq, cigar, b"*", b"0", b"0", seq, qual]) + tags + end


GOOD = line()


def good_columns(**over):
    """What GOOD decodes to, by the rules: refID of 'c' 0, POS 7 -> 6, 'ACGT' -> nibbles 1 2 4 8, 'I' - 33 = 40, 4M -> 4 << 4 | 0."""
    cols = dict(refid=[0], pos=[6], mapq=[40], flag=[0], nm=[0], l_seq=[4], seq_off=[0, 2], qual_off=[0, 4], cigar_off=[0, 1],
                seq4=[0x12, 0x48], qual=[40, 40, 40, 40], cigar=[0x40])
    cols.update(over)
    return cols


def accept(name, lines, expect, head=HEAD):
    return Case(name, head, [lines] if isinstance(lines, bytes) else list(lines), expect, None)


def refuse(name, bad, why, before=1, after=1):
    """`bad` behind `before` good lines and in front of `after` more: the file line of `bad` is the one refused."""
    assert why in REASON_TEXT
    return Case(name, HEAD, [GOOD] * before + [bad] + [GOOD] * after, None, (FIRST + before, why))


def data(case):
    return case.head + b"".join(case.lines)


def assert_literals(got, case):
    """The columns the case wrote down, value for value (got: a dict of arrays, as sam_model.decode and reads_columns give)."""
    for k, want in case.expect.items():
        have = np.asarray(got[k])
        assert have.size == len(want) and np.array_equal(have.astype(np.int64), np.asarray(want, np.int64)), "%s: column %s is not the literal" % (case.name, k)


# ---- num/ ------------------------------------------------------------------------------------------------------------------------
def number_cases():
    out = []
    for field, top in (("flag", 65535), ("pos", 2147483647), ("mapq", 255)):
        word = field.upper()
        col = (lambda v: [v - 1]) if field == "pos" else (lambda v: [v])      # POS is 0-based in the column
        out.append(accept("num/%s/0%d" % (field, top), line(**{field: b"0%d" % top}), good_columns(**{field: col(top)})))
        out.append(accept("num/%s/forty zeros then 16" % field, line(**{field: b"0" * 40 + b"16"}), good_columns(**{field: col(16)})))
        for k, bad in enumerate((top + 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64, 2 ** 64 + 1)):
            out.append(refuse("num/%s/%d" % (field, bad), line(**{field: b"%d" % bad}), word, before=k % 3))
        for bad in (b"+16", b"-0", b"1 6", b""):
            out.append(refuse("num/%s/'%s'" % (field, bad.decode()), line(**{field: bad}), word))
    return out


# ---- cigar/ ----------------------------------------------------------------------------------------------------------------------
def star(cigar, **kw):
    """A line whose CIGAR is all there is to it: SEQ and QUAL '*'."""
    return line(cigar=cigar, seq=b"*", qual=b"*", **kw)


def star_columns(words, **over):
    return good_columns(l_seq=[0], seq_off=[0, 0], qual_off=[0, 0], seq4=[], qual=[], cigar_off=[0, len(words)], cigar=list(words), **over)


def cigar_cases():
    out = [
        accept("cigar/268435455M", star(b"268435455M"), star_columns([268435455 << 4 | 0])),        # 0xFFFFFFF0: the largest word
        accept("cigar/thirty zeros then 7M", star(b"0" * 30 + b"7M"), star_columns([7 << 4])),
        accept("cigar/0M", star(b"0M"), star_columns([0])),
        accept("cigar/0000000000000I", star(b"0" * 13 + b"I"), star_columns([1])),
        accept("cigar/empty", star(b""), star_columns([])),                                        # an empty field holds no items
        accept("cigar/star", star(b"*"), star_columns([])),
    ]
    # ('*' and '-' are no digits and stand where a length must: the length is missing)
    for bad in (b"268435456M", b"4294967297M", b"18446744073709551617M", b"M", b"4", b"4M5", b"4MM", b"3M*", b"-4M"):
        out.append(refuse("cigar/%s" % bad.decode(), star(bad), "CIGAR length"))
    for bad in (b"2M2B", b"4m", b"4M1 "):
        out.append(refuse("cigar/'%s'" % bad.decode(), star(bad), "CIGAR op", before=2))
    out.append(accept("cigar/65535 ops", star(b"1M" * 65535), star_columns([0x10] * 65535)))
    out.append(refuse("cigar/65536 ops", star(b"1M" * 65536), "CIGAR ops"))
    return out


# ---- stride/ ---------------------------------------------------------------------------------------------------------------------
def cigar_text(pairs):
    return "".join("%d%s" % p for p in pairs).encode()


def cigar_words(pairs):
    return [l << 4 | OPS.index(op) for l, op in pairs]


def pairs_with_ops_at(length, at):
    """(length, op) pairs whose text is `length` bytes long and has the op letters of `at` = {offset: letter} where it says.  The
    digits in front of each letter fill the gap to the letter before; a gap of more than nine is cut by two-digit ops."""
    pairs, pos, fill = [], 0, 0
    at = dict(at)
    assert length - 1 in at, "a CIGAR ends in an op letter"
    for off in sorted(at):
        gap = off - pos
        assert gap >= 1, "two letters side by side"
        while gap > 9:
            pairs.append((10 + fill % 90, OPS[fill % 9]))
            fill, gap = fill + 1, gap - 3
        digits = "".join("123456789"[(off + i) % 9] for i in range(gap))
        if gap == 9:
            digits = "1" + digits[1:]                       # nine digits stay under 2^28 = 268435456
        pairs.append((int(digits), at[off]))
        pos = off + 1
    assert len(cigar_text(pairs)) == length
    return pairs


STRIDE_PAIRS = {
    "stride/mixed widths": [(7, "M"), (12, "I"), (345, "D"), (6789, "N"), (12345, "S"), (678901, "H"), (2345678, "P"), (89012345, "="), (123456789, "X")],
    "stride/63 bytes": pairs_with_ops_at(63, {62: "M"}),
    "stride/64 bytes, a letter at 63": pairs_with_ops_at(64, {63: "I"}),
    "stride/65 bytes, a letter at 64": pairs_with_ops_at(65, {60: "S", 64: "D"}),
    "stride/128 bytes, letters at 63 and 127": pairs_with_ops_at(128, {63: "N", 127: "S"}),
    "stride/129 bytes, letters at 64 and 128": pairs_with_ops_at(129, {64: "H", 128: "P"}),
    "stride/digits across 63|64 and 127|128": pairs_with_ops_at(135, {61: "=", 66: "X", 125: "M", 131: "I", 134: "D"}),
    "stride/nine digits across 63|64": pairs_with_ops_at(72, {58: "N", 68: "S", 71: "M"}),
    "stride/nine digits end at 63": pairs_with_ops_at(70, {54: "H", 64: "P", 69: "="}),
    "stride/every letter at a last lane": pairs_with_ops_at(64 * 9, {63 + 64 * j: OPS[j] for j in range(9)}),
    "stride/every letter at a first lane": pairs_with_ops_at(64 * 9 + 1, {64 + 64 * j: OPS[j] for j in range(9)}),
}


def stride_cases():
    return [accept(name, star(cigar_text(pairs), pos=b"%d" % (100 + k)), star_columns(cigar_words(pairs), pos=[99 + k]))
            for k, (name, pairs) in enumerate(STRIDE_PAIRS.items())]


# ---- rname/ ----------------------------------------------------------------------------------------------------------------------
def rname_cases():
    on = [(b"rhvmkwni", 6, 11), (b"gxtalwr", 8, 12), (b"bgatfnme", 2, 13), (b"uwdrhfdq", 4, 14), (b"bgatfnmeY", 14, 15), (b"k15", 15, 16)]
    lines = [line(rname=n, mapq=b"%d" % q) for n, _, q in on]
    lines.insert(3, line(rname=b"*", flag=b"4", mapq=b"99"))           # dropped, not refused
    by_ref = sorted((r, q) for _, r, q in on)
    n = len(on)
    out = [accept("rname/each colliding name its own refID", lines,
                  dict(refid=[r for r, _ in by_ref], mapq=[q for _, q in by_ref], pos=[6] * n, l_seq=[4] * n, nm=[0] * n, flag=[0] * n,
                       seq4=[0x12, 0x48] * n, qual=[40] * (4 * n), cigar=[0x40] * n, cigar_off=list(range(n + 1)))),
           accept("rname/star alone is dropped", [line(rname=b"*", flag=b"4")] * 3,
                  dict(refid=[], pos=[], mapq=[], flag=[], nm=[], l_seq=[], seq_off=[0], qual_off=[0], cigar_off=[0], seq4=[], qual=[], cigar=[]))]
    for bad in (b"bgatfnm", b"bgatfnmeX", b"", b"rhvmkwnj", b"gxtalwrq", b"**", b"C"):
        out.append(refuse("rname/'%s'" % bad.decode(), line(rname=bad), "RNAME", before=len(bad) % 3))
    return out


# ---- nref/ -----------------------------------------------------------------------------------------------------------------------
REF_COUNTS = (1, 2, 3, 256, 257, 65536, 65537)


def reference_count_case(n_ref):
    """A header of n_ref references; three records on each of refIDs 0, 1, 255, 256, 65535, 65536 and n_ref - 1 that exist, written
    in DESCENDING refID order, on each POS 9 (MAPQ 1), POS 3 (MAPQ 2), POS 9 (MAPQ 3).  Ascending refID, then POS, then file order."""
    head = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:r%d\tLN:%d\n" % (k, 1000 + k % 7) for k in range(n_ref))
    ids = sorted({r for r in (0, 1, 255, 256, 65535, 65536, n_ref - 1) if r < n_ref})
    lines = [line(rname=b"r%d" % r, pos=p, mapq=q) for r in reversed(ids) for p, q in ((b"9", b"1"), (b"3", b"2"), (b"9", b"3"))]
    expect = dict(refid=[r for r in ids for _ in range(3)], pos=[2, 8, 8] * len(ids), mapq=[2, 1, 3] * len(ids))
    return accept("nref/%d" % n_ref, lines, expect, head=head)


# ---- ties/ -----------------------------------------------------------------------------------------------------------------------
def tie_cases():
    spec = [                                   # (rname, POS, MAPQ) line by line; equal keys are told apart by MAPQ
        (b"c", 500, 1), (b"d e", 1, 2), (b"c", 0, 3), (b"*", 500, 99), (b"c", 500, 4), (b"c", 2147483647, 5), (b"c", 1, 6),
        (b"d e", 0, 7), (b"c", 500, 8), (b"c", 0, 9), (b"*", 0, 98), (b"c", 2147483647, 10), (b"d e", 1, 11), (b"c", 1, 12),
        (b"c", 499, 13), (b"c", 500, 14), (b"c", 501, 15), (b"d e", 0, 16),
    ]
    lines = [line(rname=r, pos=b"%d" % p, mapq=b"%d" % q) for r, p, q in spec]
    expect = dict(                             # c: POS 0, 0, 1, 1, 499, 500 x 4, 501, 2^31 - 1 x 2; then d e: POS 0, 0, 1, 1
        refid=[0] * 12 + [1] * 4,
        pos=[-1, -1, 0, 0, 498, 499, 499, 499, 499, 500, 2147483646, 2147483646, -1, -1, 0, 0],
        mapq=[3, 9, 6, 12, 13, 1, 4, 8, 14, 15, 5, 10, 7, 16, 2, 11])
    return [accept("ties/equal keys keep file order", lines, expect)]


# ---- seq/ ------------------------------------------------------------------------------------------------------------------------
# byte -> 4-bit code, written out: '=' 0, "ACMGRSVTWYHKDBN" 1..15 in either case, every other byte 15
SEQ_CODE = [
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,      # 0x00
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,      # 0x10
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,      # 0x20
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 0, 15, 15,       # 0x30  '=' is 0x3D
    15, 1, 14, 2, 13, 15, 15, 4, 11, 15, 15, 12, 15, 3, 15, 15,          # 0x40  @ A B C D E F G H I J K L M N O
    15, 15, 5, 6, 8, 15, 7, 9, 15, 10, 15, 15, 15, 15, 15, 15,           # 0x50  P Q R S T U V W X Y Z
    15, 1, 14, 2, 13, 15, 15, 4, 11, 15, 15, 12, 15, 3, 15, 15,          # 0x60  ` a b c d e f g h i j k l m n o
    15, 15, 5, 6, 8, 15, 7, 9, 15, 10, 15, 15, 15, 15, 15, 15,           # 0x70  p q r s t u v w x y z
] + [15] * 128                                                           # 0x80..0xFF
ALL_BYTES_SEQ = bytes(b for b in range(256) if b not in (9, 10))         # 254 bytes; '\r' (13) is not last


def pack_codes(codes):
    """4-bit codes two a byte, the first in the high nibble; an odd count leaves the last low nibble 0."""
    codes = list(codes)
    codes += [0] * (len(codes) & 1)
    return [codes[j] << 4 | codes[j + 1] for j in range(0, len(codes), 2)]


def cycle(alphabet, n, start=0):
    return bytes(alphabet[(start + i) % len(alphabet)] for i in range(n))


QUAL_ALPHABET = bytes(range(33, 127))                                    # '!'..'~'


def seq_columns(seq, qual, **over):
    l = len(seq)
    return good_columns(l_seq=[l], seq_off=[0, (l + 1) // 2], qual_off=[0, l], seq4=pack_codes(SEQ_CODE[b] for b in seq),
                        qual=[0xFF] * l if qual == b"*" else [q - 33 for q in qual], cigar_off=[0, 0], cigar=[], **over)


def seq_cases():
    q254 = cycle(QUAL_ALPHABET, 254)
    out = [accept("seq/every byte value", line(cigar=b"*", seq=ALL_BYTES_SEQ, qual=q254), seq_columns(ALL_BYTES_SEQ, q254))]
    for k, l in enumerate((1, 2, 63, 64, 65, 127, 128, 129)):
        seq, qual = cycle(b"ACGTNacgtn=MRSVWYHKDBx", l, start=k), cycle(QUAL_ALPHABET, l, start=11 * k)
        out.append(accept("seq/l_seq %d" % l, line(cigar=b"*", seq=seq, qual=qual, pos=b"%d" % (300 + l)), seq_columns(seq, qual, pos=[299 + l])))
    out += [
        accept("seq/A with QUAL star", line(cigar=b"*", seq=b"A", qual=b"*"), seq_columns(b"A", b"*")),
        accept("seq/star with QUAL star", line(cigar=b"*", seq=b"*", qual=b"*"), seq_columns(b"", b"")),
        accept("seq/star with the empty QUAL", line(cigar=b"*", seq=b"*", qual=b""), seq_columns(b"", b"")),
        accept("seq/empty with the empty QUAL", line(cigar=b"*", seq=b"", qual=b""), seq_columns(b"", b"")),
        accept("seq/QUAL of the two border characters", line(cigar=b"*", seq=b"AC", qual=b"!~"), seq_columns(b"AC", b"!~")),
        accept("seq/a star inside SEQ is a base", line(cigar=b"*", seq=b"A*", qual=b"**"), seq_columns(b"A*", b"**")),
    ]
    for q in (0x20, 0x7F, 0x80, 0xFF):
        for where, i in (("first", 0), ("middle", 3), ("last", 6)):
            qual = bytearray(b"IIIIIII")
            qual[i] = q
            out.append(refuse("seq/QUAL 0x%02X %s" % (q, where), line(cigar=b"7M", seq=b"ACGTACG", qual=bytes(qual)), "QUAL character", before=i % 2))
    for seq, qual in ((b"*", b"I"), (b"ACGT", b"IIIII"), (b"ACGT", b"III"), (b"ACGT", b""), (b"A", b"*!")):
        out.append(refuse("seq/SEQ '%s' QUAL '%s'" % (seq.decode(), qual.decode()), line(seq=seq, qual=qual), "QUAL length"))
    return out


# ---- nm/ -------------------------------------------------------------------------------------------------------------------------
def nm_cases():
    top, low = 2147483647, -2147483648
    given = [
        (b"\tNM:i:-1\tNM:i:7", -1), (b"\tNM:i:+5", 5), (b"\tNM:i:-0", 0), (b"\tNM:i:+0", 0), (b"\tNM:i:0000000000000000000000012", 12),
        (b"\tNM:i:2147483647", top), (b"\tNM:i:2147483648", top), (b"\tNM:i:99999999999999999999", top), (b"\tNM:i:4294967301", top),
        (b"\tNM:i:18446744073709551621", top),
        (b"\tNM:i:-2147483648", low), (b"\tNM:i:-2147483649", low), (b"\tNM:i:-99999999999999999999", low), (b"\tNM:i:-4294967301", low),
        (b"\tXS:A:+\tNM:Z:3\tXX:i:5\tNM:i:-7\tNM:i:2", -7),
        # absent: -1
        (b"\tNM:Z:5", -1), (b"\tXS:i:1\tNM:i", -1), (b"\tNM:i", -1), (b"\tXX:Z:NM:i:5", -1), (b"\t", -1), (b"", -1), (b"\tnm:i:5", -1),
        (b"\tNM:I:5", -1), (b"\tXS:i:1\t", -1), (b"\t\tNM:i:4", 4),
    ]
    out = [accept("nm/'%s'" % tags.decode().replace("\t", " "), line(tags=tags), good_columns(nm=[nm])) for tags, nm in given]
    for bad in (b"\tNM:i:", b"\tNM:i:-", b"\tNM:i:5x", b"\tNM:i: 5", b"\tNM:i:+", b"\tNM:i:--5", b"\tXS:i:1\tNM:i:\tNM:i:5", b"\tNM:i:5 "):
        out.append(refuse("nm/'%s'" % bad.decode().replace("\t", " "), line(tags=bad), "NM", before=len(bad) % 3))
    return out


# ---- shape/ ----------------------------------------------------------------------------------------------------------------------
def shape_cases():
    ten = b"\t".join(GOOD.split(b"\t")[:10]) + b"\n"
    return [
        refuse("shape/ten fields", ten, "short line"),
        refuse("shape/ten fields and a tab behind them is eleven, the last empty", ten[:-1] + b"\t\n", "QUAL length"),
        refuse("shape/an empty line between two good ones", b"\n", "short line"),
        refuse("shape/a line of a carriage return alone", b"\r\n", "short line"),
        refuse("shape/one field", b"q\n", "short line", before=0),
        accept("shape/eleven fields and a carriage return", line(tags=b"", end=b"\r\n"), good_columns(nm=[-1])),
        accept("shape/tags and a carriage return", line(tags=b"\tNM:i:3", end=b"\r\n"), good_columns(nm=[3])),
        accept("shape/the empty QNAME", line(qname=b""), good_columns()),
        accept("shape/no newline at the end of the file", [GOOD, line(mapq=b"41", end=b"")],
               dict(refid=[0, 0], pos=[6, 6], mapq=[40, 41], nm=[0, 0], l_seq=[4, 4], cigar=[0x40, 0x40])),
        accept("shape/no newline behind eleven fields", line(tags=b"", end=b""), good_columns(nm=[-1])),
        # (the header ends at the first line that does not begin with '@': behind it such a line is a record)
        accept("shape/a QNAME that begins with @ behind the first record", [GOOD, line(qname=b"@SQ", mapq=b"41")],
               dict(refid=[0, 0], pos=[6, 6], mapq=[40, 41], nm=[0, 0], l_seq=[4, 4], cigar=[0x40, 0x40])),
    ]


# ---- first/ ----------------------------------------------------------------------------------------------------------------------
def first_reason_cases():
    two = line(flag=b"x", cigar=b"4B")                                   # FLAG is looked at before the CIGAR
    late = line(tags=b"\tNM:i:x")                                        # NM is the last rule looked at ...
    early = line(flag=b"65536")                                          # ... FLAG the second, on a LATER line
    return [
        Case("first/a bad FLAG and a bad CIGAR on one line", HEAD, [GOOD, GOOD, two, GOOD], None, (FIRST + 2, "FLAG")),
        Case("first/every rule broken on one line", HEAD, [GOOD, line(flag=b"-1", rname=b"nope", pos=b"x", mapq=b"256", cigar=b"M", qual=b"I I", tags=b"\tNM:i:")],
             None, (FIRST + 1, "FLAG")),
        Case("first/the earlier line wins whatever its reason", HEAD, [GOOD] * 3 + [late] + [GOOD] * 5 + [early, GOOD], None, (FIRST + 3, "NM")),
    ]


def cases():
    """Every case but the reference counts (reference_count_case builds those: their headers are large)."""
    return (number_cases() + cigar_cases() + stride_cases() + rname_cases() + tie_cases() + seq_cases() + nm_cases() + shape_cases()
            + first_reason_cases())


def accepted():
    return [c for c in cases() if c.refused is None]


def refused():
    return [c for c in cases() if c.refused is not None]


def accepted_file():
    """One SAM under HEAD holding every accepted line above, in a fixed shuffled order (a line without its end gets one)."""
    lines = [l if l.endswith(b"\n") else l + b"\n" for c in accepted() if c.head == HEAD for l in c.lines]
    random.Random(14).shuffle(lines)
    assert not lines[0].startswith(b"@")            # (that line would belong to the header)
    return HEAD + b"".join(lines)


# ---- the chunk sweep's file --------------------------------------------------------------------------------------------------------
def sweep_file(eol):
    """A dozen short lines, about 600 bytes; -> (data, offsets of the line starts in the BODY, one more entry for its end)."""
    spec = [(b"c", 31, b"3M1I", b"ACGT", b"IJKL", b"\tNM:i:1"), (b"d e", 9, b"2S2M", b"acgt", b"!~5I", b"\tXS:i:4\tNM:i:2"), (b"k9", 5, b"*", b"*", b"*", b""),
            (b"c", 31, b"5M", b"NACGT", b"IIIII", b"\tNM:i:3"), (b"*", 0, b"*", b"ACG", b"III", b""), (b"Z", 77, b"1M", b"A", b"*", b"\tNM:i:4"),
            (b"c", 2, b"10M", b"ACGTACGTAC", b"0123456789", b"\tNM:i:-5"), (b"rhvmkwni", 1, b"3M", b"TTT", b"ABC", b"\tNM:i:6"),
            (b"bgatfnme", 1, b"3M", b"GGG", b"CBA", b"\tNM:i:7"), (b"c", 31, b"2M", b"=R", b"##", b"\tNM:i:8"), (b"d e", 9, b"1X", b"y", b"9", b"\tNM:Z:9"),
            (b"c", 1, b"4=", b"ACGT", b"IIII", b"\tNM:i:10")]
    lines = [line(qname=b"read_%02d:lane1" % k, rname=r, pos=b"%d" % p, mapq=b"%d" % (k + 1), cigar=c, seq=s, qual=q, tags=t, end=eol)
             for k, (r, p, c, s, q, t) in enumerate(spec)]
    starts = [0]
    for l in lines:
        starts.append(starts[-1] + len(l))
    return HEAD + b"".join(lines), starts
