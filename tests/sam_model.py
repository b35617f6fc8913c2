"""An independent pure-Python restatement of the SAM decode's field rules (include/midas_snps.h, midas_sam_load_device; DESIGN.md
section 14): SAM text in, the coordinate-sorted columns out.  It shares nothing with midas_amd (numpy only): the device decoder
(midas_amd/csrc/sam_scan.hip) and this file can only agree by both following the written rules.

    decode(data: bytes) -> (ref_names, ref_lens, cols)      cols: dict of numpy arrays, the columns of midas_bam_columns
    SamError(line, why)                                      the first bad line of the file (1-based), as the decoder reports it
"""
import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


class SamError(Exception):
    def __init__(self, line, why):
        Exception.__init__(self, "line %d: %s" % (line, why))
        self.line, self.why = line, why


def split_lines(data):
    """The file's lines without their ends: '\\n' ends a line, a '\\r' in front of it belongs to the end, the last line may lack
    its '\\n'."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def _decimal(field, top):
    if not field or not field.isdigit() or not all(48 <= c <= 57 for c in field):
        return None
    v = int(field)
    return v if v <= top else None


def parse_header(lines):
    """-> (names, lens, first record line index).  '@' lines come first; @SQ gives the references from SN: and LN:."""
    names, lens, k, seen = [], [], 0, set()
    while k < len(lines) and lines[k].startswith(b"@"):
        f = lines[k].split(b"\t")
        if f[0] == b"@SQ":
            sn = [x[3:] for x in f[1:] if x.startswith(b"SN:")]
            ln = [x[3:] for x in f[1:] if x.startswith(b"LN:")]
            length = _decimal(ln[0], INT32_MAX) if ln else None
            if not sn or not sn[0] or length is None:
                raise SamError(k + 1, "@SQ without SN or LN")
            name = sn[0].decode("latin-1")
            if name in seen:
                raise SamError(k + 1, "duplicate SN")
            seen.add(name)
            names.append(name)
            lens.append(length)
        k += 1
    if k < len(lines) and not names:
        raise SamError(k + 1, "record before @SQ")
    return names, lens, k


def parse_record(f, index_of, line):
    """The fields of one record line -> dict, or SamError naming `line`."""
    if len(f) < 11:
        raise SamError(line, "short line")
    flag = _decimal(f[1], 65535)
    if flag is None:
        raise SamError(line, "FLAG")
    if f[2] == b"*":
        refid = -1
    else:
        refid = index_of.get(f[2].decode("latin-1"), None)
        if refid is None:
            raise SamError(line, "RNAME")
    pos = _decimal(f[3], INT32_MAX)
    if pos is None:
        raise SamError(line, "POS")
    mapq = _decimal(f[4], 255)
    if mapq is None:
        raise SamError(line, "MAPQ")
    cigar = []
    if f[5] != b"*":
        digits = b""
        for c in f[5]:
            if 48 <= c <= 57:
                digits += bytes([c])
                continue
            if not digits or int(digits) >= 1 << 28:
                raise SamError(line, "CIGAR length")
            if chr(c) not in CIGAR_OPS:
                raise SamError(line, "CIGAR op")
            cigar.append(int(digits) << 4 | CIGAR_OPS.index(chr(c)))
            digits = b""
            if len(cigar) > 65535:
                raise SamError(line, "CIGAR ops")
        if digits:
            raise SamError(line, "CIGAR length")
    seq = b"" if f[9] == b"*" else f[9]
    codes = [NT16.index(chr(c).upper()) if chr(c).upper() in NT16 and c < 128 else 15 for c in seq]
    if f[10] == b"*":
        qual = [0xFF] * len(seq)
    else:
        if len(f[10]) != len(seq):
            raise SamError(line, "QUAL length")
        if any(c < 33 or c > 126 for c in f[10]):
            raise SamError(line, "QUAL character")
        qual = [c - 33 for c in f[10]]
    nm = -1
    for tag in f[11:]:
        if tag.startswith(b"NM:i:"):
            v = tag[5:]
            body = v[1:] if v[:1] in (b"+", b"-") else v
            if not body or not all(48 <= c <= 57 for c in body):
                raise SamError(line, "NM")
            nm = max(INT32_MIN, min(INT32_MAX, int(v)))
            break
    return dict(refid=refid, pos=pos - 1, mapq=mapq, flag=flag, nm=nm, cigar=cigar, codes=codes, qual=qual)


def decode(data):
    lines = split_lines(data)
    names, lens, first = parse_header(lines)
    index_of = {n: i for i, n in enumerate(names)}
    recs = []
    for k in range(first, len(lines)):
        r = parse_record(lines[k].split(b"\t"), index_of, k + 1)
        if r["refid"] >= 0:             # RNAME '*': dropped, as the BAM decode drops refID < 0
            recs.append(r)
    recs.sort(key=lambda r: (r["refid"], r["pos"] + 1))      # (stable: equal keys keep file order)
    return names, lens, columns(recs)


def columns(recs):
    n = len(recs)
    seq_off, qual_off, cigar_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    seq4, qual, cigar = [], [], []
    for i, r in enumerate(recs):
        c = r["codes"] + ([0] if len(r["codes"]) & 1 else [])
        seq4 += [c[j] << 4 | c[j + 1] for j in range(0, len(c), 2)]
        qual += r["qual"]
        cigar += r["cigar"]
        seq_off[i + 1], qual_off[i + 1], cigar_off[i + 1] = len(seq4), len(qual), len(cigar)
    return dict(refid=np.array([r["refid"] for r in recs], np.int32), pos=np.array([r["pos"] for r in recs], np.int32),
                mapq=np.array([r["mapq"] for r in recs], np.uint8), flag=np.array([r["flag"] for r in recs], np.uint16),
                nm=np.array([r["nm"] for r in recs], np.int32), l_seq=np.array([len(r["codes"]) for r in recs], np.int32),
                seq_off=seq_off, qual_off=qual_off, cigar_off=cigar_off, seq4=np.array(seq4, np.uint8), qual=np.array(qual, np.uint8),
                cigar=np.array(cigar, np.uint32))


COLUMNS = ("refid", "pos", "mapq", "flag", "nm", "l_seq", "seq_off", "qual_off", "cigar_off", "seq4", "qual", "cigar")


def reorder(cols, order):
    """The records of `cols` in the order `order` (indices), offsets and payloads rebuilt -- to bring two decodes of the same
    records into one tie order before comparing them."""
    order = np.asarray(order, np.int64)
    out = {k: cols[k][order] for k in ("refid", "pos", "mapq", "flag", "nm", "l_seq")}
    for off, data in (("seq_off", "seq4"), ("qual_off", "qual"), ("cigar_off", "cigar")):
        o = cols[off]
        lens = (o[1:] - o[:-1])[order]
        new = np.zeros(order.size + 1, np.int64)
        np.cumsum(lens, out=new[1:])
        ix = np.repeat(o[:-1][order] - new[:-1], lens) + np.arange(int(new[-1]))
        out[off], out[data] = new, cols[data][ix]
    return out


def sam_file_order(key_refid, key_pos, order):
    """Original indices of the records in the order a stable (refID, pos + 1) sort leaves the file whose line j holds record
    order[j]."""
    order = np.asarray(order, np.int64)
    key = np.asarray(key_refid)[order].astype(np.int64) << 32 | (np.asarray(key_pos)[order].astype(np.int64) + 1)
    return order[np.argsort(key, kind="stable")]


def assert_columns_equal(got, exp, what=""):
    for k in COLUMNS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k])), "%s: column %s differs" % (what, k)


def reads_columns(refid, reads):
    """The columns of a ReadsSoA-shaped object (attributes named like COLUMNS) plus its refID column, as a dict."""
    d = {k: np.asarray(getattr(reads, k)) for k in COLUMNS[1:]}
    d["refid"] = np.asarray(refid)
    return d
