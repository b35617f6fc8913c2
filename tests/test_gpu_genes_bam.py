"""`run_midas.py genes --device_inflate` on the GPU: genes/temp/pangenomes.bam counted in one pass (midas_genes_count_bam: blocks
inflated, records walked, every read's 8-byte fact made from its record where it lies -- bam_genes_facts_kernel) against today's
host route (abi.read_bam(path) + ctx.genes_count: the host's threads decode, pack_records makes the facts) and against
oracle/genes_oracle.py.  Every comparison is exact: counts as integers, depths by their bytes, statuses with the index of the
first offending read among the kept records.  The BAMs with chosen bytes (name lengths, aux blocks, refIDs) are written here with
struct + zlib; the others by the project's own writer."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from midas_amd import abi, synth
from oracle import genes_oracle as go
from tests.test_gpu_genes import GENES_ARGS, _oracle, _oracle_records
from tests.test_gpu_genes_sam import EDGE_THRESHOLDS, MAX_L, PERMISSIVE, THRESHOLD_SETS, _ZERO, _edge_cases, _make_edge, _thr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


# ---- the two routes -----------------------------------------------------------------------------------------------------------------

def _host(ctx, path, args, lengths):
    """Today's route: the host's threads inflate, walk and cut, pack_records makes the facts."""
    _, _, refid, reads = abi.read_bam(path)
    return ctx.genes_count(_thr(args), reads, refid, lengths)[:3]


def _device(ctx, path, args, lengths):
    h = abi.open_bam_device(path, ctx)
    try:
        return ctx.genes_count_bam(_thr(args), h, lengths)[:3]
    finally:
        h.close()


def _same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()


def _both_raise(ctx, path, args, lengths):
    with pytest.raises(abi.MidasSnpsError) as eh:
        _host(ctx, path, args, lengths)
    with pytest.raises(abi.MidasSnpsError) as ed:
        _device(ctx, path, args, lengths)
    return eh.value, ed.value


# ---- a BAM byte by byte (SAMv1 4.1, 4.2) --------------------------------------------------------------------------------------------

def _aux(tag, typ, val):
    b = tag.encode() + typ.encode()
    if typ in "cCsSiI":
        return b + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[typ], val)
    if typ == "A":
        return b + val.encode()
    if typ == "Z":
        return b + val.encode() + b"\0"
    sub, vals = val             # 'B'
    return b + sub.encode() + struct.pack("<i", len(vals)) + b"".join(struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub], v) for v in vals)


def _record(refid, name, quals, aux=b"", cigar=None, mapq=30, l_seq=None):
    """One alignment record; quals: the QUAL bytes (l_seq of them unless l_seq says otherwise); cigar: [(length, op)], default <l>M."""
    l = len(quals) if l_seq is None else l_seq
    cigar = [(l, 0)] if cigar is None else cigar
    name = name.encode() + b"\0"
    body = struct.pack("<iiBBHHHIiii", refid, 0, len(name), mapq, 0, len(cigar), 0, l, -1, -1, 0) + name
    body += b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + bytes([0x12] * ((l + 1) // 2)) + bytes(quals) + aux
    return struct.pack("<I", len(body)) + body


def _bgzf(data, block=0xff00):
    out = b""
    for o in range(0, len(data), block):
        piece = data[o:o + block]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(piece) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp
        out += struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece))
    return out + EOF_BLOCK


def _write(path, refs, records, block=0xff00):
    """-> the offset of every record in the inflated stream, and the stream's size."""
    text = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in refs)
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    head += b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in refs)
    at, offs = len(head), []
    for r in records:
        offs.append(at)
        at += len(r)
    with open(path, "wb") as f:
        f.write(_bgzf(head + b"".join(records), block))
    return offs, at


def _refs(n):
    return [("g%d" % i, 1000 + 7 * i) for i in range(n)]


def _expected(facts, lengths, args):
    """[(gene, aligned length, l_seq, nm, quals, mapq)] in file order -> the three arrays by the reference's own expressions."""
    n = len(lengths)
    aligned, mapped, depth = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
    for g, al, l, nm, q, mq in facts:
        aligned[g] += 1
        assert int(np.mean(q) < args['readq']) == int(sum(q) // l < args['readq'])        # (floor(sum(q) / l): the record's field)
        if go.keep_read(al, l, nm, q, mq, args['mapid'], args['readq'], args['mapq'], args['aln_cov']):
            mapped[g] += 1
            depth[g] += al / float(lengths[g])
    return aligned, mapped, depth


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------

def _dropped_by(recs, args):
    """How many reads each of keep_read's four tests drops, in its order."""
    out = [0, 0, 0, 0]
    for _, al, l, nm, q, mq in recs:
        if 100 * (al - nm) / float(al) < args['mapid']: out[0] += 1
        elif np.mean(q) < args['readq']: out[1] += 1
        elif mq < args['mapq']: out[2] += 1
        elif al / float(l) < args['aln_cov']: out[3] += 1
    return out


@pytest.fixture(scope="module")
def parity(tmp_path_factory):
    # (silent_fraction=0.0: every one of the 6000 reads aligns, so the file holds 6000 records)
    ds = synth.make_pangenome_dataset(n_species=3, genes_per_species=80, n_reads=6000, seed=101, silent_fraction=0.0)
    lengths = [len(s) for s in ds['gene_seq']]
    path = str(tmp_path_factory.mktemp("parity") / "pangenomes.bam")
    abi.write_bam(path, ds['gene_ids'], lengths, ds['refid'], ds['reads'])
    # the dataset's condition, by the oracle alone: every set maps something, every filter drops something under some set
    recs = _oracle_records(ds['reads'], ds['refid'])
    drops = [_dropped_by(recs, a) for a in THRESHOLD_SETS]
    assert all(any(d[k] > 0 for d in drops) for k in range(4)), drops
    return ds, lengths, path, [_oracle(ds, a) for a in THRESHOLD_SETS]


@pytest.mark.parametrize("k", range(len(THRESHOLD_SETS)))
def test_one_pass_the_oracle_and_the_host_route_agree(ctx, parity, k):
    ds, lengths, path, oracles = parity
    args = THRESHOLD_SETS[k]
    exp_aligned, exp_mapped, exp_depth = oracles[k][:3]
    assert sum(exp_mapped) > 0
    host = _host(ctx, path, args, lengths)
    assert host[0].tolist() == exp_aligned and host[1].tolist() == exp_mapped and host[2].tobytes() == np.array(exp_depth, np.float64).tobytes()
    h = abi.open_bam_device(path, ctx)
    assert h.ref_names == list(ds['gene_ids']) and h.ref_lengths == lengths
    got = ctx.genes_count_bam(_thr(args), h, lengths)
    assert _same(got, host) and got[3] > 0
    laps, stats = ctx.genes_count_bam_timing()
    assert list(laps) == list(abi.GENES_BAM_PHASES) and all(v > 0 for v in laps.values()), laps
    assert stats['records'] == 6000 == int(ds['refid'].size) and stats['dropped'] == 0 and stats['chunks'] > 1 and stats['blocks'] > 12, stats
    assert stats['inflated_bytes'] > 24 * 32768
    again = ctx.genes_count_bam(_thr(args), h, lengths)           # the handle is left as it was; no state is carried
    assert _same(again, got)
    h.close()


def test_a_handle_of_midas_bam_open_device_is_taken_too(ctx, parity):
    """The entry takes any open handle on which nothing is loaded; open_bam_device only picks the one that is cheapest to open."""
    ds, lengths, path, oracles = parity
    lib = abi.load_library()
    h, err = C.c_void_p(), C.create_string_buffer(256)
    assert lib.midas_bam_open_device(path.encode(), ctx._h, C.byref(h), err) == 0, err.value
    handle = abi.BamDeviceHandle(lib, h, path)
    got = ctx.genes_count_bam(_thr(GENES_ARGS), handle, lengths)
    assert got[0].tolist() == oracles[0][0] and got[1].tolist() == oracles[0][1] and got[2].tobytes() == np.array(oracles[0][2], np.float64).tobytes()
    with pytest.raises(abi.MidasSnpsError) as ei:            # as many gene lengths as the header has references
        ctx.genes_count_bam(_thr(GENES_ARGS), handle, lengths[:-1])
    assert ei.value.status == abi.ERR_INVALID_ARG
    handle.close()


# ---- 2. every alignment of a record and of its QUAL run -----------------------------------------------------------------------------

L_SEQS = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024)


def _alignment_file(path, last_aux=None):
    rng = np.random.default_rng(12)
    records, facts = [], []
    cases = [(nl, l) for nl in range(1, 17) for l in L_SEQS]
    for g, (nl, l) in enumerate(cases):
        q = [int(x) for x in rng.integers(0, 94, l)]
        nm, mapq = int(rng.integers(0, 4)), int(rng.integers(0, 60))
        aux = _aux("NM", "C", nm)
        if g == len(cases) - 1 and last_aux is not None:
            aux = last_aux
        records.append(_record(g, "abcdefghijklmnop"[:nl], q, aux, mapq=mapq))
        facts.append((g, l, l, nm, q, mapq))
    refs = _refs(len(cases))
    offs, total = _write(path, refs, records)
    starts = [o + 36 + nl + 1 + 4 + (l + 1) // 2 for o, (nl, l) in zip(offs, cases)]
    ends = [s + l for s, (_, l) in zip(starts, cases)]
    return refs, facts, starts, ends, total


def test_every_alignment_of_a_record_and_of_its_qual_run(ctx, tmp_path):
    path = str(tmp_path / "align.bam")
    refs, facts, starts, ends, _ = _alignment_file(path)
    assert len(facts) == 192
    assert {s % 16 for s in starts} == set(range(16)) and {e % 16 for e in ends} == set(range(16))
    lengths = [l for _, l in refs]
    seen = set()
    for args in EDGE_THRESHOLDS:
        exp = _expected(facts, lengths, args)
        host, got = _host(ctx, path, args, lengths), _device(ctx, path, args, lengths)
        assert _same(host, exp), args
        assert _same(got, host), args
        seen.add(int(got[1].sum()))
    assert len(seen) >= 3          # (the thresholds cut through the set)


# ---- 3. the stream's end ----------------------------------------------------------------------------------------------------------

def test_a_qual_run_that_ends_the_stream(ctx, tmp_path):
    path = str(tmp_path / "end.bam")
    refs, facts, starts, ends, total = _alignment_file(path, last_aux=b"")
    assert ends[-1] == total                       # nothing lies behind the last quality byte
    lengths = [l for _, l in refs]
    eh, ed = _both_raise(ctx, path, PERMISSIVE, lengths)
    assert (ed.status, ed.read_index) == (eh.status, eh.read_index) == (abi.ERR_READ_NO_NM, 191)
    assert ed.message == eh.message
    refs, facts, starts, ends, total = _alignment_file(path, last_aux=_aux("NM", "C", 2))
    assert ends[-1] + 4 == total
    facts[-1] = facts[-1][:3] + (2,) + facts[-1][4:]
    for args in (PERMISSIVE, GENES_ARGS):
        host = _host(ctx, path, args, lengths)
        assert _same(host, _expected(facts, lengths, args)) and _same(_device(ctx, path, args, lengths), host)


# ---- 4. NM ------------------------------------------------------------------------------------------------------------------------

def _nm_file(path, extra=()):
    rng = np.random.default_rng(3)
    md, yt = _aux("MD", "Z", "37A12^CG40"), _aux("YT", "Z", "UU")
    variants = [_aux("NM", t, v) for t, v in (("c", 100), ("C", 200), ("s", 300), ("S", 40000), ("i", 50000), ("I", 60000))]
    # (each needs its width: 200 is negative as a 'c', 300 is 44 in eight bits, 40000 / 50000 / 60000 are negative in sixteen signed
    # bits -- a reader that took the wrong width gives "no NM" or another identity; values that need MORE than sixteen bits are
    # beyond the record's field and have files of their own below, test_a_read_beyond_the_records_fields_is_the_hosts_status)
    values = [100, 200, 300, 40000, 50000, 60000]
    variants += [_aux("NM", "C", 5) + _aux("XS", "A", "+") + yt, _aux("XS", "i", -70000) + yt + _aux("NM", "C", 6), md + _aux("NM", "C", 7)]
    values += [5, 6, 7]
    for k, (sub, vals) in enumerate((("c", [-1, 2, 3]), ("C", [255]), ("s", [-300, 5]), ("S", [65535] * 5), ("i", [1 << 30]), ("I", [4000000000, 1]), ("f", [1.5]))):
        variants.append(_aux("ZB", "B", (sub, vals)) + _aux("NM", "C", 10 + k))
        values.append(10 + k)
    variants += list(extra)
    records, facts = [], []
    for g, aux in enumerate(variants):
        q = [int(x) for x in rng.integers(20, 41, 1024)]
        records.append(_record(g, "r%d" % g, q, aux, mapq=40))
        if g < len(values):
            facts.append((g, 1024, 1024, values[g], q, 40))
    refs = _refs(len(variants))
    _write(path, refs, records)
    return refs, facts


def test_nm_of_every_width_and_in_every_place(ctx, tmp_path):
    path = str(tmp_path / "nm.bam")
    refs, facts = _nm_file(path)
    lengths = [l for _, l in refs]
    seen = set()
    # identities of 90.2, 80.5 and 70.7 percent, three below zero, the others above 98.4: the thresholds fall between them
    for mapid in (1.0, 75.0, 85.0, 95.0, 99.5):
        args = dict(mapid=mapid, readq=0, mapq=0, aln_cov=0.0)
        host, got = _host(ctx, path, args, lengths), _device(ctx, path, args, lengths)
        assert _same(host, _expected(facts, lengths, args)) and _same(got, host), mapid
        seen.add(int(got[1].sum()))
    assert seen == {13, 12, 11, 10, 1}


def test_a_tag_named_nm_that_is_no_integer_is_absent(ctx, tmp_path):
    path = str(tmp_path / "nmz.bam")
    refs, facts = _nm_file(path, extra=[_aux("NM", "Z", "3")])
    eh, ed = _both_raise(ctx, path, PERMISSIVE, [l for _, l in refs])
    assert (ed.status, ed.read_index, ed.message) == (eh.status, eh.read_index, eh.message) and eh.status == abi.ERR_READ_NO_NM and eh.read_index == len(refs) - 1


# ---- 5. records without a reference -------------------------------------------------------------------------------------------------

def test_the_read_index_counts_kept_records_only(ctx, tmp_path):
    rng = np.random.default_rng(9)
    records, kept = [], 0
    victim = None
    for k in range(300):
        q = [int(x) for x in rng.integers(10, 41, 40 + k % 50)]
        if k % 7 == 0:
            records.append(_record(-1, "u%d" % k, q, b""))
            continue
        if k == 250:
            victim = kept
        records.append(_record(k % 5, "r%d" % k, q, b"" if k == 250 else _aux("NM", "C", 1)))
        kept += 1
    path = str(tmp_path / "unmapped.bam")
    _write(path, _refs(5), records, block=4096)
    assert victim == 250 - len(range(0, 250, 7))
    eh, ed = _both_raise(ctx, path, PERMISSIVE, [1000 + 7 * i for i in range(5)])
    assert (ed.status, ed.read_index, ed.message) == (eh.status, eh.read_index, eh.message) and (eh.status, eh.read_index) == (abi.ERR_READ_NO_NM, victim)
    assert ctx.genes_count_bam_timing()[1]['dropped'] == len(range(0, 300, 7)) and ctx.genes_count_bam_timing()[1]['records'] == kept


@pytest.mark.parametrize("n_unmapped", [0, 40])
def test_no_kept_record_gives_zeros(ctx, tmp_path, n_unmapped):
    path = str(tmp_path / "empty.bam")
    _write(path, _refs(3), [_record(-1, "u%d" % k, [30] * 50) for k in range(n_unmapped)])
    lengths = [1000, 1007, 1014]
    got, host = _device(ctx, path, GENES_ARGS, lengths), _host(ctx, path, GENES_ARGS, lengths)
    assert _same(got, host) and got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0.0, 0.0, 0.0]
    stats = ctx.genes_count_bam_timing()[1]
    assert stats['records'] == 0 and stats['dropped'] == n_unmapped


# ---- 6. CIGAR ends ----------------------------------------------------------------------------------------------------------------

def test_cigar_ends_one_read_a_gene(ctx, tmp_path):
    cases = _edge_cases()
    reads = _make_edge(cases)
    n = reads.n_reads
    refid = np.arange(n, dtype=np.int32)
    names, lengths = ["g%d" % i for i in range(n)], [1000 + 7 * i for i in range(n)]
    path = str(tmp_path / "edge.bam")
    abi.write_bam(path, names, lengths, refid, reads)
    _, _, rid, host_reads = abi.read_bam(path)
    for args in EDGE_THRESHOLDS:
        term = ctx.genes_terms(_thr(args), host_reads, rid, lengths)
        aligned, mapped, depth = _device(ctx, path, args, lengths)
        assert aligned.tolist() == [1] * n
        assert depth.tobytes() == term.tobytes() and mapped.tolist() == (term > 0).astype(np.int64).tolist(), args
    exp = np.array([c[2] / float(lengths[i]) for i, c in enumerate(cases)])
    assert _device(ctx, path, PERMISSIVE, lengths)[2].tobytes() == exp.tobytes()        # (the hand-derived aligned lengths)


def test_a_read_of_clips_alone_is_zero_align(ctx, tmp_path):
    reads = _make_edge([(20, "20M", 20), _ZERO, (20, "20M", 20)])
    path = str(tmp_path / "zero.bam")
    abi.write_bam(path, ["a", "b", "c"], [500, 600, 700], np.arange(3, dtype=np.int32), reads)
    eh, ed = _both_raise(ctx, path, PERMISSIVE, [500, 600, 700])
    assert (ed.status, ed.read_index, ed.message) == (eh.status, eh.read_index, eh.message) and (eh.status, eh.read_index) == (abi.ERR_READ_ZERO_ALIGN, 1)


# ---- 7. one hot gene ----------------------------------------------------------------------------------------------------------------

def test_one_hot_gene_keeps_file_order(ctx, tmp_path):
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=8, n_reads=5200, seed=7, silent_fraction=0.0)
    refid = np.full_like(ds['refid'], 3)
    lengths = [len(s) for s in ds['gene_seq']]
    recs = [(3,) + r[1:] for r in _oracle_records(ds['reads'], refid)]
    exp_aligned, exp_mapped, exp_depth, _ = go.count_mapped_bp(GENES_ARGS, recs, ds['gene_ids'], ds['gene_species'], lengths)
    assert refid.size >= 5000 and exp_mapped[3] > 2048
    path = str(tmp_path / "hot.bam")
    abi.write_bam(path, ds['gene_ids'], lengths, refid, ds['reads'])
    aligned, mapped, depth = _device(ctx, path, GENES_ARGS, lengths)
    assert aligned.tolist() == exp_aligned and mapped.tolist() == exp_mapped and depth.tobytes() == np.array(exp_depth, np.float64).tobytes()


# ---- 8. statuses --------------------------------------------------------------------------------------------------------------------

def _status_file(path, at, rng_seed=21):
    """120 reads over 6 genes; at: {index: record bytes} put in place of the ordinary ones."""
    rng = np.random.default_rng(rng_seed)
    records = []
    for k in range(120):
        q = [int(x) for x in rng.integers(10, 41, 60 + k % 40)]
        records.append(at[k] if k in at else _record(k % 6, "r%d" % k, q, _aux("NM", "C", k % 3)))
    _write(path, _refs(6), records, block=2048)
    return [1000 + 7 * i for i in range(6)]


LONG = _record(2, "long", [30] * (MAX_L + 1), _aux("NM", "C", 0))
BIG_NM = _record(2, "bignm", [30] * 50, _aux("NM", "S", 65535))
# NM that needs more than sixteen bits: read through a narrower load it would be 4464 and give a count, not the status
WIDE_NM = [_record(2, "widenm", [30] * 50, _aux("NM", t, v)) for t, v in (("i", 70000), ("I", 70000), ("I", 4000000000))]
NO_NM = _record(1, "nonm", [30] * 50, b"")
OFF_TABLE = _record(6, "offtable", [30] * 50, _aux("NM", "C", 0))


@pytest.mark.parametrize("bad", [LONG, BIG_NM] + WIDE_NM, ids=["l_seq 1025", "NM:S 65535", "NM:i 70000", "NM:I 70000", "NM:I 4000000000"])
def test_a_read_beyond_the_records_fields_is_the_hosts_status(ctx, tmp_path, bad):
    path = str(tmp_path / "size.bam")
    lengths = _status_file(path, {37: bad, 90: bad})
    eh, ed = _both_raise(ctx, path, PERMISSIVE, lengths)
    assert (ed.status, ed.read_index, ed.message) == (eh.status, eh.read_index, eh.message) and (eh.status, eh.read_index) == (abi.ERR_UNSUPPORTED, 37)
    assert _same(_device(ctx, path, PERMISSIVE, _status_file(path, {})), _host(ctx, path, PERMISSIVE, lengths))       # the context carries nothing over


@pytest.mark.parametrize("where", [20, 80], ids=["in front", "behind"])
def test_a_malformed_read_comes_before_a_read_without_nm(ctx, tmp_path, where):
    path = str(tmp_path / "first.bam")
    lengths = _status_file(path, {50: NO_NM, where: LONG})
    eh, ed = _both_raise(ctx, path, PERMISSIVE, lengths)
    assert (ed.status, ed.read_index, ed.message) == (eh.status, eh.read_index, eh.message) and (eh.status, eh.read_index) == (abi.ERR_UNSUPPORTED, where)
    # a refID that names no reference of the header: the host's decode refuses the file, the one pass the record; both before the NM
    _status_file(path, {50: NO_NM, where: OFF_TABLE})
    eh, ed = _both_raise(ctx, path, PERMISSIVE, lengths)
    assert ed.status == eh.status == abi.ERR_BAD_LAYOUT and ed.read_index == where


def test_a_flipped_crc_byte_names_the_block(ctx, tmp_path):
    path = str(tmp_path / "crc.bam")
    lengths = _status_file(path, {})
    data = bytearray(open(path, "rb").read())
    at, starts = 0, []
    while at < len(data):
        starts.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    assert len(starts) > 4
    victim = starts[3] - 8                       # the CRC-32 in the footer of the third block
    data[victim] ^= 0x40
    open(path, "wb").write(bytes(data))
    with pytest.raises(abi.MidasSnpsError) as eh:
        abi.read_bam(path, ctx)
    with pytest.raises(abi.MidasSnpsError) as ed:
        _device(ctx, path, PERMISSIVE, lengths)
    assert ed.value.status == eh.value.status == abi.ERR_BAD_LAYOUT
    assert ed.value.message == eh.value.message and "file offset %d " % starts[2] in ed.value.message
    data[victim] ^= 0x40
    open(path, "wb").write(bytes(data))
    assert _same(_device(ctx, path, PERMISSIVE, lengths), _host(ctx, path, PERMISSIVE, lengths))        # the same context, afterwards


# ---- 9. the command ---------------------------------------------------------------------------------------------------------------

def _run_cli(out, db, fq, mode):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_midas.py"), "genes", out, "--call_genes", "-d", db, "-1", fq,
                           "--device_inflate", mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _fastq(tmp_path):
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as h:
        h.write("@r1\nACGT\n+\nIIII\n")
    return fq


def _outputs(out, species_ids):
    return ([gzip.open(os.path.join(out, "genes", "output", sp + ".genes.gz"), "rb").read() for sp in species_ids],
            open(os.path.join(out, "genes", "summary.txt"), "rb").read())


def _stdout(r, mode):
    """stdout less what cannot be equal between two runs: in the echo of the command line the option's value is masked, and the two
    lines of the stage's own clock and memory are dropped.  Every other line, the command line's other words included, stays as
    it was printed and is compared verbatim."""
    lines = [l.replace("--device_inflate " + mode, "--device_inflate *") if l.startswith("command:") else l for l in r.stdout.split("\n")]
    return [l for l in lines if not l.endswith(" minutes") and not l.endswith(" Gb maximum memory")]


def test_the_command_writes_the_same_files_by_both_routes(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=3, genes_per_species=40, n_reads=6000, seed=23)
    out, db, fq = str(tmp_path / "s"), str(tmp_path / "db"), _fastq(tmp_path)
    synth.write_pangenome_sample(out, db, ds)
    _, _, _, tables, summary = _oracle(ds, GENES_ARGS)
    results = {}
    for mode in ("on", "off"):
        r = _run_cli(out, db, fq, mode)
        assert r.returncode == 0, r.stderr
        results[mode] = (_outputs(out, ds['species_ids']), _stdout(r, mode), open(os.path.join(out, "genes", "log.txt")).read())
        for sp in ds['species_ids']:
            assert gzip.open(os.path.join(out, "genes", "output", sp + ".genes.gz"), "rt").read() == tables[sp], (mode, sp)
        assert open(os.path.join(out, "genes", "summary.txt")).read() == summary, mode
    assert results["on"][0] == results["off"][0] and results["on"][1] == results["off"][1]
    assert "one pass on the device" in results["on"][2] and "%d records decoded" % ds['refid'].size in results["on"][2]
    assert "decoded by the host's threads, %d records" % ds['refid'].size in results["off"][2] and "one pass" not in results["off"][2]
    assert "one pass" not in results["on"][1] and "host's threads" not in results["off"][1]


def _exits_alike(tmp_path, ds, bam_writer=None):
    out, db, fq = str(tmp_path / "s"), str(tmp_path / "db"), _fastq(tmp_path)
    synth.write_pangenome_sample(out, db, ds)
    if bam_writer:
        bam_writer(os.path.join(out, "genes", "temp", "pangenomes.bam"))
    runs = [_run_cli(out, db, fq, mode) for mode in ("on", "off")]
    assert runs[0].returncode == runs[1].returncode == 1
    assert runs[0].stderr == runs[1].stderr
    return runs[0].stderr


def test_a_header_gene_the_database_lacks_exits_as_the_host_route_does(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=12, n_reads=600, seed=29)
    lengths = [len(s) for s in ds['gene_seq']]
    refid = ds['refid'].copy()
    refid[77] = len(lengths)

    def with_a_ghost(path):
        abi.write_bam(path, list(ds['gene_ids']) + ["ghost"], lengths + [900], refid, ds['reads'])
    assert "gene 'ghost' of the BAM header is not in the pangenome database" in _exits_alike(tmp_path, ds, with_a_ghost)


def test_a_read_without_nm_exits_with_the_host_routes_text_and_index(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=12, n_reads=600, seed=29)
    ds['reads'].nm[41] = -1
    err = _exits_alike(tmp_path, ds)
    assert "NM" in err and "[read 41 of the BAM]" in err
