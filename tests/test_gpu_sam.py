"""SAM input on the GPU: midas_sam_load_device (midas_amd/csrc/sam_scan.hip) against the independent model (tests/sam_model.py)
and against the BAM decode of the same reads; chunking and line ends; `run_midas.py snps --pileup` over a SAM against the same
sample's BAM run; the hand-derived cases; refused lines as statuses naming the line; two ranks with only a SAM."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, synth
from tests import helpers as H
from tests import sam_model
from tests.sam_model import assert_columns_equal, reads_columns, sam_file_order

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def device_columns(ctx, path):
    names, lens, refid, reads = abi.read_sam(path, ctx)
    assert reads.device is not None and reads.seq4.size == 0
    full = ctx.fetch_payload(reads)
    return names, lens, reads_columns(refid, full)


def check_against_model(ctx, path):
    names, lens, got = device_columns(ctx, path)
    mn, ml, exp = sam_model.decode(open(path, "rb").read())
    assert names == mn and lens == ml
    assert_columns_equal(got, exp, path)
    return got


def _sample(seed, **kw):
    contigs, reads = synth.make_dataset(seed=seed, **kw)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    return contigs, reads, refid


def _long_read_sample():
    """A few ordinary reads and one 5 kb read with a long CIGAR."""
    contigs, reads, refid = _sample(41, n_species=1, contigs_per_species=2, contig_len=9000, n_reads=300)
    rng = np.random.default_rng(7)
    L = 5000
    ops = []
    left = L
    while left > 40:
        m = int(rng.integers(5, 30))
        ops += [(0, m), (1, 1)]
        left -= m + 1
    ops.append((0, left))
    one = H.reads_from_dicts([dict(pos=1234, cigar=ops, seq="".join("ACGTN"[int(x)] for x in rng.integers(0, 5, L)),
                                   qual=[int(x) for x in rng.integers(2, 42, L)], nm=77, mapq=33, flag=16)])
    return contigs, synth.concat_reads([reads, one]), np.concatenate([refid, np.array([1], np.int32)])


SAMPLES = {
    "s11": lambda: _sample(11, n_species=2, contigs_per_species=3, contig_len=6000, n_reads=4000, var_len=True, lowercase_frac=0.05),
    "s12": lambda: _sample(12, n_species=3, contigs_per_species=2, contig_len=5000, n_reads=3000),
    "s13_250": lambda: _sample(13, n_species=1, contigs_per_species=4, contig_len=7000, n_reads=2500, read_len=250, var_len=True),
    "long_5kb": _long_read_sample,
}


def test_spec_fixture_columns(ctx):
    got = check_against_model(ctx, os.path.join(H.GOLDEN, "spec_fixture.sam"))
    names, lens, refid, reads = abi.read_bam(os.path.join(H.GOLDEN, "spec_fixture.bam"), ctx, payload_on_device=True)
    n = int(refid.size)
    came = sam_file_order(np.asarray(refid), np.asarray(reads.pos), np.arange(n)[::-1])
    assert_columns_equal(sam_model.reorder(got, np.argsort(came)), reads_columns(refid, ctx.fetch_payload(reads)), "fixture vs BAM")


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_columns_equal_the_model_and_the_bam_decode(ctx, tmp_path, name):
    contigs, reads, refid = SAMPLES[name]()
    lens = [int(x) for x in contigs.length]
    order = np.random.default_rng(len(name)).permutation(reads.n_reads)
    sam, bam = str(tmp_path / "x.sam"), str(tmp_path / "x.bam")
    synth.write_sam(sam, contigs.ids, lens, reads, refid, order=order)
    got = check_against_model(ctx, sam)
    assert got["refid"].size == reads.n_reads
    key = got["refid"].astype(np.int64) << 32 | (got["pos"].astype(np.int64) + 1)
    assert (key[1:] >= key[:-1]).all()
    # the same reads written sorted, as a BAM: both in (refID, pos, file index) order
    srt = np.lexsort((np.arange(reads.n_reads), np.asarray(reads.pos), refid))
    cols = sam_model.reorder(reads_columns(refid, reads), srt)
    sorted_reads = abi.ReadsSoA(**{k: v for k, v in cols.items() if k != "refid"})
    abi.write_bam(bam, contigs.ids, lens, cols["refid"], sorted_reads)
    _, _, brefid, breads = abi.read_bam(bam, ctx, payload_on_device=True)
    bcols = reads_columns(brefid, ctx.fetch_payload(breads))
    came = sam_file_order(refid, np.asarray(reads.pos), order)          # original indices, in the SAM decode's order
    rank_in_bam = np.empty(reads.n_reads, np.int64)
    rank_in_bam[srt] = np.arange(reads.n_reads)
    assert_columns_equal(sam_model.reorder(got, np.argsort(rank_in_bam[came])), bcols, name + " vs BAM")


def test_the_decoded_bytes_do_not_depend_on_the_chunk_size(ctx, tmp_path, monkeypatch):
    contigs, reads, refid = SAMPLES["s11"]()
    sam = str(tmp_path / "x.sam")
    synth.write_sam(sam, contigs.ids, [int(x) for x in contigs.length], reads, refid, order=np.random.default_rng(3).permutation(reads.n_reads))
    base = device_columns(ctx, sam)[2]
    two_lines = min(len(l) for l in open(sam, "rb").read().split(b"\n")[8:-1]) * 2
    for chunk in (64, 4096, 1 << 16):       # 64: smaller than any line -- it has to grow
        assert 64 < two_lines
        monkeypatch.setenv("MIDAS_SNPS_SAM_CHUNK_BYTES", str(chunk))
        assert_columns_equal(device_columns(ctx, sam)[2], base, "chunk %d" % chunk)
    monkeypatch.delenv("MIDAS_SNPS_SAM_CHUNK_BYTES")
    # no trailing newline; \r\n line ends -- whole, and in small chunks
    data = open(sam, "rb").read()
    bare, crlf = str(tmp_path / "bare.sam"), str(tmp_path / "crlf.sam")
    open(bare, "wb").write(data[:-1])
    open(crlf, "wb").write(data.replace(b"\n", b"\r\n"))
    for path in (bare, crlf):
        assert_columns_equal(check_against_model(ctx, path), base, path)
        monkeypatch.setenv("MIDAS_SNPS_SAM_CHUNK_BYTES", "1000")
        assert_columns_equal(device_columns(ctx, path)[2], base, path + " chunked")
        monkeypatch.delenv("MIDAS_SNPS_SAM_CHUNK_BYTES")


MANY_SQ = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:ref%d\tLN:%d\n" % (k, 1000 + k) for k in range(100))      # 101 lines
HEAD = b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:900\n@SQ\tSN:d e\tLN:50\n"
GOOD = b"q\t0\tc\t7\t40\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n"


def test_odd_but_legal_text(ctx, tmp_path):
    """Lower case, '=', '.', IUPAC letters, every CIGAR op, leading zeros, POS 0, tags in front of NM, NM of another type, a
    negative NM, RNAME '*' between the others, an RNAME with a blank in it."""
    body = (GOOD +
            b"q\t65535\td e\t0\t255\t1M2I3D4N5S6H7P8=9X\t=\t1\t-5\tacgtnNmrsvwyhkdb=.x\t!\"#$%&'()*+,-./0123\tXS:A:+\tNM:Z:3\tXX:i:5\tNM:i:-7\tNM:i:2\n" +
            b"q\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\t+++++\n" +
            b"q\t0016\tc\t0000000007\t007\t0004M\t*\t0\t0\tAC\t*\n" +
            b"q\t0\tc\t7\t0\t*\t*\t0\t0\t*\t*\tNM:i:99999999999\n" +
            b"q\t0\tc\t2147483647\t1\t1M\t*\t0\t0\tA\t~\n")
    path = str(tmp_path / "odd.sam")
    open(path, "wb").write(HEAD + body)
    got = check_against_model(ctx, path)
    assert got["refid"].tolist() == [0, 0, 0, 0, 1] and got["pos"].tolist() == [6, 6, 6, 2147483646, -1]
    assert got["nm"].tolist() == [0, -1, 2147483647, -1, -7]


@pytest.mark.parametrize("what,body,line", [
    ("short line", GOOD + b"q\t0\tc\t7\t40\t4M\t*\t0\t0\tACGT\n", 5),
    ("bad FLAG", GOOD + GOOD + GOOD.replace(b"q\t0\t", b"q\t0x10\t"), 6),
    ("FLAG out of range", GOOD.replace(b"q\t0\t", b"q\t65536\t"), 4),
    ("unknown RNAME", GOOD + GOOD.replace(b"\tc\t", b"\tcc\t") + GOOD.replace(b"\tc\t", b"\tzz\t"), 5),
    ("bad CIGAR letter", GOOD.replace(b"4M", b"2M2B"), 4),
    ("CIGAR without a length", GOOD.replace(b"4M", b"M4"), 4),
    ("QUAL length mismatch", GOOD + GOOD.replace(b"IIII", b"IIIII"), 5),
    ("QUAL character", GOOD.replace(b"IIII", b"II I"), 4),
    ("POS", GOOD.replace(b"\t7\t40", b"\t2147483648\t40"), 4),
    ("MAPQ", GOOD.replace(b"\t7\t40", b"\t7\t256"), 4),
    ("empty line", GOOD + b"\n" + GOOD, 5),
])
def test_a_bad_line_is_a_status_naming_the_line(ctx, tmp_path, what, body, line):
    path = str(tmp_path / "bad.sam")
    open(path, "wb").write(HEAD + body)
    with pytest.raises(sam_model.SamError) as mi:
        sam_model.decode(HEAD + body)
    assert mi.value.line == line
    for chunk in (None, "100"):       # the first bad line wins whatever chunk met it
        if chunk:
            os.environ["MIDAS_SNPS_SAM_CHUNK_BYTES"] = chunk
        try:
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.read_sam(path, ctx)
        finally:
            os.environ.pop("MIDAS_SNPS_SAM_CHUNK_BYTES", None)
        assert ei.value.status == abi.ERR_BAD_LAYOUT, what
        assert "line %d:" % line in ei.value.message, ei.value.message


def test_the_first_bad_line_in_file_order_wins(ctx, tmp_path):
    path = str(tmp_path / "two.sam")
    lines = [GOOD] * 40
    lines[31] = GOOD.replace(b"IIII", b"III")
    lines[9] = GOOD.replace(b"\tc\t", b"\tnope\t")
    open(path, "wb").write(HEAD + b"".join(lines))
    for chunk in ("90", "700", None):
        if chunk:
            os.environ["MIDAS_SNPS_SAM_CHUNK_BYTES"] = chunk
        try:
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.read_sam(path, ctx)
        finally:
            os.environ.pop("MIDAS_SNPS_SAM_CHUNK_BYTES", None)
        assert ei.value.status == abi.ERR_BAD_LAYOUT and "line 13:" in ei.value.message, ei.value.message


@pytest.mark.parametrize("text,line", [
    (b"@HD\tVN:1.6\n" + GOOD, 2),                                   # a record before any @SQ
    (b"@SQ\tSN:c\n" + GOOD, 1),                                     # no LN
    (b"@SQ\tLN:5\n" + GOOD, 1),                                     # no SN
    (b"@SQ\tSN:c\tLN:900\n@CO\tx\n@SQ\tSN:c\tLN:900\n" + GOOD, 3),   # duplicate SN
    (b"@SQ\tSN:c\tLN:12x\tLN:5\n" + GOOD, 1),                      # the first LN counts, and it is no number
    (b"@SQ\tSN:\tSN:c\tLN:5\n" + GOOD, 1),                         # the first SN counts, and it is empty
    (MANY_SQ + b"@SQ\tSN:ref17\tLN:5\n@SQ\tSN:x\n" + GOOD, 102),    # many references: the duplicate comes first in the file ...
    (MANY_SQ + b"@SQ\tSN:x\n@SQ\tSN:ref17\tLN:5\n" + GOOD, 102),    # ... or the @SQ without LN does
])
def test_header_errors(ctx, tmp_path, text, line):
    path = str(tmp_path / "h.sam")
    open(path, "wb").write(text)
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.read_sam(path, ctx)
    assert ei.value.status == abi.ERR_BAD_LAYOUT and "line %d:" % line in ei.value.message, ei.value.message
    with pytest.raises(sam_model.SamError) as mi:
        sam_model.decode(text)
    assert mi.value.line == line


def test_a_header_of_many_references(ctx, tmp_path):
    """More @SQ lines than any other test writes (a metagenome's header holds thousands): every name finds its refID."""
    path = str(tmp_path / "many.sam")
    body = b"".join(GOOD.replace(b"\tc\t", b"\tref%d\t" % k).replace(b"\t7\t40", b"\t%d\t40" % (k % 7 + 1)) for k in (99, 0, 64, 17, 63, 17, 65))
    open(path, "wb").write(MANY_SQ + body)
    got = check_against_model(ctx, path)
    assert got["refid"].tolist() == [0, 17, 17, 63, 64, 65, 99]
    names, lens, _ = device_columns(ctx, path)
    assert names == ["ref%d" % k for k in range(100)] and lens == [1000 + k for k in range(100)]


def test_unmapped_records_are_dropped_and_empty_files_decode(ctx, tmp_path):
    path = str(tmp_path / "u.sam")
    star = b"q\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n"
    open(path, "wb").write(HEAD + star + GOOD + star + star)
    got = check_against_model(ctx, path)
    assert got["refid"].tolist() == [0] and got["seq4"].tolist() == [0x12, 0x48]
    open(path, "wb").write(HEAD + star)
    assert check_against_model(ctx, path)["refid"].size == 0
    open(path, "wb").write(HEAD)
    names, lens, got = device_columns(ctx, path)
    assert names == ["c", "d e"] and lens == [900, 50] and got["refid"].size == 0 and got["seq_off"].tolist() == [0]


def _run_pileup(out, db, extra=()):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_midas.py"), "snps", out, "--pileup", "-d", db, "-t", "4"] + list(extra),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_pileup_over_a_sam_writes_the_bam_runs_files(tmp_path):
    contigs, reads = synth.make_dataset(n_species=3, contigs_per_species=4, contig_len=6000, n_reads=9000, seed=17, var_len=True,
                                        lowercase_frac=0.05)
    a, b, db = str(tmp_path / "bam"), str(tmp_path / "sam"), str(tmp_path / "db")
    synth.write_sample(a, db, contigs, reads)
    synth.write_sample(b, db, contigs, reads, sam=True)
    assert os.path.isfile(os.path.join(b, "snps", "temp", "genomes.sam")) and not os.path.exists(os.path.join(b, "snps", "temp", "genomes.bam"))
    # ... and unsorted, as the aligner leaves it
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    synth.write_sam(os.path.join(b, "snps", "temp", "genomes.sam"), contigs.ids, [int(x) for x in contigs.length], reads, refid,
                    order=np.random.default_rng(5).permutation(reads.n_reads))
    for d in (a, b):
        r = _run_pileup(d, db)
        assert r.returncode == 0, r.stderr
    files = sorted(os.listdir(os.path.join(a, "snps", "output")))
    assert files == sorted(os.listdir(os.path.join(b, "snps", "output"))) and len(files) == 3
    for f in files:
        assert gzip.open(os.path.join(a, "snps", "output", f), "rb").read() == gzip.open(os.path.join(b, "snps", "output", f), "rb").read(), f
    assert open(os.path.join(a, "snps", "summary.txt")).read() == open(os.path.join(b, "snps", "summary.txt")).read()
    assert "coordinate-sorted on the GPU" in open(os.path.join(b, "snps", "log.txt")).read()
    assert "coordinate-sorted on the GPU" not in open(os.path.join(a, "snps", "log.txt")).read()


def test_kat_cases_written_as_sam(ctx, tmp_path):
    """The hand-derived cases through SAM text (lines in reversed order): the decoded reads give the expected counts and
    counters, or the status the case expects.  A case whose read starts more than one position in front of its contig cannot be
    written as SAM (POS would be negative) and is left to the BAM tests."""
    ran = 0
    for case in H.load_kat_cases():
        contigs, reads, thr, args = H.kat_inputs(case)
        if reads.n_reads and int(np.asarray(reads.pos).min()) < -1:
            continue
        path = str(tmp_path / (case["name"] + ".sam"))
        synth.write_sam(path, contigs.ids, [int(x) for x in contigs.length], reads, np.zeros(reads.n_reads, np.int32),
                        order=np.arange(reads.n_reads)[::-1])
        names, lens, refid, dreads = abi.read_sam(path, ctx)
        assert dreads.n_reads == reads.n_reads and (refid == 0).all()
        table = abi.ContigTable(length=contigs.length, species=contigs.species, read_begin=[0, dreads.n_reads], ref=contigs.ref,
                                n_species=1, ids=contigs.ids, species_ids=contigs.species_ids)
        ctx.set_pad_rule(abi.PAD_PYSAM if H.kat_pysam_pad_rule(case) else abi.PAD_SPEC)
        try:
            if "error" in case:
                with pytest.raises(abi.MidasSnpsError) as ei:
                    ctx.pileup(thr, table, dreads)
                assert ei.value.status == case["error"], case["name"]
            else:
                counts, allele, stats = ctx.pileup(thr, table, dreads)
                assert np.array_equal(counts, H.kat_expected_counts(case)), case["name"]
                assert np.array_equal(stats, H.kat_expected_stats(case)), case["name"]
        finally:
            ctx.set_pad_rule(abi.PAD_SPEC)
        ran += 1
    assert ran >= 30


@pytest.mark.parametrize("edit,status,text", [
    (lambda l: l.replace(b"\tACGT\tIIII", b"\t*\t*"), abi.ERR_READ_NO_SEQ, "has no SEQ"),
    (lambda l: l.replace(b"\tIIII", b"\t*"), abi.ERR_READ_NO_QUAL, "has no QUAL"),
    (lambda l: l.replace(b"\tNM:i:0", b"\tNM:Z:0"), abi.ERR_READ_NO_NM, "has no NM tag"),
])
def test_missing_seq_qual_nm_reach_the_pileups_messages(tmp_path, edit, status, text):
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=1, contig_len=900, n_reads=50, seed=3)
    out, db = str(tmp_path / "s"), str(tmp_path / "db")
    synth.write_sample(out, db, contigs, reads, sam=True)
    sam = os.path.join(out, "snps", "temp", "genomes.sam")
    line = edit(GOOD.replace(b"\tc\t", b"\t" + contigs.ids[0].encode() + b"\t"))
    assert line != GOOD
    open(sam, "ab").write(line)
    r = _run_pileup(out, db)
    assert r.returncode != 0 and "Error: an alignment " + text in r.stderr, r.stderr[-1500:]


def test_two_ranks_with_only_a_sam_exit_together(tmp_path):
    from tests.test_dist_gloo import ROOT as R, SNPS_WORKER, _run_snps_workers
    script = tmp_path / "snps_worker.py"
    script.write_text(SNPS_WORKER % {"root": R})
    contigs, reads = synth.make_dataset(n_species=2, contigs_per_species=2, contig_len=5000, n_reads=2000, seed=8)
    out, db = str(tmp_path / "s"), str(tmp_path / "db")
    synth.write_sample(out, db, contigs, reads, sam=True)
    os.environ["SNPS_REAL_DEVICE"] = "1"
    try:
        res = _run_snps_workers(tmp_path, script, out, db, 2)
    finally:
        os.environ.pop("SNPS_REAL_DEVICE", None)
    assert len(res) == 2
    for rc, o, e in res:
        assert rc != 0 and "2-rank runs need snps/temp/genomes.bam" in e, e[-1500:]
    assert not os.listdir(os.path.join(out, "snps", "output"))
