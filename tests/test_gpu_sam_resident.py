"""SAM text straight into the pileup kernel's layout (midas_sam_load_resident, abi.read_sam(..., resident=True)): the columns cut
back out of the resident handle against the independent model (tests/sam_model.py) at every size border of sam_direct_kernel --
record counts around a workgroup's eight half-wave slots and beyond one grid, l_seq around the 8 bases a lane and the 256 a half
wave encode a step and beyond 16 bits, CIGARs around the 64 ops a step copies, every kind of exceptional read, odd l_seq; the
same bytes whatever the chunk size and the line ends; batches over the handle against the C oracle and against batches over the
same reads' resident BAM; refused files; and `run_midas.py snps --pileup` under MIDAS_SNPS_SAM_RESIDENT."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, bam, synth
from oracle import c_oracle
from tests import helpers as H
from tests import sam_model
from tests.sam_model import assert_columns_equal, reads_columns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def resident(ctx, path):
    names, lens, refid, rr = abi.read_sam(path, ctx, resident=True)
    assert isinstance(rr, abi.ResidentReads) and rr.n_reads == refid.size and rr.first == 0
    return names, lens, refid, rr


def resident_columns(ctx, path):
    names, lens, refid, rr = resident(ctx, path)
    came_down = np.array(refid)                 # refID as the decode left it on the host, before any other column exists there
    cols = rr.to_columns(ctx)
    assert cols.device is not None and cols.seq4.size == 0
    full = ctx.fetch_payload(cols)
    assert rr.l_seq_total == int(np.asarray(full.l_seq).sum(dtype=np.int64))
    np.testing.assert_array_equal(came_down, refid)
    return names, lens, reads_columns(came_down, full)


def check_against_model(ctx, path):
    names, lens, got = resident_columns(ctx, path)
    mn, ml, exp = sam_model.decode(open(path, "rb").read())
    assert names == mn and lens == ml
    assert np.array_equal(got["refid"], exp["refid"]), path       # (the host's refID column)
    assert_columns_equal(got, exp, path)
    return got


# ---- SAM text by hand ------------------------------------------------------------------------------------------------------------
HEAD = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c\tLN:200000\n@SQ\tSN:d e\tLN:5000\n"
GOOD = b"q\t0\tc\t7\t40\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\n"


def sam_line(name, flag=0, rname=b"c", pos=1, mapq=40, cigar=b"*", seq=b"*", qual=b"*", tags=b"NM:i:0"):
    f = [name, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, b"*", b"0", b"0", seq, qual]
    return b"\t".join(f + ([tags] if tags else [])) + b"\n"


def _bases(rng, l):
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, l))


def _quals(rng, l):
    return bytes(int(x) for x in rng.integers(33 + 2, 33 + 42, l))


def shape_lines():
    """Every shape of the list above once (more where a shape has several forms), in a shuffled line order."""
    rng = np.random.default_rng(5)
    out = []
    for l in (0, 1, 7, 8, 9, 255, 256, 257, 70000):                      # l_seq; the odd ones carry a pad nibble
        out.append(sam_line(b"l%d" % l, pos=int(rng.integers(1, 100000)), cigar=b"%dM" % l if l else b"*", seq=_bases(rng, l) or b"*",
                            qual=_quals(rng, l) or b"*"))
    for k in (0, 1, 2, 63, 64, 65):                                      # n_cigar
        ops = [b"2M" if j % 2 == 0 else b"1I" for j in range(k)]
        l = sum(2 if j % 2 == 0 else 1 for j in range(k)) or 10
        out.append(sam_line(b"c%d" % k, flag=16, rname=b"d e", pos=int(rng.integers(1, 4000)), cigar=b"".join(ops) or b"*", seq=_bases(rng, l),
                            qual=_quals(rng, l), tags=b"XS:i:3\tNM:i:%d" % k))
    exceptional = [
        (b"iupac", b"ACGTRYACGTM", None), (b"equals", b"AC=GT=", None), (b"lower", b"acgtnacgt", None),
        (b"tilde", b"ACGTACGTAC", b"~~~~~~~~~~"), (b"one_tilde", b"ACGTACGTACGTA", b"IIIIIII~IIIII"),
        (b"n51", b"ACNGT", b"IITII"), (b"n52", b"ACNGT", b"IIUII"), (b"noqual", b"ACGTACG", b"*"),
        (b"exact", b"ACGTNACGT", b"SSSSTSSSS"),                            # q 50 on A/C/G/T and q 51 on N: the last the bytes give back
    ]
    for name, seq, qual in exceptional:
        out.append(sam_line(name, pos=int(rng.integers(1, 100000)), cigar=b"%dM" % len(seq), seq=seq, qual=qual or _quals(rng, len(seq))))
    out.append(sam_line(b"nm_absent", pos=4242, cigar=b"5M", seq=b"ACGTA", qual=b"IIIII", tags=b"YT:Z:UU"))
    out.append(sam_line(b"nm_70000", pos=4243, cigar=b"5M", seq=b"ACGTA", qual=b"IIIII", tags=b"NM:i:70000"))
    out.append(sam_line(b"pos0", pos=0, cigar=b"3M", seq=b"ACG", qual=b"III"))
    for k in range(3):                                                  # equal (refID, pos) keys in three different lines
        out.append(sam_line(b"tie%d" % k, pos=777, mapq=10 + k, cigar=b"%dM" % (4 + k), seq=_bases(rng, 4 + k), qual=_quals(rng, 4 + k)))
    for k in range(6):                                                  # unmapped lines between the mapped ones
        out.append(sam_line(b"u%d" % k, flag=4, rname=b"*", pos=0, mapq=0, seq=_bases(rng, 9 + k), qual=_quals(rng, 9 + k), tags=b""))
    return [out[int(i)] for i in rng.permutation(len(out))]


def count_lines(n, seed):
    """n short mapped records (every ninth one exceptional) and a few unmapped ones between them, in random coordinate order."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        l = int(rng.integers(1, 40))
        seq = _bases(rng, l) if i % 9 else b"N" * l
        qual = _quals(rng, l) if i % 9 else b"U" * l               # (N at q 52)
        on_d = i % 5 == 0
        out.append(sam_line(b"r%d" % i, rname=b"d e" if on_d else b"c", pos=int(rng.integers(1, 4000 if on_d else 150000)), mapq=int(rng.integers(0, 61)),
                            cigar=b"%dM" % l, seq=seq, qual=qual, tags=b"NM:i:%d" % (i % 4)))
        if i % 50 == 7:
            out.append(sam_line(b"u%d" % i, flag=4, rname=b"*", pos=0, mapq=0, seq=seq, qual=qual, tags=b""))
    return out


def _write(path, lines, head=HEAD):
    with open(path, "wb") as f:
        f.write(head + b"".join(lines))
    return path


# ---- 1. columns ------------------------------------------------------------------------------------------------------------------
def test_every_shape_comes_back_as_the_models_columns(ctx, tmp_path):
    got = check_against_model(ctx, _write(str(tmp_path / "shapes.sam"), shape_lines()))
    assert got["refid"].size == 9 + 6 + 9 + 3 + 3 and int(got["l_seq"].max()) == 70000 and int(got["nm"].max()) == 70000
    ties = [int(l[3:4]) for l in shape_lines() if l.startswith(b"tie")]                                  # as their lines come in the file
    assert sorted(ties) == [0, 1, 2] and got["mapq"][got["pos"] == 776].tolist() == [10 + k for k in ties]      # equal keys keep that order
    assert int(got["pos"].min()) == -1 and (got["nm"] == -1).sum() == 1
    assert sorted(np.diff(got["cigar_off"]).tolist())[-3:] == [63, 64, 65]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 3000, 34000])     # eight half-wave slots a workgroup; 34 000: more records than one grid holds slots
def test_record_counts_around_a_workgroup_and_beyond_a_grid(ctx, tmp_path, n):
    got = check_against_model(ctx, _write(str(tmp_path / "n.sam"), count_lines(n, seed=n + 1)))
    assert got["refid"].size == n


def test_the_spec_fixture(ctx):
    check_against_model(ctx, os.path.join(H.GOLDEN, "spec_fixture.sam"))


def _sample(seed, **kw):
    contigs, reads = synth.make_dataset(seed=seed, **kw)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    return contigs, reads, refid


SAMPLES = {
    "s11": lambda: _sample(11, n_species=2, contigs_per_species=3, contig_len=6000, n_reads=4000, var_len=True, lowercase_frac=0.05),
    "s13_250": lambda: _sample(13, n_species=1, contigs_per_species=4, contig_len=7000, n_reads=2500, read_len=250, var_len=True),
}


@pytest.mark.parametrize("name", sorted(SAMPLES))
def test_synthetic_samples(ctx, tmp_path, name):
    contigs, reads, refid = SAMPLES[name]()
    sam = str(tmp_path / "x.sam")
    synth.write_sam(sam, contigs.ids, [int(x) for x in contigs.length], reads, refid, order=np.random.default_rng(len(name)).permutation(reads.n_reads))
    got = check_against_model(ctx, sam)
    assert got["refid"].size == reads.n_reads
    key = got["refid"].astype(np.int64) << 32 | (got["pos"].astype(np.int64) + 1)
    assert (key[1:] >= key[:-1]).all()


# ---- 2. chunking -----------------------------------------------------------------------------------------------------------------
def test_the_bytes_do_not_depend_on_the_chunk_size_or_the_line_ends(ctx, tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    lines = shape_lines() + count_lines(500, seed=77)
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    sam = _write(str(tmp_path / "x.sam"), lines)
    base = check_against_model(ctx, sam)
    for chunk in (64, 4096, 65536):           # 64: smaller than any line -- it has to grow, up to the 70 000-base line's 140 kB
        monkeypatch.setenv("MIDAS_SNPS_SAM_CHUNK_BYTES", str(chunk))
        assert_columns_equal(resident_columns(ctx, sam)[2], base, "chunk %d" % chunk)
    monkeypatch.delenv("MIDAS_SNPS_SAM_CHUNK_BYTES")
    data = open(sam, "rb").read()
    bare, crlf = str(tmp_path / "bare.sam"), str(tmp_path / "crlf.sam")
    open(bare, "wb").write(data[:-1])
    open(crlf, "wb").write(data.replace(b"\n", b"\r\n"))
    for path in (bare, crlf):
        assert_columns_equal(check_against_model(ctx, path), base, path)
        monkeypatch.setenv("MIDAS_SNPS_SAM_CHUNK_BYTES", "4096")
        assert_columns_equal(resident_columns(ctx, path)[2], base, path + " chunked")
        monkeypatch.delenv("MIDAS_SNPS_SAM_CHUNK_BYTES")


# ---- 3. counts -------------------------------------------------------------------------------------------------------------------
def _thr(baseq):
    return abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq))


def _counts_sample():
    """Reads of a synthetic sample, some of them exceptional in the direct layout: every quality 93, one quality 60, an N at q 51 / 52."""
    contigs, reads, refid = _sample(21, n_species=2, contigs_per_species=3, contig_len=6000, n_reads=4000, var_len=True, lowercase_frac=0.05)
    rng = np.random.default_rng(9)
    qual, seq4 = np.array(reads.qual), np.array(reads.seq4)
    so, qo = np.asarray(reads.seq_off), np.asarray(reads.qual_off)
    picks = rng.choice(reads.n_reads, 160, replace=False)
    for i in picks[:40]:
        qual[qo[i]:qo[i + 1]] = 93
    for i in picks[40:80]:
        qual[qo[i] + int(rng.integers(0, qo[i + 1] - qo[i]))] = 60
    for i, q in zip(picks[80:160], [51, 52] * 40):
        seq4[so[i]] |= 0xF0          # the read's first base: N
        qual[qo[i]] = q
    return contigs, abi.ReadsSoA(**{**reads.as_dict(), "qual": qual, "seq4": seq4}), refid


def _fetch(batch, thr):
    batch.run(thr)
    return batch.fetch()


def test_batches_over_the_handle_count_what_the_oracle_and_the_bam_count(ctx, tmp_path):
    contigs, reads, refid = _counts_sample()
    lens = [int(x) for x in contigs.length]
    sam, bamp = str(tmp_path / "x.sam"), str(tmp_path / "x.bam")
    synth.write_sam(sam, contigs.ids, lens, reads, refid, order=np.random.default_rng(4).permutation(reads.n_reads))
    bam.write_bam(bamp, contigs.ids, lens, refid, reads)                  # (the sample's reads are coordinate-sorted as they are)
    _, _, srefid, srr = resident(ctx, sam)
    _, _, brefid, brr = abi.read_bam(bamp, ctx, resident=True)
    assert isinstance(brr, abi.ResidentReads)
    np.testing.assert_array_equal(srefid, brefid)
    off = contigs.site_offsets()
    oracle = {q: c_oracle.pileup(_thr(q), contigs, reads) for q in (0, 30, 51)}
    assert all(o[0] == 0 for o in oracle.values())
    stats = {q: np.zeros_like(oracle[q][4]) for q in oracle}
    for lo, hi in ((0, 2), (2, 6)):            # two runs of the handle: the second starts behind record 0
        ids = contigs.ids[lo:hi]
        ssub, srb = bam.group_by_contig(contigs.ids, srefid, srr, ids)
        bsub, brb = bam.group_by_contig(contigs.ids, brefid, brr, ids)
        assert isinstance(ssub, abi.ResidentReads) and ssub.first == int(contigs.read_begin[lo]) and (lo == 0 or ssub.first > 0)
        np.testing.assert_array_equal(srb, brb)
        table = abi.ContigTable(length=contigs.length[lo:hi], species=contigs.species[lo:hi], read_begin=srb, ref=contigs.ref[off[lo]:off[hi]],
                                n_species=contigs.n_species)
        sb, bb = ctx.batch(table, ssub), ctx.batch(table, bsub)
        assert sb.info().path == bb.info().path
        for q in (0, 30, 51):                   # 51: above the clamp of a batch that holds clamped qualities -- that run takes the long path
            sc, sa, ss = _fetch(sb, _thr(q))
            bc, ba, bs = _fetch(bb, _thr(q))
            np.testing.assert_array_equal(sc, bc, err_msg="counts, baseq %d" % q)
            np.testing.assert_array_equal(sa, ba, err_msg="alleles, baseq %d" % q)
            np.testing.assert_array_equal(ss, bs, err_msg="counters, baseq %d" % q)
            np.testing.assert_array_equal(sc, oracle[q][2][off[lo]:off[hi]], err_msg="oracle counts, baseq %d" % q)
            np.testing.assert_array_equal(sa, oracle[q][3][off[lo]:off[hi]], err_msg="oracle alleles, baseq %d" % q)
            stats[q] += ss
        sb.close()
        bb.close()
    for q in oracle:
        np.testing.assert_array_equal(stats[q], oracle[q][4], err_msg="oracle counters, baseq %d" % q)


def test_a_70_kb_read_takes_the_long_path_and_matches_the_oracle(ctx, tmp_path):
    contigs, reads, _ = _sample(31, n_species=1, contigs_per_species=1, contig_len=80000, n_reads=300)
    ref = bytes(contigs.ref[100:70100]).decode().upper()
    one = H.reads_from_dicts([dict(pos=100, cigar=[(0, 70000)], seq=ref, qual=[30 + (k % 11) for k in range(70000)], nm=3, mapq=44, flag=0)])
    both = synth.concat_reads([reads, one])
    refid = np.zeros(both.n_reads, np.int32)
    sam = str(tmp_path / "long.sam")
    synth.write_sam(sam, contigs.ids, [80000], both, refid, order=np.random.default_rng(6).permutation(both.n_reads))
    table = abi.ContigTable(length=contigs.length, species=contigs.species, read_begin=[0, both.n_reads], ref=contigs.ref, n_species=1)
    st, _, oc, oa, os_ = c_oracle.pileup(_thr(30), table, both)
    # (the long read is kept: it covers the contig's middle, but for the reference's letters that are not A, C, G or T)
    assert st == 0 and int((oc[20000:60000].sum(axis=1) >= 1).sum()) > 39000
    _, _, srefid, srr = resident(ctx, sam)
    b = ctx.batch(table, srr)
    assert b.info().path == abi.PATH_LONG
    for want, got in zip((oc, oa, os_), _fetch(b, _thr(30))):
        np.testing.assert_array_equal(want, got)
    b.close()


# ---- 4. statuses -----------------------------------------------------------------------------------------------------------------
def _both_errors(ctx, path, chunk=None):
    out = []
    for res in (False, True):
        if chunk:
            os.environ["MIDAS_SNPS_SAM_CHUNK_BYTES"] = chunk
        try:
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.read_sam(path, ctx, resident=res)
        finally:
            os.environ.pop("MIDAS_SNPS_SAM_CHUNK_BYTES", None)
        out.append((ei.value.status, ei.value.message))
    return out


def test_refused_files_give_the_column_forms_status_and_text(ctx, tmp_path):
    path = str(tmp_path / "bad.sam")
    _write(path, [GOOD, GOOD, GOOD.replace(b"q\t0\t", b"q\t0x10\t")], head=HEAD)
    cols, res = _both_errors(ctx, path)
    assert cols == res and res[0] == abi.ERR_BAD_LAYOUT and "line 6:" in res[1] and "FLAG" in res[1]
    # two bad lines in different chunks: the first in file order wins, whatever chunk met it
    lines = [GOOD] * 40
    lines[31] = GOOD.replace(b"IIII", b"III")
    lines[9] = GOOD.replace(b"\tc\t", b"\tnope\t")
    _write(path, lines)
    for chunk in ("90", "700", None):
        cols, res = _both_errors(ctx, path, chunk)
        assert cols == res and res[0] == abi.ERR_BAD_LAYOUT and "line 13:" in res[1] and "RNAME" in res[1], res
    # a header error
    _write(path, [GOOD], head=b"@HD\tVN:1.6\n@SQ\tSN:c\n")
    cols, res = _both_errors(ctx, path)
    assert cols == res and res[0] == abi.ERR_BAD_LAYOUT and "line 2:" in res[1]


@pytest.mark.parametrize("edit,status", [
    (lambda l: l.replace(b"\tACGT\tIIII", b"\t*\t*"), abi.ERR_READ_NO_SEQ),
    (lambda l: l.replace(b"\tIIII", b"\t*"), abi.ERR_READ_NO_QUAL),
    (lambda l: l.replace(b"\tNM:i:0", b"\tNM:Z:0"), abi.ERR_READ_NO_NM),
])
def test_missing_seq_qual_nm_reach_the_pileups_own_message(ctx, tmp_path, edit, status):
    contigs, reads, refid = _sample(3, n_species=1, contigs_per_species=1, contig_len=900, n_reads=50)
    sam = str(tmp_path / "s.sam")
    synth.write_sam(sam, contigs.ids, [900], reads, refid)
    line = edit(GOOD.replace(b"\tc\t", b"\t" + contigs.ids[0].encode() + b"\t"))
    assert line != GOOD
    open(sam, "ab").write(line)
    table = abi.ContigTable(length=contigs.length, species=contigs.species, read_begin=[0, reads.n_reads + 1], ref=contigs.ref, n_species=1)
    seen = []
    for res in (True, False):
        _, _, _, decoded = abi.read_sam(sam, ctx, resident=res)
        assert isinstance(decoded, abi.ResidentReads) == res
        made = []
        with pytest.raises(abi.MidasSnpsError) as ei:
            made.append(ctx.batch(table, decoded))
            made[0].run(_thr(30))
            made[0].fetch()
        for b in made:
            b.close()
        seen.append((ei.value.status, ei.value.message, ei.value.read_index))
    assert seen[0] == seen[1] and seen[0][0] == status, seen


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def _run_pileup(out, db, env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_midas.py"), "snps", out, "--pileup", "-d", db, "-t", "4"],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, MIDAS_SNPS_TRACE="1", **env))


def test_pileup_over_a_sam_in_both_forms_writes_the_bam_runs_files(tmp_path):
    contigs, reads = synth.make_dataset(n_species=3, contigs_per_species=2, contig_len=6000, n_reads=5000, seed=19, var_len=True, lowercase_frac=0.05)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    db = str(tmp_path / "db")
    runs = {"bam": ({}, "(resident)"), "res": ({"MIDAS_SNPS_SAM_RESIDENT": "1"}, "SAM decoded and sorted on the device (resident)"),
            "col": ({"MIDAS_SNPS_SAM_RESIDENT": "0"}, "SAM decoded and sorted on the device (columns)")}
    for tag, (env, stage_line) in runs.items():
        d = str(tmp_path / tag)
        synth.write_sample(d, db, contigs, reads, sam=tag != "bam")
        if tag != "bam":      # unsorted, as the aligner leaves it
            synth.write_sam(os.path.join(d, "snps", "temp", "genomes.sam"), contigs.ids, [int(x) for x in contigs.length], reads, refid,
                            order=np.random.default_rng(5).permutation(reads.n_reads))
        r = _run_pileup(d, db, env)
        assert r.returncode == 0, r.stderr
        if tag != "bam":
            assert stage_line in r.stderr, r.stderr[-3000:]
    a = str(tmp_path / "bam")
    files = sorted(os.listdir(os.path.join(a, "snps", "output")))
    assert len(files) == 3
    for tag in ("res", "col"):
        b = str(tmp_path / tag)
        assert files == sorted(os.listdir(os.path.join(b, "snps", "output")))
        for f in files:
            assert gzip.open(os.path.join(a, "snps", "output", f), "rb").read() == gzip.open(os.path.join(b, "snps", "output", f), "rb").read(), (tag, f)
        assert open(os.path.join(a, "snps", "summary.txt")).read() == open(os.path.join(b, "snps", "summary.txt")).read(), tag


def test_two_ranks_with_only_a_sam_exit_together_as_before(tmp_path, monkeypatch):
    from tests.test_dist_gloo import ROOT as R, SNPS_WORKER, _run_snps_workers
    script = tmp_path / "snps_worker.py"
    script.write_text(SNPS_WORKER % {"root": R})
    contigs, reads = synth.make_dataset(n_species=2, contigs_per_species=2, contig_len=5000, n_reads=2000, seed=8)
    out, db = str(tmp_path / "s"), str(tmp_path / "db")
    synth.write_sample(out, db, contigs, reads, sam=True)
    monkeypatch.setenv("SNPS_REAL_DEVICE", "1")
    monkeypatch.setenv("MIDAS_SNPS_SAM_RESIDENT", "1")
    res = _run_snps_workers(tmp_path, script, out, db, 2)
    assert len(res) == 2
    for rc, o, e in res:
        assert rc != 0 and "2-rank runs need snps/temp/genomes.bam" in e, e[-1500:]
    assert not os.listdir(os.path.join(out, "snps", "output"))
