"""SAM input, the parts that need no GPU: the text writer against the independent model (tests/sam_model.py), the committed
spec_fixture.sam against the columns of spec_fixture.bam, the command line (--sam), and the binding."""
import ctypes as C
import json
import os
import stat
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, build, synth
from tests import helpers as H
from tests import sam_model
from tests.sam_model import assert_columns_equal, reads_columns, sam_file_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_MIDAS = os.path.join(ROOT, "scripts", "run_midas.py")


def test_write_sam_round_trips_through_the_model(tmp_path):
    """Indels, clips, reads against lower-case reference bases, N: every record comes back as it was given, whatever the
    order of the lines; without NM tags nm is -1."""
    contigs, reads = synth.make_dataset(n_species=2, contigs_per_species=3, contig_len=4000, n_reads=1500, seed=5, var_len=True,
                                        lowercase_frac=0.05)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    lens = [int(x) for x in contigs.length]
    assert (np.asarray(reads.seq4) & 15 == 15).any() and len(set((np.asarray(reads.cigar) & 15).tolist())) >= 4
    order = np.random.default_rng(1).permutation(reads.n_reads)
    for tag, perm in (("sorted", None), ("shuffled", order)):
        path = str(tmp_path / (tag + ".sam"))
        synth.write_sam(path, contigs.ids, lens, reads, refid, order=perm)
        names, ref_lens, cols = sam_model.decode(open(path, "rb").read())
        assert names == list(contigs.ids) and ref_lens == lens
        came = sam_file_order(refid, np.asarray(reads.pos), np.arange(reads.n_reads) if perm is None else perm)
        assert_columns_equal(sam_model.reorder(cols, np.argsort(came)), reads_columns(refid, reads), tag)
    path = str(tmp_path / "no_nm.sam")
    synth.write_sam(path, contigs.ids, lens, reads, refid, with_nm=False)
    assert (sam_model.decode(open(path, "rb").read())[2]["nm"] == -1).all()
    text = open(str(tmp_path / "sorted.sam")).read().splitlines()
    assert text[1 + contigs.n_contigs].startswith("r0\t") and text[-1].endswith("\tYT:Z:UU") and "\tNM:i:" in text[-1]


def test_the_model_is_case_blind_and_reads_both_line_ends(tmp_path):
    head = b"@SQ\tSN:c\tLN:100\n"
    a = head + b"q\t0\tc\t5\t9\t4M\t*\t0\t0\tACGN\tIIII\tNM:i:1\n"
    b = head.replace(b"\n", b"\r\n") + b"q\t0\tc\t5\t9\t4M\t*\t0\t0\tacgn\tIIII\tXX:Z:NM:i:7\tNM:Z:x\tNM:i:1\tNM:i:9"
    ca, cb = sam_model.decode(a)[2], sam_model.decode(b)[2]
    assert_columns_equal(ca, cb)
    assert ca["seq4"].tolist() == [0x12, 0x4F] and ca["pos"].tolist() == [4] and ca["nm"].tolist() == [1]


def test_spec_fixture_sam_equals_the_bam_fixture():
    """The committed SAM twin of spec_fixture.bam (reversed lines) through the model = the BAM through the host decoder, once
    the two records that share (refID, pos) are put in the BAM's order."""
    with open(os.path.join(H.GOLDEN, "spec_fixture.json")) as f:
        n = len(json.load(f)["records"])
    names, lens, refid, reads = abi.read_bam(os.path.join(H.GOLDEN, "spec_fixture.bam"))
    sn, sl, cols = sam_model.decode(open(os.path.join(H.GOLDEN, "spec_fixture.sam"), "rb").read())
    assert sn == names and sl == lens and cols["refid"].size == n == reads.n_reads
    came = sam_file_order(np.asarray(refid), np.asarray(reads.pos), np.arange(n)[::-1])
    assert came.tolist() != list(range(n))         # (the tie at chrA:17 comes out in the SAM's order)
    assert_columns_equal(sam_model.reorder(cols, np.argsort(came)), reads_columns(refid, reads))


def test_the_committed_sam_fixture_is_what_its_generator_writes(tmp_path):
    src = open(os.path.join(H.GOLDEN, "make_sam_fixture.py")).read().replace("HERE, \"spec_fixture.sam\"", "%r, \"spec_fixture.sam\"" % str(tmp_path))
    g = dict(__name__="fixture", __file__=os.path.join(H.GOLDEN, "make_sam_fixture.py"))
    exec(compile(src, "make_sam_fixture.py", "exec"), g)
    g["main"]()
    assert open(str(tmp_path / "spec_fixture.sam"), "rb").read() == open(os.path.join(H.GOLDEN, "spec_fixture.sam"), "rb").read()


@pytest.mark.parametrize("text,line", [
    (b"@SQ\tSN:c\tLN:9\nq\t0\tc\t1\t0\t*\t*\t0\t0\t*\n", 2),                      # short line
    (b"@SQ\tSN:c\tLN:9\nq\t0\tc\t1\t0\t*\t*\t0\t0\t*\t*\nq\t7x\tc\t1\t0\t*\t*\t0\t0\t*\t*\n", 3),      # FLAG
    (b"@SQ\tSN:c\tLN:9\nq\t0\td\t1\t0\t*\t*\t0\t0\t*\t*\n", 2),                  # RNAME
    (b"@SQ\tSN:c\tLN:9\nq\t0\tc\t1\t0\t3M1Z\t*\t0\t0\tACGT\tIIII\n", 2),          # CIGAR op
    (b"@SQ\tSN:c\tLN:9\nq\t0\tc\t1\t0\t4M\t*\t0\t0\tACGT\tIII\n", 2),             # QUAL length
    (b"@HD\tVN:1.6\nq\t0\tc\t1\t0\t*\t*\t0\t0\t*\t*\n", 2),                      # record before @SQ
    (b"@SQ\tSN:c\n", 1), (b"@SQ\tSN:c\tLN:9\n@SQ\tSN:c\tLN:9\n", 2),
    (b"@SQ\tSN:c\tLN:12x\tLN:5\n", 1), (b"@SQ\tSN:\tSN:c\tLN:5\n", 1),        # only the first SN: / LN: of a line counts
])
def test_the_model_names_the_bad_line(text, line):
    with pytest.raises(sam_model.SamError) as ei:
        sam_model.decode(text)
    assert ei.value.line == line


def _run(argv, env=None):
    return subprocess.run([sys.executable, RUN_MIDAS] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


def test_help_shows_sam():
    r = _run(["snps", "-h"])
    assert r.returncode == 0 and "--sam" in r.stdout and "genomes.sam" in r.stdout and "skip samtools" in r.stdout


def _aligned_sample(tmp_path):
    """A sample as --build_db leaves it (genomes.fa, no alignments), reads to align, and a directory holding a stub bowtie2:
    two lines that record their argv and write a tiny SAM to the path behind -S."""
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=1, contig_len=500, n_reads=4, seed=2)
    out, db, bindir = str(tmp_path / "sample"), str(tmp_path / "db"), str(tmp_path / "bin")
    synth.write_sample(out, db, contigs, reads)
    os.remove(os.path.join(out, "snps", "temp", "genomes.bam"))
    os.makedirs(bindir)
    stub = os.path.join(bindir, "bowtie2")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\n"
                "echo \"$@\" > \"%s/argv.txt\"; while [ $# -gt 1 ]; do [ \"$1\" = -S ] && printf '@SQ\\tSN:c\\tLN:9\\n' > \"$2\"; shift; done\n" % bindir)
    os.chmod(stub, os.stat(stub).st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    fq = str(tmp_path / "reads.fq")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    env = dict(os.environ, PATH=bindir)        # (nothing else on it: no samtools)
    return out, db, bindir, fq, env


def test_align_with_sam_needs_bowtie2_alone(tmp_path):
    import shutil
    out, db, bindir, fq, env = _aligned_sample(tmp_path)
    if shutil.which("samtools", path=env["PATH"]):
        pytest.fail("the temporary PATH must not hold samtools")
    r = _run(["snps", out, "--align", "--sam", "-d", db, "-1", fq], env)
    assert r.returncode == 0, r.stderr
    argv = open(os.path.join(bindir, "argv.txt")).read().split()
    sam = os.path.join(out, "snps", "temp", "genomes.sam")
    assert argv[argv.index("-S") + 1] == sam and "--no-unal" in argv and "--very-sensitive" in argv and argv[argv.index("-U") + 1] == fq
    assert open(sam).read() == "@SQ\tSN:c\tLN:9\n"
    assert not os.path.exists(os.path.join(out, "snps", "temp", "genomes.bam"))
    log = open(os.path.join(out, "snps", "log.txt")).read()
    assert "genomes.sam" in log and "samtools view" not in log
    assert "genomes.sam" in open(os.path.join(out, "snps", "readme.txt")).read()


def test_align_with_sam_refuses_to_leave_an_older_bam_in_the_pileups_way(tmp_path):
    out, db, bindir, fq, env = _aligned_sample(tmp_path)
    bam = os.path.join(out, "snps", "temp", "genomes.bam")
    open(bam, "wb").write(b"older")
    r = _run(["snps", out, "--align", "--sam", "-d", db, "-1", fq], env)
    assert r.returncode != 0 and "genomes.bam exists and --pileup reads it in preference to genomes.sam" in r.stderr
    assert not os.path.exists(os.path.join(bindir, "argv.txt"))


def test_align_without_sam_still_asks_for_samtools(tmp_path):
    out, db, bindir, fq, env = _aligned_sample(tmp_path)
    r = _run(["snps", out, "--align", "-d", db, "-1", fq], env)
    assert r.returncode != 0
    assert "\nError: bowtie2 / samtools not found on PATH (needed for --align; the aligner is not part of this build)\n" in r.stderr
    assert not os.path.exists(os.path.join(bindir, "argv.txt"))


def test_pileup_without_any_alignment_keeps_its_message(tmp_path):
    out, db, bindir, fq, env = _aligned_sample(tmp_path)
    r = _run(["snps", out, "--pileup", "-d", db], env)
    assert r.returncode != 0 and "You've specified --pileup, but no alignments were found" in r.stderr


def test_read_sam_without_a_device_context_is_invalid_arg():
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.read_sam(os.path.join(H.GOLDEN, "spec_fixture.sam"))
    assert ei.value.status == abi.ERR_INVALID_ARG
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.read_sam(os.path.join(H.GOLDEN, "spec_fixture.sam"), ctx=object())
    assert ei.value.status == abi.ERR_INVALID_ARG


def test_the_library_exports_the_sam_entry_points():
    assert "midas_sam_load_device" in abi.SAM_SYMBOLS
    lib = C.CDLL(build.build_native())
    header = open(os.path.join(ROOT, "include", "midas_snps.h")).read()
    for sym in abi.SAM_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert "int32_t %s(" % sym in header, sym
    assert b"sam_fields_kernel" in open(build.LIB_PATH, "rb").read()
    # a null context is refused before anything is touched
    bound = abi.load_library(build_if_missing=False)
    h = C.c_void_p()
    n = C.c_int64()
    assert bound.midas_sam_load_device(b"x.sam", None, C.byref(h), C.byref(n), C.byref(n), C.byref(n), C.byref(n), None) == abi.ERR_INVALID_ARG
