"""The direct layout's one byte per base (layout.h dense_byte) on the device: the pileup it feeds against the C oracle for base-quality
thresholds on both sides of the byte's 50 cap (a batch with a clamped A/C/G/T quality and a baseq above 50 goes the long way), the
read filter's mean quality from the stored sum of the TRUE qualities, and the resident decodes giving every read back byte for byte
-- the reads the byte cannot hold through the streamed decode's side buffer, including the group that finds it full."""
import numpy as np
import pytest

from midas_amd import abi, bam, synth
from oracle import c_oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        c.set_default_path(abi.PATH_DIRECT)
        yield c


def _same(ctx, thr, contigs, reads):
    st, er, oc, oa, os_ = c_oracle.pileup(thr, contigs, reads)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    b = ctx.batch(contigs, reads)
    assert b.info().path == abi.PATH_DIRECT
    b.run(thr)
    counts, allele, stats = b.fetch()
    b.close()
    bad = np.nonzero((counts != oc).any(axis=1))[0]
    assert bad.size == 0, "baseq %d: counts differ at %d sites, first %s: hip %s oracle %s" % (
        thr.baseq, bad.size, bad[:5], counts[bad[:5]].tolist(), oc[bad[:5]].tolist())
    np.testing.assert_array_equal(allele, oa)
    np.testing.assert_array_equal(stats, os_)
    return counts


def _reads(rng, L, n, quals, letters="ACGTACGTACGTNRYKM="):
    reads = []
    for _ in range(n):
        l = int(rng.integers(20, 160))
        shape = rng.integers(0, 3)
        if shape == 0:
            cigar = "%dM" % l
        elif shape == 1:
            s = int(rng.integers(1, 6))
            cigar = "%dS%dM" % (s, l - s)
        else:
            a = int(rng.integers(5, l - 5))
            cigar = "%dM%dD%dM" % (a, int(rng.integers(1, 20)), l - a)
        seq = "".join(rng.choice(list(letters), size=l))
        qual = [int(x) for x in rng.choice(quals, size=l)]
        if qual[0] == 255:
            qual[0] = 40          # (0xFF first: QUAL absent, which the reference raises on)
        reads.append(dict(pos=int(rng.integers(0, L - 200)), cigar=cigar, seq=seq, qual=qual, nm=int(rng.choice([0, 1, 2])),
                          mapq=int(rng.choice([42, 30, 3]))))
    reads.sort(key=lambda r: r["pos"])
    return H.reads_from_dicts(reads)


@pytest.mark.parametrize("baseq", [0, 1, 30, 50, 51, 52, 63, 93])
def test_direct_parity_across_the_quality_cap(ctx, baseq):
    rng = np.random.default_rng(71)
    L = 30000
    quals = np.array(list(range(0, 94)) + [49, 50, 51, 52, 53, 255] * 4)
    soa = _reads(rng, L, 3000, quals)
    contigs = H.single_contig(L, soa.n_reads, ref="".join(rng.choice(list("ACGTacgtN"), size=L)))
    for args in (dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=1.0, readq=0, aln_cov=0.0), dict(abi.DEFAULT_ARGS, baseq=baseq)):
        _same(ctx, abi.Thresholds.from_args(args), contigs, soa)


@pytest.mark.parametrize("baseq", [30, 51, 60])
def test_direct_parity_without_clamped_qualities(ctx, baseq):
    """Qualities <= 50 only: a baseq above the cap counts nothing, on the direct kernel itself."""
    rng = np.random.default_rng(72)
    L = 20000
    soa = _reads(rng, L, 2000, np.arange(0, 51))
    contigs = H.single_contig(L, soa.n_reads, ref="".join(rng.choice(list("ACGT"), size=L)))
    counts = _same(ctx, abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=1.0, readq=0, aln_cov=0.0)), contigs, soa)
    assert (int(counts.sum()) > 0) == (baseq <= 50)


def test_readq_boundary_on_qualities_above_the_cap(ctx):
    """np.mean(q) < readq on reads whose qualities lie above 50: the stored sum is of the true qualities, not the clamped bytes."""
    L = 5000
    reads = []
    for k in range(200):
        q = [60 + (k % 30)] * 100
        if k % 2:
            q[k % 100] -= 1       # mean just below 60 + (k % 30)
        reads.append(dict(pos=100 + 20 * k, cigar="100M", seq="ACGT" * 25, qual=q, nm=0, mapq=42))
    soa = H.reads_from_dicts(reads)
    contigs = H.single_contig(L, soa.n_reads, ref="ACGT" * (L // 4))
    for readq in (60, 61, 75, 89, 90):
        _same(ctx, abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=0, readq=readq)), contigs, soa)


def _exceptional_bam(tmp_path, seed, n_reads):
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=2, contig_len=40000, n_reads=n_reads, seed=seed, var_len=True)
    rng = np.random.default_rng(seed)
    qual = reads.qual.copy()
    seq4 = reads.seq4.copy()
    qual[:] = rng.choice(np.array(list(range(0, 94)) + [255], dtype=np.uint8), size=qual.size)
    l = np.diff(reads.qual_off)
    for i in rng.choice(reads.n_reads, reads.n_reads // 20, replace=False):     # QUAL absent
        qual[reads.qual_off[i]:reads.qual_off[i + 1]] = 0xFF
    iupac = rng.integers(0, seq4.size, seq4.size // 50)                        # IUPAC / '=' codes
    seq4[iupac] = (seq4[iupac] & 0x0F) | (rng.choice(np.array([0, 3, 5, 6, 9, 10, 12, 14], dtype=np.uint8), iupac.size) << 4)
    odd = np.nonzero(l % 2 == 1)[0]
    for i in odd[::3]:                                                         # a nonzero pad nibble
        seq4[reads.seq_off[i + 1] - 1] |= 0x07
    reads = abi.ReadsSoA(**{**reads.as_dict(), "qual": qual, "seq4": seq4})
    path = str(tmp_path / ("x%d.bam" % seed))
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    bam.write_bam(path, contigs.ids, [int(x) for x in contigs.length], refid, reads)
    return path, odd.size


@pytest.mark.parametrize("stream", ["0", "1"])
def test_fetch_payload_gives_exceptional_reads_back(ctx, tmp_path, monkeypatch, capfd, stream):
    path, n_odd = _exceptional_bam(tmp_path, 91, 40000)
    assert n_odd > 0
    _, _, _, host = abi.read_bam(path)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_STREAM", stream)
    if stream == "1":
        monkeypatch.setenv("MIDAS_SNPS_DECODE_GROUP_BLOCKS", "9")
    _, _, _, res = abi.read_bam(path, ctx, resident=True)
    err = capfd.readouterr().err
    if stream == "1":
        assert any(ln.startswith("[device decode] streamed:") and "groups of" in ln for ln in err.splitlines())
        assert "the side buffer grown" in err          # nearly every read is exceptional: the first room overflows
    down = ctx.fetch_payload(res)
    for k in abi._SOA_DTYPES:
        np.testing.assert_array_equal(getattr(host, k), getattr(down, k), err_msg=k)


@pytest.mark.parametrize("stream", ["0", "1"])
def test_fetch_payload_decodes_ordinary_reads(ctx, tmp_path, monkeypatch, capfd, stream):
    """Reads the bytes DO hold (qualities 0-50, A/C/G/T/N), a few exceptional ones among them: what comes back is the decode of the
    base bytes itself, not the side buffer's copies."""
    contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=2, contig_len=40000, n_reads=30000, seed=93, var_len=True)
    rng = np.random.default_rng(93)
    qual = rng.integers(0, 51, size=reads.qual.size).astype(np.uint8)
    seq4 = reads.seq4.copy()
    few = rng.choice(reads.n_reads, 60, replace=False)
    for i in few:                                                              # 0.2 % exceptional
        qual[reads.qual_off[i]] = 77
    reads = abi.ReadsSoA(**{**reads.as_dict(), "qual": qual, "seq4": seq4})
    path = str(tmp_path / "ordinary.bam")
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    bam.write_bam(path, contigs.ids, [int(x) for x in contigs.length], refid, reads)
    _, _, _, host = abi.read_bam(path)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_STREAM", stream)
    if stream == "1":
        monkeypatch.setenv("MIDAS_SNPS_DECODE_GROUP_BLOCKS", "9")
    _, _, _, res = abi.read_bam(path, ctx, resident=True)
    err = capfd.readouterr().err
    if stream == "1":
        assert any(ln.startswith("[device decode] streamed:") and "groups of" in ln for ln in err.splitlines())
        assert "the side buffer grown" not in err
    down = ctx.fetch_payload(res)
    for k in abi._SOA_DTYPES:
        np.testing.assert_array_equal(getattr(host, k), getattr(down, k), err_msg=k)
