"""`run_midas.py genes --sam` on the GPU: the SAM decode in file order (midas_sam_load_device_order) against the independent
model, the per-read facts made on the device (genes_facts_kernel behind midas_genes_count_device) against the host's
pack_records route and against oracle/genes_oracle.py, and the command over a pangenomes.sam.  Every comparison is exact:
counts as integers, depths by repr() or by their bytes, statuses with the index of the first offending read."""
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, synth
from oracle import genes_oracle as go
from tests import helpers as H
from tests import sam_model
from tests.sam_model import assert_columns_equal, reads_columns
from tests.test_genes_sam_host import file_order_columns
from tests.test_gpu_genes import GENES_ARGS, _oracle, _oracle_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD_SETS = [GENES_ARGS, dict(mapid=97.0, readq=32, mapq=25, aln_cov=0.95), dict(mapid=1.0, readq=0, mapq=0, aln_cov=0.0)]
PERMISSIVE = THRESHOLD_SETS[2]


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _thr(args):
    return abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, **args))


def _columns(ctx, refid, reads):
    assert reads.device is not None and reads.qual.size == 0
    return reads_columns(refid, ctx.fetch_payload(reads))


# ---- file order ---------------------------------------------------------------------------------------------------------------

def _shuffled_sam(tmp_path):
    """A few hundred reads over four contigs, every ninth without a reference, the lines shuffled against coordinate order."""
    contigs, reads = synth.make_dataset(n_species=2, contigs_per_species=2, contig_len=3000, n_reads=420, seed=77, var_len=True)
    refid = np.repeat(np.arange(contigs.n_contigs, dtype=np.int32), np.diff(contigs.read_begin))
    refid[::9] = -1
    path = str(tmp_path / "shuffled.sam")
    synth.write_sam(path, contigs.ids, [int(x) for x in contigs.length], reads, refid, order=np.random.default_rng(4).permutation(reads.n_reads))
    return path, int((refid >= 0).sum())


def test_file_order_keeps_the_lines_order(ctx, tmp_path, monkeypatch):
    path, n_kept = _shuffled_sam(tmp_path)
    names, lens, exp = file_order_columns(open(path, "rb").read())
    assert exp["refid"].size == n_kept and (np.diff(exp["refid"].astype(np.int64) << 32 | exp["pos"]) < 0).any()
    mn, ml, refid, reads = abi.read_sam(path, ctx, order='file')
    assert mn == names and ml == lens
    got = _columns(ctx, refid, reads)
    assert_columns_equal(got, exp, "file order")
    monkeypatch.setenv("MIDAS_SNPS_SAM_CHUNK_BYTES", "64")           # smaller than a line: it grows, and every chunk appends
    _, _, refid, reads = abi.read_sam(path, ctx, order='file')
    assert_columns_equal(_columns(ctx, refid, reads), exp, "file order, 64-byte chunks")


def _read_sam_by_the_new_entry(ctx, path, order):
    lib = abi.load_library()
    h, err = C.c_void_p(), C.create_string_buffer(256)
    n, sb, qb, nc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    st = lib.midas_sam_load_device_order(path.encode(), ctx._h, order, C.byref(h), C.byref(n), C.byref(sb), C.byref(qb), C.byref(nc), err)
    if st != 0:
        raise abi.MidasSnpsError(st, err.value.decode())
    owner = abi._BamOwner(lib, h)
    names, lens = abi._bam_refs(lib, h)
    return (names, lens) + abi._bam_columns(lib, h, int(n.value), int(sb.value), int(qb.value), int(nc.value), owner, on_device=True)


def test_coordinate_order_through_the_new_entry_is_the_old_entrys(ctx, tmp_path):
    path, _ = _shuffled_sam(tmp_path)
    n0, l0, r0, reads0 = abi.read_sam(path, ctx)                                   # midas_sam_load_device
    n1, l1, r1, reads1 = _read_sam_by_the_new_entry(ctx, path, abi.SAM_ORDERS['coordinate'])
    assert n0 == n1 and l0 == l1
    a, b = _columns(ctx, r0, reads0), _columns(ctx, r1, reads1)
    for k in sam_model.COLUMNS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert_columns_equal(b, sam_model.decode(open(path, "rb").read())[2], "coordinate order")
    with pytest.raises(abi.MidasSnpsError) as ei:
        _read_sam_by_the_new_entry(ctx, path, 2)
    assert ei.value.status == abi.ERR_INVALID_ARG


def test_an_empty_body_decodes_to_zero_reads(ctx, tmp_path):
    path = str(tmp_path / "empty.sam")
    for body in (b"", b"q\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n"):
        open(path, "wb").write(b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:900\n@SQ\tSN:d\tLN:50\n" + body)
        names, lens, refid, reads = abi.read_sam(path, ctx, order='file')
        assert names == ["c", "d"] and lens == [900, 50] and refid.size == 0 and reads.n_reads == 0
        assert reads.seq_off.tolist() == [0] and reads.qual_off.tolist() == [0] and reads.cigar_off.tolist() == [0]
        aligned, mapped, depth, _ = ctx.genes_count_device(_thr(GENES_ARGS), reads, refid, lens)
        assert aligned.tolist() == [0, 0] and mapped.tolist() == [0, 0] and depth.tolist() == [0.0, 0.0]


# ---- parity of the facts kernel ---------------------------------------------------------------------------------------------------

def _device_routes(ctx, tmp_path, names, lens, refid, reads):
    """The reads as the device holds them by both decoders: (route name, refid, ReadsSoA with device payload)."""
    sam, bam = str(tmp_path / "r.sam"), str(tmp_path / "r.bam")
    synth.write_sam(sam, names, lens, reads, refid)
    abi.write_bam(bam, names, lens, refid, reads)
    _, _, rs, ds = abi.read_sam(sam, ctx, order='file')
    _, _, rb, db = abi.read_bam(bam, ctx, payload_on_device=True)
    assert ds.device is not None and db.device is not None
    return [("sam", rs, ds), ("bam", rb, db)]


@pytest.fixture(scope="module")
def parity(ctx, tmp_path_factory):
    ds = synth.make_pangenome_dataset(n_species=3, genes_per_species=80, n_reads=6000, seed=101)
    lengths = [len(s) for s in ds['gene_seq']]
    routes = _device_routes(ctx, tmp_path_factory.mktemp("parity"), ds['gene_ids'], lengths, ds['refid'], ds['reads'])
    return ds, lengths, routes


@pytest.mark.parametrize("k", range(len(THRESHOLD_SETS)))
def test_three_routes_and_the_oracle_agree(ctx, parity, k):
    ds, lengths, routes = parity
    args = THRESHOLD_SETS[k]
    exp_aligned, exp_mapped, exp_depth, _, _ = _oracle(ds, args)
    host = ctx.genes_count(_thr(args), ds['reads'], ds['refid'], lengths)
    assert host[0].tolist() == exp_aligned and host[1].tolist() == exp_mapped
    assert [repr(float(x)) for x in host[2]] == [repr(float(x)) for x in exp_depth]
    assert sum(exp_mapped) > 0
    for name, refid, reads in routes:
        assert np.array_equal(refid, ds['refid']), name
        aligned, mapped, depth, ms = ctx.genes_count_device(_thr(args), reads, refid, lengths)
        assert aligned.tolist() == exp_aligned and mapped.tolist() == exp_mapped, name
        assert [repr(float(x)) for x in depth] == [repr(float(x)) for x in exp_depth], name
        assert ms > 0
        timing = ctx.genes_count_timing()
        assert timing['facts kernel'] > 0 and timing['filter + sort + sums'] > 0
        # a second call on the same context gives the same answer (no state carried over)
        again = ctx.genes_count_device(_thr(args), reads, refid, lengths)
        assert np.array_equal(again[0], aligned) and np.array_equal(again[1], mapped) and again[2].tobytes() == depth.tobytes(), name


def test_one_hot_gene_keeps_file_order(ctx, tmp_path):
    """5 200 reads on one gene (more than a thread sums: the wave kernel takes it): one long sequential fp64 sum."""
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=8, n_reads=5200, seed=7, silent_fraction=0.0)
    refid = np.full_like(ds['refid'], 3)
    lengths = [len(s) for s in ds['gene_seq']]
    assert refid.size >= 5000
    recs = [(3,) + r[1:] for r in _oracle_records(ds['reads'], refid)]
    exp_aligned, exp_mapped, exp_depth, _ = go.count_mapped_bp(GENES_ARGS, recs, ds['gene_ids'], ds['gene_species'], lengths)
    assert exp_mapped[3] > 2048
    for name, rid, reads in _device_routes(ctx, tmp_path, ds['gene_ids'], lengths, refid, ds['reads']):
        aligned, mapped, depth, _ = ctx.genes_count_device(_thr(GENES_ARGS), reads, rid, lengths)
        assert aligned.tolist() == exp_aligned and mapped.tolist() == exp_mapped, name
        assert [repr(float(x)) for x in depth] == [repr(float(x)) for x in exp_depth], name


# ---- edge reads, hand-made -------------------------------------------------------------------------------------------------------

MAX_L = 1024          # kMaxLSeq: the longest read a record holds
_ZERO = (10, "10S", 0)          # everything clipped: keep_read divides by an aligned length of 0
EDGE_THRESHOLDS = [THRESHOLD_SETS[2], GENES_ARGS, dict(mapid=90.0, readq=10, mapq=5, aln_cov=0.5), dict(mapid=1.0, readq=25, mapq=0, aln_cov=0.0),
                   dict(mapid=1.0, readq=30, mapq=20, aln_cov=0.9)]


def _edge_cases():
    """[(l_seq, CIGAR, aligned length by pysam's rules, worked out by hand)]: the lengths around the sixteen-byte granule and
    the sixteen-lane step, the longest supported one, the CIGAR shapes, and a staircase of lengths so that quality runs start at
    every offset mod 16."""
    cases = [(l, "%dM" % l, l) for l in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, MAX_L)]
    cases += [(50, "*", 50), (50, "50M", 50), (50, "5S45M", 45), (50, "45M5S", 45), (48, "2H3S40M5S2H", 40), (50, "3S2I40M5S", 42),
              (50, "5H45M5S", 45),
              (50, "5S", 45)]          # one op: the start hops over it, the backward walk never inspects op 0, so the end stays l_seq
    cases += [(l, "%dM" % l, l) for l in range(1, 33)]        # 1 + 2 + 3 + ...: the running offset visits every residue mod 16
    cases += [(MAX_L, "%dS%dM" % (7, MAX_L - 7), MAX_L - 7), (33, "33M", 33)]
    return cases


def _make_edge(cases, seed=5):
    rng = np.random.default_rng(seed)
    dicts = []
    for k, (l, cg, _) in enumerate(cases):
        mean = int(rng.integers(3, 41))
        q = np.clip(rng.integers(mean - 3, mean + 4, l), 0, 93)
        dicts.append(dict(pos=k, cigar=[] if cg == "*" else cg, seq="".join("ACGT"[int(x)] for x in rng.integers(0, 4, l)),
                          qual=[int(x) for x in q], nm=int(rng.integers(0, 3)) if l >= 4 else 0, mapq=int(rng.integers(0, 60)), flag=0))
    return H.reads_from_dicts(dicts)


def test_edge_reads_one_read_a_gene(ctx, tmp_path):
    """One read a gene, so a gene's depth IS its read's term: the device route against midas_genes_terms over the host copy, and
    both against the hand-derived aligned lengths through the oracle's keep_read."""
    cases = _edge_cases()
    reads = _make_edge(cases)
    n = reads.n_reads
    assert set((np.asarray(reads.qual_off[:-1]) % 16).tolist()) == set(range(16))
    refid = np.arange(n, dtype=np.int32)
    names, lengths = ["g%d" % i for i in range(n)], [1000 + 7 * i for i in range(n)]
    quals = [reads.qual[int(reads.qual_off[i]):int(reads.qual_off[i + 1])].tolist() for i in range(n)]
    for name, rid, dreads in _device_routes(ctx, tmp_path, names, lengths, refid, reads):
        assert int(dreads.qual_off[n]) == int(reads.qual_off[n])          # (the last read ends exactly at the column's end)
        host = ctx.fetch_payload(dreads)
        assert_columns_equal(reads_columns(rid, host), reads_columns(refid, reads), name)
        seen = set()
        for args in EDGE_THRESHOLDS:
            exp = np.array([c[2] / float(lengths[i]) if go.keep_read(c[2], c[0], int(reads.nm[i]), quals[i], int(reads.mapq[i]), args['mapid'],
                                                                      args['readq'], args['mapq'], args['aln_cov']) else 0.0
                            for i, c in enumerate(cases)], np.float64)
            term = ctx.genes_terms(_thr(args), host, rid, lengths)
            aligned, mapped, depth, _ = ctx.genes_count_device(_thr(args), dreads, rid, lengths)
            assert aligned.tolist() == [1] * n, name
            assert depth.tobytes() == term.tobytes() and mapped.tolist() == (term > 0).astype(np.int64).tolist(), (name, args)
            assert depth.tobytes() == exp.tobytes(), (name, args)
            seen.add(int(mapped.sum()))
        assert n in seen and len(seen) >= 4          # (nothing filtered once; the other thresholds cut through the set: qmean and mapq are seen)


def test_a_read_of_clips_alone_has_aligned_length_zero(ctx, tmp_path):
    """`10S` and nothing else: pysam's start hops over it (10), its end never looks at op 0 (10): aligned length 0."""
    reads = _make_edge([(20, "20M", 20), _ZERO, (20, "20M", 20)])
    refid = np.arange(3, dtype=np.int32)
    for name, rid, dreads in _device_routes(ctx, tmp_path, ["a", "b", "c"], [500, 600, 700], refid, reads):
        with pytest.raises(abi.MidasSnpsError) as eh:
            ctx.genes_count(_thr(PERMISSIVE), ctx.fetch_payload(dreads), rid, [500, 600, 700])
        with pytest.raises(abi.MidasSnpsError) as ed:
            ctx.genes_count_device(_thr(PERMISSIVE), dreads, rid, [500, 600, 700])
        assert (ed.value.status, ed.value.read_index) == (eh.value.status, eh.value.read_index) == (abi.ERR_READ_ZERO_ALIGN, 1), name


# ---- statuses -------------------------------------------------------------------------------------------------------------------

VICTIMS = (201, 433)


def _status_case(what):
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=12, n_reads=800, seed=11)
    reads, refid = ds['reads'], ds['refid'].copy()
    lengths = [len(s) for s in ds['gene_seq']]
    assert reads.n_reads > VICTIMS[1] + 10
    if what in ("seq", "long"):
        L = 0 if what == "seq" else MAX_L + 1
        one = H.reads_from_dicts([dict(pos=5, cigar=[] if L == 0 else "%dM" % L, seq="A" * L, qual=[30] * L, nm=0, mapq=40, flag=0)])
        n = reads.n_reads
        parts = [synth.take_reads(reads, np.arange(0, VICTIMS[0])), one, synth.take_reads(reads, np.arange(VICTIMS[0] + 1, VICTIMS[1])), one,
                 synth.take_reads(reads, np.arange(VICTIMS[1] + 1, n))]
        reads = synth.concat_reads(parts)
    for v in VICTIMS:
        if what == "nm":
            reads.nm[v] = -1
        elif what == "qual":
            reads.qual[int(reads.qual_off[v]):int(reads.qual_off[v + 1])] = 0xFF
        elif what == "align":
            c0 = int(reads.cigar_off[v])
            reads.cigar[c0:int(reads.cigar_off[v + 1])] = 0
            reads.cigar[c0] = (int(reads.l_seq[v]) << 4) | 4
        elif what == "gene":
            refid[v] = len(lengths)
    return ds['gene_ids'], lengths, refid, reads


@pytest.mark.parametrize("what,status", [("seq", abi.ERR_READ_NO_SEQ), ("nm", abi.ERR_READ_NO_NM), ("align", abi.ERR_READ_ZERO_ALIGN),
                                         ("qual", abi.ERR_READ_NO_QUAL), ("long", abi.ERR_UNSUPPORTED), ("gene", abi.ERR_BAD_LAYOUT)])
def test_statuses_are_the_hosts_with_the_first_bad_read(ctx, tmp_path, what, status):
    names, lengths, refid, reads = _status_case(what)
    file_refid = np.where(refid < len(lengths), refid, 0).astype(np.int32)       # (a gene outside the table cannot be written: it goes in through ref_id)
    for name, rid, dreads in _device_routes(ctx, tmp_path, names, lengths, file_refid, reads):
        assert np.array_equal(rid, file_refid)
        host = ctx.fetch_payload(dreads)
        with pytest.raises(abi.MidasSnpsError) as eh:
            ctx.genes_count(_thr(PERMISSIVE), host, refid, lengths)
        with pytest.raises(abi.MidasSnpsError) as ed:
            ctx.genes_count_device(_thr(PERMISSIVE), dreads, refid, lengths)
        assert (ed.value.status, ed.value.read_index) == (eh.value.status, eh.value.read_index) == (status, VICTIMS[0]), name
        assert ed.value.message == eh.value.message


def test_a_malformed_read_comes_before_the_filters_own_statuses(ctx, tmp_path):
    """The host makes every record before the filter sees one: a read no record can be made of wins over an earlier read the
    filter would raise on."""
    names, lengths, refid, reads = _status_case("nm")               # reads 201 and 433 have no NM ...
    refid[VICTIMS[1] + 5] = len(lengths)                            # ... and a later one is on no gene
    file_refid = np.where(refid < len(lengths), refid, 0).astype(np.int32)
    for name, rid, dreads in _device_routes(ctx, tmp_path, names, lengths, file_refid, reads):
        with pytest.raises(abi.MidasSnpsError) as eh:
            ctx.genes_count(_thr(PERMISSIVE), ctx.fetch_payload(dreads), refid, lengths)
        with pytest.raises(abi.MidasSnpsError) as ed:
            ctx.genes_count_device(_thr(PERMISSIVE), dreads, refid, lengths)
        assert (ed.value.status, ed.value.read_index) == (eh.value.status, eh.value.read_index) == (abi.ERR_BAD_LAYOUT, VICTIMS[1] + 5), name


# ---- the command ------------------------------------------------------------------------------------------------------------------

def _run_cli(out, db, fq, extra=()):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_midas.py"), "genes", out, "--call_genes",
                           "-d", db, "-1", fq] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _fastq(tmp_path):
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as h:
        h.write("@r1\nACGT\n+\nIIII\n")
    return fq


def _outputs(out, species_ids):
    return ([gzip.open(os.path.join(out, "genes", "output", sp + ".genes.gz"), "rb").read() for sp in species_ids],
            open(os.path.join(out, "genes", "summary.txt"), "rb").read())


def test_call_genes_over_a_sam_writes_the_oracles_and_the_bam_runs_files(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=3, genes_per_species=40, n_reads=6000, seed=23)
    a, b, both, db = str(tmp_path / "bam"), str(tmp_path / "sam"), str(tmp_path / "both"), str(tmp_path / "db")
    synth.write_pangenome_sample(a, db, ds)
    synth.write_pangenome_sample(b, db, ds, sam=True)
    temp = os.path.join(b, "genes", "temp")
    assert os.path.isfile(os.path.join(temp, "pangenomes.sam")) and not os.path.exists(os.path.join(temp, "pangenomes.bam"))
    # both files, the SAM unusable: the BAM wins and the SAM is never opened
    shutil.copytree(a, both)
    bad = os.path.join(both, "genes", "temp", "pangenomes.sam")
    open(bad, "wb").write(b"not a SAM file\n")
    os.chmod(bad, 0)
    fq = _fastq(tmp_path)
    for d in (a, b, both):
        r = _run_cli(d, db, fq)
        assert r.returncode == 0, r.stderr
        assert "Computing coverage of pangenomes" in r.stdout
    _, _, _, tables, summary = _oracle(ds, GENES_ARGS)
    for d in (a, b, both):
        for sp in ds['species_ids']:
            assert gzip.open(os.path.join(d, "genes", "output", sp + ".genes.gz"), "rt").read() == tables[sp], (d, sp)
        assert open(os.path.join(d, "genes", "summary.txt")).read() == summary, d
    assert _outputs(a, ds['species_ids']) == _outputs(b, ds['species_ids']) == _outputs(both, ds['species_ids'])


def test_a_read_without_nm_exits_naming_its_index_in_the_sam(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=1, genes_per_species=12, n_reads=600, seed=29)
    ds['reads'].nm[41] = -1
    out, db = str(tmp_path / "sample"), str(tmp_path / "db")
    synth.write_pangenome_sample(out, db, ds, sam=True)
    # records without a reference in front of it do not count: the index is the BAM's
    sam = os.path.join(out, "genes", "temp", "pangenomes.sam")
    lines = open(sam, "rb").read().split(b"\n")
    first = next(k for k, l in enumerate(lines) if not l.startswith(b"@"))
    lines[first:first] = [b"u%d\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII" % k for k in range(3)]
    open(sam, "wb").write(b"\n".join(lines))
    r = _run_cli(out, db, _fastq(tmp_path))
    assert r.returncode == 1
    assert "NM" in r.stderr and "[read 41 of the SAM]" in r.stderr


def test_two_ranks_with_only_a_sam_exit_together(tmp_path):
    from tests.test_dist_gloo import GENES_WORKER, _free_port
    ds = synth.make_pangenome_dataset(n_species=2, genes_per_species=8, n_reads=300, seed=8)
    out, db = str(tmp_path / "s"), str(tmp_path / "db")
    synth.write_pangenome_sample(out, db, ds, sam=True)
    script = tmp_path / "genes_worker.py"
    script.write_text(GENES_WORKER % {"root": ROOT})
    env1 = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env1["GENES_REAL_DEVICE"] = "1"               # (the ranks share device 0)
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, str(script), out, db], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(env1, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for k in range(2)]
    for p in procs:
        o, e = p.communicate(timeout=300)
        assert p.returncode != 0 and "2-rank runs need genes/temp/pangenomes.bam" in e, e[-1500:]
    assert not os.listdir(os.path.join(out, "genes", "output"))
