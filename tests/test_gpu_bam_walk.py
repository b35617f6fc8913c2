"""The device BAM record walk (bam_walk.hip, decode_plan.h stitch_chunks, bam_device.hip WalkTables::walk_again) on files that make
its guesses WRONG.  A chunk's thread takes the first offset from which four records in a row look plausible; the host stitches the
chunks and has every chunk whose guess the true chain does not hit walked a second time.  On plain files every guess is right
(profiles/genes_bam.txt records `chunks_again 0` at every size: that is what plain files give; `decoy4`, `refused_names`,
`long_record` and `everywhere` here are the files on which the count is not zero), so the second walk, the replacement of a
chunk's results after it, the `v == total` rule at a segment's end and the chunks without any record start run here and nowhere
else.

The fixtures and the sequential model that predicts the walk are tests/bam_walk_model.py; tests/test_bam_walk_model_host.py proves
on the CPU that every fixture does what its name says.  The files are valid BAMs -- pysam and the host decode read them without
complaint -- so every route of the device decode must return exactly what was written: one arena, the one-pass genes count, the
streamed decode, a rank's slices, and `run_midas.py snps` as one process and as two ranks.  Everything is compared exactly, and the
number of second walks the device reports is the model's.

Second walks, the device's count next to the model's (one arena / genes count; they lay the same grid from the header's end):
decoy4 36 / 36, decoy3 0 / 0, refused_names 49 / 49, end_decoy 0 / 0 (the chain from the header's end stands at the stream's end
when it comes to the last chunk: the decoy is guessed, the chunk emptied, nothing walked again), long_record 1 / 1, everywhere
36 / 36, every borders_* and short_tail_* 0 / 0; streamed in groups of five blocks: decoy4 8 / 8, everywhere 41 / 41; the slices
k of n: everywhere 0/2 17 / 17, 1/2 14 / 14, 0/3 11 / 11 (1/3 and 2/3: the walk from the guessed first record turns bad, in the
model as on the device, and the host's walk decides), decoy4 0/2 20 / 20, 0/3 13 / 13, its other slices and end_decoy's 0 / 0."""
import os
import re
import shutil

import numpy as np
import pytest

from midas_amd import abi, synth
from tests import bam_walk_model as M
from tests.test_gpu_genes import GENES_ARGS
from tests.test_gpu_genes_sam import _thr

pytestmark = pytest.mark.gpu

BUILDERS = dict([("decoy4", M.decoy4), ("decoy3", M.decoy3), ("refused_names", M.refused_names)]
                + [("borders_%s" % d, lambda tmp, d=d: M.borders(tmp, d)) for d in M.BORDER_DISTANCES + ("end",)]
                + [("short_tail_%s" % k, lambda tmp, k=k: M.short_tail(tmp, k)) for k in M.SHORT_TAILS]
                + [("end_decoy", M.end_decoy), ("long_record", M.long_record), ("everywhere", M.everywhere)])

@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    """name -> Fixture, each written and modelled once for the module"""
    tmp, made = tmp_path_factory.mktemp("bam_walk"), {}

    def get(name):
        if name not in made:
            made[name] = BUILDERS[name](tmp)
        return made[name]
    return get


def _same_columns(got, want, what):
    for k in abi._SOA_DTYPES:
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg="%s: %s" % (what, k))


def _walked_again(err):
    """the numbers of the one-arena decode's trace lines `[device decode] N chunk(s) walked again`"""
    return [int(m.group(1)) for m in re.finditer(r"^\[device decode\] (\d+) chunk\(s\) walked again$", err, re.M)]


# ---- (a) one arena ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BUILDERS))
def test_one_arena_returns_what_was_written(ctx, fixtures, monkeypatch, capfd, name):
    fx = fixtures(name)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_STREAM", "0")
    capfd.readouterr()
    names, lens, refid, res = abi.read_bam(fx.path, ctx, resident=True)
    err = capfd.readouterr().err
    assert "[device decode] streamed:" not in err
    again = _walked_again(err)
    print("%s: one arena: %s chunk(s) walked again, the model %d" % (name, again, fx.again))
    assert names == fx.ref_names and lens == fx.ref_lens
    np.testing.assert_array_equal(refid, fx.refid)
    assert res.n_reads == fx.reads.n_reads
    down = ctx.fetch_payload(res)
    _same_columns(down, fx.reads, "one arena against what was written")
    _, _, refid_h, host = abi.read_bam(fx.path)
    np.testing.assert_array_equal(refid, refid_h)
    _same_columns(down, host, "one arena against the host decode")
    assert again == ([fx.again] if fx.again else [])           # (no second walk: no line)


# ---- (b) the one-pass genes count ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BUILDERS))
def test_genes_count_bam_counts_the_same_records(ctx, fixtures, name):
    """midas_genes_count_bam decodes the whole file as ONE segment from the header's end (bam_host.cpp decode_whole_file: seg.from =
    rec_begin, exact) -- the grid of the model's whole_file(), so `chunks_again` is the model's count itself."""
    fx = fixtures(name)
    thr = _thr(GENES_ARGS)
    _, _, refid, reads = abi.read_bam(fx.path)
    host = host_error = None
    try:
        host = ctx.genes_count(thr, reads, refid, fx.ref_lens)[:3]
    except abi.MidasSnpsError as e:
        host_error = e
    # (a record of 100 000 bases is beyond the genes record's fields: both routes refuse it, with the same status and read)
    assert (host_error is not None) == (name == "long_record")
    h = abi.open_bam_device(fx.path, ctx)
    try:
        if host_error is not None:
            with pytest.raises(abi.MidasSnpsError) as ed:
                ctx.genes_count_bam(thr, h, fx.ref_lens)
            assert (ed.value.status, ed.value.read_index) == (host_error.status, host_error.read_index) == (abi.ERR_UNSUPPORTED, M.LONG_AT)
        else:
            got = ctx.genes_count_bam(thr, h, fx.ref_lens)
            assert got[0].tolist() == host[0].tolist() and got[1].tolist() == host[1].tolist() and got[2].tobytes() == host[2].tobytes()
            assert int(got[0].sum()) == fx.reads.n_reads and int(got[1].sum()) > 0
        stats = ctx.genes_count_bam_timing()[1]
    finally:
        h.close()
    print("%s: genes count: %d chunk(s) walked again, the model %d" % (name, stats["chunks_again"], fx.again))
    assert stats["records"] == fx.reads.n_reads and stats["dropped"] == fx.dropped
    assert stats["inflated_bytes"] == fx.total and stats["chunks"] == len(fx.chunks)
    assert stats["chunks_again"] == fx.again


# ---- (c) the streamed decode --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["everywhere", "decoy4"])
def test_streamed_decode_returns_what_was_written(ctx, fixtures, monkeypatch, capfd, name):
    fx = fixtures(name)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_STREAM", "1")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_GROUP_BLOCKS", "5")
    monkeypatch.setenv("MIDAS_SNPS_DECODE_SLOTS", "2")
    capfd.readouterr()
    _, _, refid, res = abi.read_bam(fx.path, ctx, resident=True)
    err = capfd.readouterr().err
    groups = [int(m.group(1)) for m in re.finditer(r"^\[device decode\] streamed: (\d+) groups of", err, re.M)]
    again = [int(m.group(1)) for m in re.finditer(r"^\[device decode\] streamed: \d+ records in .*; (\d+) chunk\(s\) walked again;", err, re.M)]
    want_groups, want_again, want_offsets = M.streamed(fx.path, fx.stream, 5)
    print("%s: streamed: %s groups, %s chunk(s) walked again, the model %d and %d" % (name, groups, again, want_groups, want_again))
    assert want_offsets == fx.offsets
    assert len(groups) == 1 and groups[0] >= 3 and groups[0] == want_groups
    np.testing.assert_array_equal(refid, fx.refid)
    assert res.n_reads == fx.reads.n_reads
    _same_columns(ctx.fetch_payload(res), fx.reads, "streamed against what was written")
    assert len(again) == 1 and again[0] == want_again
    if name == "everywhere":
        assert again[0] > 0


# ---- (d) a rank's slices ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", ["everywhere", "decoy4", "end_decoy"])
def test_device_slices_stand_on_true_records(ctx, fixtures, monkeypatch, capfd, name, n):
    fx = fixtures(name)
    offsets, starts = fx.truth["offset"], fx.true_starts()
    kept_offsets = np.array(fx.offsets, np.int64)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    end_before, seen = None, []
    for k in range(n):
        capfd.readouterr()
        sd = abi.BamSlice(fx.path, k, n, ctx)
        err = capfd.readouterr().err
        u_lo, u_hi, r = M.slice_walk(fx.path, k, n, fx.stream)
        seen.append("%s: slice %d of %d: %s chunk(s) walked again; the model: %s" % (name, k, n, _walked_again(err), r and (r["what"], r["again"])))
        assert u_lo < u_hi
        assert sd.end in starts or sd.end == fx.total
        at = int(np.searchsorted(offsets, u_lo, side="left"))
        first_true = int(offsets[at]) if at < offsets.size else fx.total
        assert sd.first == first_true or sd.first not in starts
        if k == 0:
            assert sd.first == fx.rec_begin
        if r["what"] == "settled":        # the walk the model makes over the slice's grid: the device's, guess for guess
            assert (sd.first, sd.end) == (r["first"], r["end"])
            assert _walked_again(err) == ([r["again"]] if r["again"] else [])
        if sd.first in starts:
            sh = abi.BamSlice(fx.path, k, n)
            assert (sd.first, sd.end, sd.sorted) == (sh.first, sh.end, sh.sorted)
            for f in ("ref_reads", "ref_bases", "ref_first"):
                np.testing.assert_array_equal(getattr(sd, f), getattr(sh, f), err_msg=f)
            sh.close()
            refid, rr = sd.load_ranges([(sd.first, sd.end)], ctx, resident=True)
            i0, i1 = (int(x) for x in np.searchsorted(kept_offsets, [sd.first, sd.end], side="left"))
            assert i1 > i0 and rr.n_reads == i1 - i0
            np.testing.assert_array_equal(np.array(refid), fx.refid[i0:i1])
            _same_columns(ctx.fetch_payload(rr), synth.take_reads(fx.reads, np.arange(i0, i1)), "slice %d of %d" % (k, n))
            if end_before is not None:
                assert sd.first == end_before
        end_before = sd.end
        sd.close()
    print("\n".join(seen))


# ---- (e) end to end -----------------------------------------------------------------------------------------------------------------

def test_run_midas_snps_as_one_process_and_as_two_ranks(fixtures, tmp_path, monkeypatch):
    """`run_midas.py snps` over `everywhere` as one process and as two ranks that share the one GPU, the blocks inflated and the
    records walked on the device either way: the same files -- whichever way the ranks' slices meet, confirmed boundaries or the
    fall-back to a whole decode."""
    from tests.test_dist_gloo import ROOT, SNPS_WORKER, _run_snps_workers
    fx = fixtures("everywhere")
    script = tmp_path / "snps_worker.py"
    script.write_text(SNPS_WORKER % {"root": ROOT})
    db, one, two = str(tmp_path / "db"), str(tmp_path / "n1"), str(tmp_path / "n2")
    synth.write_sample(one, db, fx.contigs, fx.written)
    shutil.copyfile(fx.path, os.path.join(one, "snps", "temp", "genomes.bam"))
    shutil.copytree(one, two)
    monkeypatch.setenv("SNPS_REAL_DEVICE", "1")
    monkeypatch.setenv("SNPS_DEVICE_INFLATE", "on")
    for d, n in ((one, 1), (two, 2)):
        res = _run_snps_workers(tmp_path, script, d, db, n)
        assert all(rc == 0 for rc, _, _ in res), "\n".join("rank %d: rc %d\n%s" % (k, rc, e[-1500:]) for k, (rc, _, e) in enumerate(res))
    files = sorted(os.listdir(os.path.join(one, "snps", "output")))
    assert len(files) == fx.contigs.n_species and sorted(os.listdir(os.path.join(two, "snps", "output"))) == files
    for f in files:
        got = open(os.path.join(two, "snps", "output", f), "rb").read()
        assert got == open(os.path.join(one, "snps", "output", f), "rb").read() and len(got) > 1000, f
    assert open(os.path.join(two, "snps", "summary.txt")).read() == open(os.path.join(one, "snps", "summary.txt")).read()
