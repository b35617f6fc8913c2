"""The merge site kernel (merge_sites.hip) on the tables of tests/merge_cases.py: every form of it past one pass of its grid
(MIDAS_SNPS_MERGE_GRID_BLOCKS=3) and past one chunk of per-site results (MIDAS_SNPS_MERGE_CHUNK_SITES=700), with the chosen
sites on and around every pass border, compared with the vectorised model at every site, exactly.  Which form ran, and that it
took more than one pass, is read from the library's `[merge kernel]` trace line.  tests/test_merge_cases_host.py holds the model
to the oracle and the cases to their claims."""
import functools
import os
import re

import numpy as np
import pytest

from midas_amd import abi
from tests import merge_cases as MC

pytestmark = pytest.mark.gpu
GRID, CHUNK = 3, 700
ids = lambda table: ['S%d%s' % (S, '_deep' if deep else '') for S, deep in table]
LINE = re.compile(r"\[merge kernel\] form (\w+(?: [SG]=\d+)?), (\d+) samples, (\d+) blocks x (\d+) threads, (\d+) sites")


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=2)
def fill(S, n):
    return MC.random_sites(1000 + S, S, n)


def launches(err):
    """The launches a call made: [(form, samples, blocks, threads, sites)]."""
    return [(m.group(1),) + tuple(int(x) for x in m.groups()[1:]) for m in LINE.finditer(err)]


def merge(ctx, counts, mean, args):
    return ctx.merge_sites(abi.MergeParams.from_args(args), [counts[s] for s in range(counts.shape[0])], mean)


def shape_of(S, mean):
    """-> (form, sites of the table, sites a pass of three blocks covers, threads of a block)"""
    form = MC.form_of(S, mean)
    per = MC.sites_per_block(form)
    return form, (1037 if per == 64 else 2381), GRID * per, (64 * int(form.split('=')[1]) if per == 64 else 256)


def lay(g, n, pass_sites):
    return MC.lay(g.counts, fill(g.counts.shape[0], n), pass_sites)


def chunk_sizes(n):
    return [CHUNK] * (n // CHUNK) + ([n % CHUNK] if n % CHUNK else [])


@pytest.mark.parametrize("S,deep", MC.FORM_TABLE + MC.PREV_TABLE, ids=ids(MC.FORM_TABLE + MC.PREV_TABLE))
def test_every_group_past_one_pass_and_one_chunk(ctx, S, deep, monkeypatch, capfd):
    """Per group of cases one table (merge_cases.lay): runs of its sites at the start, across every pass border and at the end,
    none over another and every site in at least one, seeded sites between; a run wider than a tile crosses tile borders too.
    The sample counts are the issue's per form, and those at which k / S is exactly 0.6 or 0.95.  Three blocks take it in four passes (register and byte forms: 2381 sites,
    768 a pass) or six (split forms: 1037 sites = 17 tiles, so the blocks do 6, 6 and 5 and either set of accumulators is used
    three times; the last tile has 13 live lanes).  Then the same table in chunks of 700 through the default entry."""
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_MERGE_GRID_BLOCKS", str(GRID))
    for g in MC.groups(S, deep):
        form, n, pass_sites, threads = shape_of(S, g.mean)
        counts = lay(g, n, pass_sites)
        capfd.readouterr()
        got = merge(ctx, counts, g.mean, g.args)
        ran = launches(capfd.readouterr().err)
        assert ran == [(form, S, GRID, threads, n)], (g.name, ran)
        assert GRID * MC.sites_per_block(form) < n
        exp = MC.model(counts, g.mean, g.args)
        assert exp['raises'] == -1
        for k in MC.FIELDS:
            assert np.array_equal(got[k], exp[k]), (g.name, k)
        monkeypatch.setenv("MIDAS_SNPS_MERGE_CHUNK_SITES", str(CHUNK))
        chunked = merge(ctx, counts, g.mean, g.args)
        ran = launches(capfd.readouterr().err)
        monkeypatch.delenv("MIDAS_SNPS_MERGE_CHUNK_SITES")
        assert [r[4] for r in ran] == chunk_sizes(n) and all(r[0] == form for r in ran), (g.name, ran)
        for k in MC.FIELDS:
            assert np.array_equal(chunked[k], got[k]), (g.name, k, 'chunked')


def raised(call):
    with pytest.raises(abi.MidasSnpsError) as e:
        call()
    return e.value.status, e.value.message, e.value.read_index


@pytest.mark.parametrize("S,deep", MC.FORM_TABLE, ids=ids(MC.FORM_TABLE))
def test_zero_mean_depth_in_every_form(ctx, S, deep, monkeypatch, capfd, tmp_path):
    """A sample of mean depth 0.0 or -0.0 first, in the middle and last (split forms: in wave 0, a middle wave and the last one
    too).  Raising sites in a later block of the first pass, in a later pass of the first block, in a later chunk and in the
    last ragged block or tile; table j keeps the last 4 - j of them, once as they are and once with the earliest holding 2^28
    (the 64-bit route), and the earliest in file order is reported -- by one launch, by the chunked default entry and by
    merge_sites_tables, which leaves no file."""
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_MERGE_GRID_BLOCKS", str(GRID))
    mean0 = [10.0] * S
    if deep:
        mean0[1] = MC.DEEP
    form, n, pass_sites, threads = shape_of(S, mean0)
    per = MC.sites_per_block(form)
    plant = [per + 44, pass_sites + 8, 2 * CHUNK + 300 if per == 256 else CHUNK + 50, n - 7]
    assert plant == sorted(plant) and plant[0] // per == 1 and plant[1] // pass_sites == 1 and plant[1] % pass_sites < per and plant[2] // CHUNK > plant[1] // CHUNK
    out = tmp_path / "out"
    out.mkdir()
    for j, z in enumerate(MC.zero_positions(S, form)):
        for name, counts, mean, args, first in MC.zero_mean_tables(S, z, -0.0 if j % 2 else 0.0, n, plant, deep):
            assert MC.form_of(S, mean) == form and MC.model(counts, mean, args)['raises'] == first, name
            prm = abi.MergeParams.from_args(args)
            tables = [counts[s] for s in range(S)]
            capfd.readouterr()
            one = raised(lambda: ctx.merge_sites(prm, tables, mean))
            ran = launches(capfd.readouterr().err)
            assert ran == [(form, S, GRID, threads, n)], (name, ran)
            assert one[0] == abi.ERR_MERGE_ZERO_MEAN_DEPTH and one[2] == first and "ZeroDivisionError" in one[1], (name, one)
            assert raised(lambda: ctx.merge_sites_tables(prm, tables, mean, str(out / "f.txt"), str(out / "d.txt"), "h\n")) == one, name
            monkeypatch.setenv("MIDAS_SNPS_MERGE_CHUNK_SITES", str(CHUNK))
            capfd.readouterr()
            chunked = raised(lambda: ctx.merge_sites(prm, tables, mean))
            ran = launches(capfd.readouterr().err)
            in_tables = raised(lambda: ctx.merge_sites_tables(prm, tables, mean, str(out / "f.txt"), str(out / "d.txt"), "h\n"))
            monkeypatch.delenv("MIDAS_SNPS_MERGE_CHUNK_SITES")
            assert chunked == one and in_tables == one, (name, chunked, in_tables)
            assert [r[4] for r in ran] == chunk_sizes(n)[:first // CHUNK + 1], (name, ran)      # it stops at the chunk that raised
            assert os.listdir(str(out)) == [], name


@pytest.mark.parametrize("S", [65, 72, 128])
def test_the_byte_form_and_the_split_form_agree(ctx, S, monkeypatch, capfd):
    """The same counts with every mean 64.0 (a byte per count) and with one mean the next double above (the split form).  At
    site_ratio 2 both means keep depths 1..128, so the two launches answer the same question."""
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_MERGE_GRID_BLOCKS", str(GRID))
    args = dict(MC.DEFAULTS, snp_type=['bi', 'tri'], site_prev=0.5)
    assert MC.limits(64.0, args['site_ratio'], args['site_depth']) == MC.limits(MC.DEEP, args['site_ratio'], args['site_depth']) == (1, 128)
    g = MC.order_group(S)
    counts = lay(g, 2381, GRID * 256)
    counts[:, 700:1400:3, 0] += np.arange(120, 136, dtype=np.uint32).repeat(S // 16 + 1)[:S, None]      # depths on both sides of 128
    got = {}
    for deep in (False, True):
        mean = [64.0] * S
        if deep:
            mean[S // 2] = MC.DEEP
        capfd.readouterr()
        got[deep] = merge(ctx, counts, mean, args)
        ran = launches(capfd.readouterr().err)
        assert [r[0] for r in ran] == [MC.form_of(S, mean)] and ran[0][2] * MC.sites_per_block(ran[0][0]) < 2381, ran
        exp = MC.model(counts, mean, args)
        for k in MC.FIELDS:
            assert np.array_equal(got[deep][k], exp[k]), (deep, k)
    assert len(set(got[False]['count_samples'].tolist())) > 3
    for k in MC.FIELDS:
        assert np.array_equal(got[False][k], got[True][k]), k


@pytest.mark.parametrize("S", range(65, 72))
def test_padded_rows_read_sample_0_site_0_and_drop_it(ctx, S, monkeypatch, capfd):
    """65..71 samples run the 72-sample instantiation: its rows past the last sample are loaded from sample 0's first site and
    masked away.  Whatever lies there -- a count that fits a byte, one that does not, the largest there is -- every other site
    answers as before, and site 0 as the model says.  Then the same in chunks, whose padded rows read the chunk's first site."""
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    monkeypatch.setenv("MIDAS_SNPS_MERGE_GRID_BLOCKS", str(GRID))
    g = MC.freq_groups(S)[2]
    counts = lay(g, 2381, GRID * 256)
    base = merge(ctx, counts, g.mean, g.args)
    for v in (255, 256, MC.TOP):
        c = counts.copy()
        c[0, 0] = v
        capfd.readouterr()
        got = merge(ctx, c, g.mean, g.args)
        assert launches(capfd.readouterr().err) == [('bytes S=72', S, GRID, 256, 2381)]
        exp = MC.model(c, g.mean, g.args)
        for k in MC.FIELDS:
            assert np.array_equal(got[k], exp[k]), (v, k)
            a, b = (got[k], base[k]) if k not in ('depth', 'minor_count') else (got[k].T, base[k].T)
            assert np.array_equal(a[1:], b[1:]), (v, k)
        # in chunks of 700 the padded rows read sample 0's first site OF THE CHUNK: the value at sites 700, 1400 and 2100 too
        first = list(range(0, 2381, CHUNK))
        c[0, first] = v
        monkeypatch.setenv("MIDAS_SNPS_MERGE_CHUNK_SITES", str(CHUNK))
        got = merge(ctx, c, g.mean, g.args)
        monkeypatch.delenv("MIDAS_SNPS_MERGE_CHUNK_SITES")
        assert [r[4] for r in launches(capfd.readouterr().err)] == chunk_sizes(2381)
        exp = MC.model(c, g.mean, g.args)
        others = np.setdiff1d(np.arange(2381), first)
        for k in MC.FIELDS:
            assert np.array_equal(got[k], exp[k]), (v, k, 'chunked')
            a, b = (got[k], base[k]) if k not in ('depth', 'minor_count') else (got[k].T, base[k].T)
            assert np.array_equal(a[others], b[others]), (v, k, 'chunked')


def test_the_grid_as_shipped_takes_a_second_pass(ctx, monkeypatch, capfd):
    """No knob: 3 samples x (1 048 576 + 300) sites, 4096 blocks of 256, so the first 300 threads take a second site.  The order
    and allele_freq 0.01 cases at the start, across site 1 048 575 / 1 048 576 and at the end; every site against the model."""
    monkeypatch.delenv("MIDAS_SNPS_MERGE_GRID_BLOCKS", raising=False)
    monkeypatch.delenv("MIDAS_SNPS_MERGE_CHUNK_SITES", raising=False)
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    S, n = 3, (1 << 20) + 300
    counts = np.random.default_rng(3).integers(0, 9, (S, n, 4), dtype=np.uint32)
    chosen = np.concatenate([MC.order_group(S).counts, MC.freq_groups(S)[0].counts], axis=1).astype(np.uint32)
    k = chosen.shape[1]
    assert k > 300
    counts[:, :k] = chosen
    counts[:, (1 << 20) - k // 2:(1 << 20) - k // 2 + k] = np.roll(chosen, 97, axis=1)
    counts[:, n - 200:] = chosen[:, :200]
    args = dict(MC.DEFAULTS, snp_type=['bi', 'quad'], site_prev=0.5)
    mean = [4.0, 4.0, 4.0]
    capfd.readouterr()
    got = merge(ctx, counts, mean, args)
    assert launches(capfd.readouterr().err) == [('regs32', S, 4096, 256, n)]
    exp = MC.model(counts, mean, args)
    for f in MC.FIELDS:
        assert np.array_equal(got[f], exp[f]), f
    assert set(exp['snp_type'].tolist()) == {0, 1, 2, 3, 4} and set(exp['flag'].tolist()) == {0, 1, 2}
