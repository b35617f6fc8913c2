"""snp_ld.py without a GPU: the sequential model (tests/snp_ld_model.py) against a case computed by hand, its calls against
snp_trees_model's planes, the command through the model (ld.run_pipeline's make_context), NA bins, the order check, every
argument error, and the positions reader of the tables."""
import contextlib
import io
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, ld, sites, synth
from tests import analyze_model
from tests import snp_ld_model as M
from tests import snp_trees_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_HEADER = ['site_id', 'ref_id', 'ref_pos', 'ref_allele', 'major_allele', 'minor_allele', 'count_samples', 'count_a', 'count_c', 'count_g',
               'count_t', 'locus_type', 'gene_id', 'snp_type', 'site_type', 'amino_acids']


def _run(indir, options, out, make_context=M.ModelContext):
    args = cli.ld_arguments([indir] + list(options) + ['--out', out])
    cli.check_ld_args(args)
    with contextlib.redirect_stdout(io.StringIO()):
        return ld.run_pipeline(args, make_context=make_context)


def _copy(src, dst):
    shutil.copytree(src, dst)
    return dst


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    """600 sites x 7 samples; positions in three contigs, genes in runs with sites outside any gene between them."""
    d = str(tmp_path_factory.mktemp("ld") / "species_1")
    synth.write_species_dir(d, n_sites=600, n_samples=7, seed=5)
    ref_id, ref_pos = M.spread_positions(600, np.arange(600), 60, seed=1)
    locus, gene = M.gene_runs(600)
    M.rewrite_info(d, dict(ref_id=ref_id, ref_pos=ref_pos, locus_type=locus, gene_id=gene))
    return d


def _write_dir(d, positions, minor, depth=None):
    """A species directory by hand: minor [site][sample] 0 / 1 is the frequency, depth 10 everywhere unless given."""
    os.makedirs(d)
    n_samples = len(minor[0])
    ids = ['s%d' % k for k in range(n_samples)]
    with open(os.path.join(d, 'snps_summary.txt'), 'w') as f:
        f.write('sample_id\tgenome_length\tcovered_bases\tfraction_covered\tmean_coverage\n')
        f.write(''.join('%s\t100\t100\t1.0\t10.0\n' % i for i in ids))
    with open(os.path.join(d, 'snps_info.txt'), 'w') as f:
        f.write('\t'.join(INFO_HEADER) + '\n')
        f.write(''.join('%d\t%s\t%d\tA\tA\tC\t%d\t0\t0\t0\t0\tIGR\t\tbi\t\t\n' % (k + 1, c, p, n_samples) for k, (c, p) in enumerate(positions)))
    for name, rows in (('snps_freq.txt', [['%.1f' % x for x in r] for r in minor]),
                       ('snps_depth.txt', depth or [['10'] * n_samples for _ in minor])):
        with open(os.path.join(d, name), 'w') as f:
            f.write('\t'.join(['site_id'] + ids) + '\n')
            f.write(''.join('\t'.join([str(k + 1)] + [str(c) for c in r]) + '\n' for k, r in enumerate(rows)))
    return d


def test_four_sites_by_six_samples_computed_by_hand(tmp_path):
    """Every sample is called at every site.  The minor alleles:  site 1 (position 1) s0 s1 s2; site 2 (position 2) s0 s1; site 3
    (position 4) s0 s2 s4; site 4 (position 12) none.  --max_dist 12 --bin_width 5: the bins 1-5, 6-10 and 11-12.
      (1, 2) distance 1: n 6, na 3, nb 2, nab 2 -> Dn = 12 - 6 = 6, ha = 9, hb = 8: r2 = 36 / 72, d2 = 36 / 1296, het = 72 / 1296
      (1, 3) distance 3: n 6, na 3, nb 3, nab 2 -> Dn = 12 - 9 = 3, ha = 9, hb = 9: r2 = 9 / 81, d2 = 9 / 1296, het = 81 / 1296
      (2, 3) distance 2: n 6, na 2, nb 3, nab 1 -> Dn = 6 - 6 = 0, ha = 8, hb = 9: r2 = 0, d2 = 0, het = 72 / 1296
      (2, 4) distance 10, (3, 4) distance 8, (1, 4) distance 11: site 4 has one allele, so none of them is informative."""
    d = _write_dir(str(tmp_path / 'species_1'), [('c1', 1), ('c1', 2), ('c1', 4), ('c1', 12)],
                   [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0]])
    out = str(tmp_path / 'ld.txt')
    res = _run(d, ['--max_dist', '12', '--bin_width', '5'], out)
    anchor_1 = [(0.0 + 36.0 / 72.0) + 9.0 / 81.0, (0.0 + 36.0 / 1296.0) + 9.0 / 1296.0, (0.0 + 72.0 / 1296.0) + 81.0 / 1296.0]
    anchor_2 = [0.0 + 0.0 / 72.0, 0.0 + 0.0 / 1296.0, 0.0 + 72.0 / 1296.0]
    sum_r2, sum_d2, sum_het = ((0.0 + a) + b for a, b in zip(anchor_1, anchor_2))
    assert res['window'].tolist() == [3, 2, 1] and res['pairs'].tolist() == [3, 0, 0]
    assert [res['sum_r2'][0], res['sum_d2'][0], res['sum_het'][0]] == [sum_r2, sum_d2, sum_het]
    assert abs(sum_r2 / 3.0 - (0.5 + 1 / 9) / 3) < 1e-15 and abs(sum_d2 / sum_het - 0.2) < 1e-15
    assert open(out).read() == ('bin_start\tbin_end\tsite_pairs\tld_pairs\tr2\tsigma2_d\n'
                                '1\t5\t3\t3\t%r\t%r\n'
                                '6\t10\t2\t0\tNA\tNA\n'
                                '11\t12\t1\t0\tNA\tNA\n' % (sum_r2 / 3.0, sum_d2 / sum_het))
    # --min_samples 7: no pair has seven samples called at both sites; every bin is NA, the pairs of sites stay
    _run(d, ['--max_dist', '12', '--bin_width', '5', '--min_samples', '7'], out)
    assert [ln.split('\t')[2:] for ln in open(out).read().splitlines()[1:]] == [['3', '0', 'NA', 'NA'], ['2', '0', 'NA', 'NA'], ['1', '0', 'NA', 'NA']]
    # a second contig takes no pair across: its sites pair among themselves alone
    d2 = _write_dir(str(tmp_path / 'two' / 'species_1'), [('c1', 1), ('c1', 2), ('c2', 1), ('c2', 3)],
                    [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0], [0, 1, 1, 0, 1, 0]])
    res = _run(d2, ['--max_dist', '12', '--bin_width', '5'], out)
    assert res['window'].tolist() == [2, 0, 0] and res['pairs'].tolist() == [2, 0, 0]
    # a sample without a read at a site is not called there: n drops to 5 at the pairs with site 2
    depth = [['10'] * 6, ['10', '10', '10', '0', '10', '10'], ['10'] * 6, ['10'] * 6]
    d3 = _write_dir(str(tmp_path / 'three' / 'species_1'), [('c1', 1), ('c1', 2), ('c1', 4), ('c1', 12)],
                    [[1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0], [0, 0, 0, 0, 0, 0]], depth)
    res = _run(d3, ['--max_dist', '5', '--bin_width', '5', '--min_samples', '6'], out)
    assert res['window'].tolist() == [3] and res['pairs'].tolist() == [1] and res['sum_r2'][0] == 9.0 / 81.0
    res = _run(d3, ['--max_dist', '5', '--bin_width', '5', '--min_samples', '5'], out)
    # (1, 2): n 5, na 3, nb 2, nab 2 -> Dn = 10 - 6 = 4, ha = 6, hb = 6;  (2, 3): n 5, na 2, nb 3, nab 1 -> Dn = 5 - 6 = -1
    assert res['pairs'].tolist() == [3] and res['sum_r2'][0] == ((0.0 + 16.0 / 36.0) + 9.0 / 81.0) + (0.0 + 1.0 / 36.0)


@pytest.mark.parametrize("kw", [dict(), dict(site_maf=0.05, site_prev=0.5), dict(max_sites=150), dict(flags=abi.SITES_MASK_ONLY)])
def test_the_models_calls_are_the_planes_of_snp_trees_model(species, kw):
    t = abi.SitesTables(species)
    cols, mask = [0, 2, 3, 5, 6], sites.info_mask(t)
    mask[::7] = False
    opts = dict(dict(site_depth=3, site_ratio=3.0, allele_support=0.6, site_prev=0.8, site_maf=0.0), **kw)
    mine = M.consensus_calls(t.freq_text, t.depth_text, mask, cols, t.mean_coverage[cols], **opts)
    n = mask.shape[0]
    flags = (opts.pop('flags', 0) & abi.SITES_MASK_ONLY) | abi.SITES_SEQ
    ref = analyze_model.sites_scan(t.freq_text, t.depth_text, mask, cols, t.mean_coverage[cols], flags=flags,
                                   minor=np.full(n, snp_trees_model.MINOR, np.uint8), major=np.full(n, snp_trees_model.MAJOR, np.uint8),
                                   dump_keep=True, **opts)
    assert np.array_equal(mine['rows'], np.flatnonzero(ref['keep'])) and 100 < mine['n_kept'] < n
    assert np.array_equal(mine['called'], ref['seq'] != ord('-')) and np.array_equal(mine['minor'], ref['seq'] == snp_trees_model.MINOR)
    assert (mine['n_sites'], mine['n_kept'], mine['side_freq'], mine['side_depth']) == tuple(ref[k] for k in ('n_sites', 'n_kept', 'side_freq', 'side_depth'))
    assert mine['minor'].any() and not mine['called'].all()
    pairs = snp_trees_model.sites_consensus_pairs(t.freq_text, t.depth_text, mask, cols, t.mean_coverage[cols], **dict(opts, flags=flags))
    for i in range(len(cols)):
        for j in range(i, len(cols)):
            shared = mine['called'][i] & mine['called'][j]
            assert (int(shared.sum()), int((shared & (mine['minor'][i] ^ mine['minor'][j])).sum())) == (pairs['both'][i, j], pairs['diff'][i, j])


@pytest.mark.parametrize("options", [['--max_dist', '60', '--bin_width', '7'], ['--max_dist', '45', '--bin_width', '9', '--within', 'gene', '--min_samples', '5'],
                                     ['--max_dist', '60', '--bin_width', '20', '--site_prev', '0.9', '--site_depth', '4', '--exclude_samples', 'sample_003'],
                                     ['--max_dist', '30', '--bin_width', '1', '--max_sites', '200', '--locus_type', 'CDS']])
def test_the_command_through_the_model(species, tmp_path, options):
    out = str(tmp_path / 'ld.txt')
    res = _run(species, options, out)
    text, exp = M.expected_file([species] + options)
    assert open(out).read() == text and M.means_something(exp)
    lines = text.splitlines()
    args = cli.ld_arguments([species] + options)
    assert len(lines) == 1 + -(-args['max_dist'] // args['bin_width']) and lines[-1].split('\t')[1] == str(args['max_dist'])
    assert np.array_equal(res['window'], exp['window']) and res['n_kept'] == exp['n_kept']
    if '--within' in options:
        everywhere = M.expected_file([species] + [o for o in options if o not in ('--within', 'gene')])[1]
        assert 0 < exp['window'].sum() < everywhere['window'].sum()
    if '--max_sites' in options:
        assert exp['n_kept'] == 200 and exp['n_sites'] < 600


def test_keys_follow_first_appearance_and_must_ascend_over_the_mask(species, tmp_path):
    t = abi.SitesTables(species)
    key = ld.site_keys(t, np.ones(t.n_sites, bool))
    assert np.array_equal(key, M.info_keys(species)) and t.contig_names == ['contig_a', 'contig_b', 'contig_c']
    assert sorted(set((key >> 40).tolist())) == [0, 1, 2] and int((key >> 40 == 1).sum()) == 1
    out = str(tmp_path / 'ld.txt')
    ref_id, ref_pos = M.read_info_columns(species, ['ref_id', 'ref_pos'])
    info = lambda d: os.path.join(d, 'snps_info.txt')
    # a position that repeats the one before it; one that steps back; a contig that comes back
    for k, (row, col, value, line_before) in enumerate(((100, 'ref_pos', ref_pos[99], 101), (50, 'ref_pos', '3', 51), (450, 'ref_id', 'contig_a', 451))):
        d = _copy(species, str(tmp_path / ('order_%d' % k) / 'species_1'))
        column = list(ref_id if col == 'ref_id' else ref_pos)
        column[row] = value
        M.rewrite_info(d, {col: column})
        with pytest.raises(SystemExit) as e:
            _run(d, [], out)
        assert e.value.code.startswith("\nError: %s, line %d: the site does not lie behind the one before it (line %d)" % (info(d), row + 2, line_before))
        # ... unless the row is none of the mask's: a --site_list without it
        listed = str(tmp_path / ('sites_%d.txt' % k))
        with open(listed, 'w') as f:
            f.write(''.join('%d\n' % (r + 1) for r in range(600) if r != row and (col == 'ref_pos' or r < 440)))
        _run(d, ['--site_list', listed], out)
    d = _copy(species, str(tmp_path / 'far' / 'species_1'))
    M.rewrite_info(d, dict(ref_pos=ref_pos[:-1] + [str(1 << 40)]))
    with pytest.raises(SystemExit) as e:
        _run(d, [], out)
    assert e.value.code == "\nError: %s, line 601: ref_pos must be between 0 and 2^40 - 1\n" % info(d)


def test_the_positions_reader(species, tmp_path):
    t = abi.SitesTables(species)
    ref_id, ref_pos = M.read_info_columns(species, ['ref_id', 'ref_pos'])
    assert t.ref_pos.dtype == np.int64 and t.ref_pos.tolist() == [int(p) for p in ref_pos] and t.contig.dtype == np.int32
    assert [t.contig_names[k] for k in t.contig.tolist()] == ref_id
    assert t.n_sites == 600 and len(t.strings('site_id')) == 600 and t.gene.shape == (600,)          # the rest is as it was
    with open(os.path.join(species, 'snps_info.txt')) as f:
        text = f.read()

    def variant(name, new_text):
        d = _copy(species, str(tmp_path / name / 'species_1'))
        with open(os.path.join(d, 'snps_info.txt'), 'w') as f:
            f.write(new_text)
        return d, abi.SitesTables(d)                                   # opens as ever: only the positions are at fault

    header, body = text.split('\n', 1)
    for name, column in (('no_pos', 'ref_pos'), ('no_id', 'ref_id')):
        d, tv = variant(name, header.replace(column, 'other') + '\n' + body)
        with pytest.raises(abi.MidasSnpsError) as e:
            tv.ref_pos
        assert e.value.message == "%s/snps_info.txt, line 1: the header lacks the column %s" % (d, column)
        assert tv.n_sites == 600
        with pytest.raises(SystemExit) as e:
            _run(d, [], str(tmp_path / 'ld.txt'))
        assert e.value.code == "\nError: %s/snps_info.txt, line 1: the header lacks the column %s\n" % (d, column)
    lines = text.split('\n')
    for name, value in (('bad_pos', '12x'), ('float_pos', '12.0'), ('empty_pos', '')):
        cells = lines[300].split('\t')
        cells[2] = value
        d, tv = variant(name, '\n'.join(lines[:300] + ['\t'.join(cells)] + lines[301:]))
        with pytest.raises(abi.MidasSnpsError) as e:
            tv.contig
        assert e.value.message == "%s/snps_info.txt, line 301: ref_pos is not an integer" % d
    d, tv = variant('moved', '\n'.join('\t'.join(ln.split('\t')[3:] + ln.split('\t')[:3]) if ln else ln for ln in lines))
    assert tv.ref_pos.tolist() == t.ref_pos.tolist() and tv.contig.tolist() == t.contig.tolist()      # found by name, wherever they stand
    moved = open(os.path.join(d, 'snps_info.txt')).read().split('\n')
    d, tv = variant('short', '\n'.join(moved[:200] + [moved[200].rsplit('\t', 1)[0]] + moved[201:]))       # ref_pos stands last there
    with pytest.raises(abi.MidasSnpsError) as e:
        tv.ref_pos
    assert e.value.message == "%s/snps_info.txt, line 201: the row lacks ref_id or ref_pos" % d


def test_every_argument_error(species, tmp_path):
    for options, message in ((['--max_dist', '0'], "--max_dist must be >= 1"), (['--max_dist', str(1 << 39), '--bin_width', str(1 << 30)], "--max_dist must be below 2^39"),
                             (['--bin_width', '0'], "--bin_width must be >= 1"), (['--bin_width', '-3'], "--bin_width must be >= 1"),
                             (['--max_dist', '4097', '--bin_width', '1'], "--max_dist / --bin_width gives more than 4096 distance bins: raise --bin_width"),
                             (['--min_samples', '0'], "--min_samples must be >= 1"), (['--site_depth', '0'], "--site_depth must be >=1"),
                             (['--site_prev', '1.5'], "--site_prev must be between 0 and 1"), (['--max_sites', '0'], "--max_sites must be >= 1 to calculate nucleotide variation"),
                             (['--anchor_chunk', '-1'], "--group_rows, --chunk_bytes and --anchor_chunk cannot be negative")):
        with pytest.raises(SystemExit) as e:
            cli.check_ld_args(cli.ld_arguments([species] + options))
        assert e.value.code == "\nError: %s\n" % message, options
    cli.check_ld_args(cli.ld_arguments([species, '--max_dist', '4096', '--bin_width', '1']))            # 4096 bins are allowed
    cli.check_ld_args(cli.ld_arguments([species, '--max_dist', str((1 << 39) - 1), '--bin_width', str(1 << 27)]))
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(io.StringIO()):
        cli.ld_arguments([species, '--within', 'operon'])
    assert e.value.code == 2
    args = cli.ld_arguments([species])
    assert (args['max_dist'], args['bin_width'], args['min_samples'], args['within'], args['site_depth'], args['out']) == (1000, 10, 4, 'contig', 2, '/dev/stdout')
    script = os.path.join(ROOT, 'scripts', 'snp_ld.py')
    r = subprocess.run([sys.executable, script, str(tmp_path / 'nowhere')], capture_output=True, text=True)
    assert r.returncode != 0 and "does not exist" in r.stderr
    r = subprocess.run([sys.executable, script, species, '--bin_width', '0'], capture_output=True, text=True)
    assert r.returncode != 0 and "--bin_width must be >= 1" in r.stderr
    r = subprocess.run([sys.executable, script, '-h'], capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stdout for o in ('--max_dist', '--bin_width', '--min_samples', '--within', '--exclude_samples'))
    assert '--anchor_chunk' not in r.stdout and '--group_rows' not in r.stdout


def test_the_exits_of_the_device_call(species, tmp_path):
    out = str(tmp_path / 'ld.txt')
    with pytest.raises(SystemExit) as e:
        _run(species, [], out, make_context=lambda: M.ModelContext(site_limit=500))
    assert e.value.code.startswith("\nError: 600 sites pass the site filters that need no frequency, but the calls of at most 500 sites of 7 samples fit")
    _run(species, ['--max_sites', '100'], out, make_context=lambda: M.ModelContext(site_limit=600))
    d = _copy(species, str(tmp_path / 'cell' / 'species_1'))
    with open(os.path.join(d, 'snps_depth.txt')) as f:
        lines = f.read().split('\n')
    cells = lines[41].split('\t')
    cells[3] = '7.5'
    lines[41] = '\t'.join(cells)
    with open(os.path.join(d, 'snps_depth.txt'), 'w') as f:
        f.write('\n'.join(lines))
    with pytest.raises(SystemExit) as e:
        _run(d, [], out)
    assert e.value.code == "\nError: %s, line 42: sample sample_002: the cell is not an integer\n" % os.path.join(d, 'snps_depth.txt')
    _run(d, ['--max_sites', '30'], out)                      # the walk ends before the row


def test_the_new_symbols_are_declared_bound_and_built_without_contraction():
    from midas_amd import build
    lib = abi.load_library()
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    for sym in ('midas_sites_ld', 'midas_sites_tables_positions'):
        assert re.search(r"\b%s\s*\(" % sym, header) and getattr(lib, sym).argtypes is not None and sym in abi.SITES_SYMBOLS
    assert 'sites_ld.hip' in build.SOURCES and build.SOURCE_FLAGS['sites_ld.hip'] == ['-ffp-contract=off']
    assert abi.SITES_LD_SAME_GENE == int(re.search(r"#define MIDAS_SITES_LD_SAME_GENE (\d+)", header).group(1))
    assert abi.SITES_LD_MAX_BINS == cli.LD_MAX_BINS == 4096
    assert abi.SITES_LD_SAME_GENE not in (abi.SITES_WEIGHT, abi.SITES_ROUND, abi.SITES_POOLED, abi.SITES_PER_GENE, abi.SITES_MASK_ONLY, abi.SITES_SEQ, abi.SITES_SUMS)
