"""snp_pairs.py without a GPU: the sequential model of the pair call (tests/pairs_model.py) against the existing oracle of the
pooled scan (tests/analyze_model.py, itself pinned to the reference's vectors), then the command with the model injected through
run_pipeline's make_context against one snp_diversity.py run per pair (Contract A, byte for byte), the identity that ties the
shared block to the pooled one, the formatting, the refusals and the tree."""
import contextlib
import io
import itertools
import os
import re

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, diversity, pairs, synth, trees
from tests import analyze_model as AM
from tests import pairs_model as M
from tests import snp_trees_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')
N_SITES, N_SAMPLES, THIN = 400, 7, 5          # sample THIN keeps its depth in one row of 20 only: 20 sites at the most
POOLED_COLUMNS = ['samples'] + diversity.BLOCK_COLUMNS


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def thin_column(indir, k, every):
    """Every depth of matrix column k becomes 0, but in one row of `every`."""
    path = os.path.join(indir, 'snps_depth.txt')
    with open(path) as f:
        lines = f.read().split('\n')
    for r in range(1, len(lines)):
        if lines[r] and r % every:
            cells = lines[r].split('\t')
            cells[1 + k] = '0'
            lines[r] = '\t'.join(cells)
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def write_species(path):
    ids = synth.write_species_dir(path, N_SITES, N_SAMPLES, seed=31, n_genes=9)['sample_ids']
    thin_column(path, THIN, 20)
    with open(os.path.join(path, 'sites.list'), 'w') as f:
        f.write(''.join('%d\n' % k for k in range(3, N_SITES, 3)))
    return ids


def write_rows_dir(path, ids, frows, drows, mean=10.0):
    """A species directory of hand-written cells: IGR sites with reference allele A."""
    os.makedirs(path, exist_ok=True)
    n = len(frows)
    with open(os.path.join(path, 'snps_summary.txt'), 'w') as f:
        f.write('\t'.join(['sample_id', 'genome_length', 'covered_bases', 'fraction_covered', 'mean_coverage']) + '\n')
        f.write(''.join('%s\t%d\t%d\t0.9\t%r\n' % (i, n, n, float(mean)) for i in ids))
    for name, rows in (('freq', frows), ('depth', drows)):
        with open(os.path.join(path, 'snps_%s.txt' % name), 'w') as f:
            f.write('\t'.join(['site_id'] + list(ids)) + '\n')
            f.write(''.join('%d\t%s\n' % (r + 1, '\t'.join(row)) for r, row in enumerate(rows)))
    with open(os.path.join(path, 'snps_info.txt'), 'w') as f:
        f.write('\t'.join(['site_id', 'ref_id', 'ref_pos', 'ref_allele', 'major_allele', 'minor_allele', 'count_samples', 'count_a', 'count_c',
                           'count_g', 'count_t', 'locus_type', 'gene_id', 'snp_type', 'site_type', 'amino_acids']) + '\n')
        f.write(''.join('%d\tcontig_1\t%d\tA\tA\tC\t%d\t0\t0\t0\t0\tIGR\t\tbi\t\t\n' % (r + 1, r + 1, len(ids)) for r in range(n)))
    return path


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pairs") / "species_1")
    return d, write_species(d)


def run_pairs(argv, make_context=M.ModelContext):
    """The command as scripts/snp_pairs.py runs it -> (the table's text, the tree's text or None, the result)."""
    args = cli.pairs_arguments(argv)
    cli.check_pairs_args(args)
    with contextlib.redirect_stdout(io.StringIO()):
        res = pairs.run_pipeline(args, make_context=make_context)
    return open(args['out']).read(), open(args['tree']).read() if args['tree'] else None, res


def table(text):
    rows = [ln.split('\t') for ln in text.split('\n') if ln != '']
    return rows[0], rows[1:]


def project(text):
    """Contract A: per row, the table without sample1, sample2 and the columns from shared_sites on -> {(sample1, sample2): file}."""
    header, rows = table(text)
    assert header == pairs.HEADER
    pick = [header.index(c) for c in POOLED_COLUMNS]
    return {(r[0], r[1]): ''.join('\t'.join(x) + '\n' for x in ([header[k] for k in pick], [r[k] for k in pick])) for r in rows}


def separate_run(indir, a, b, opts, out, make_context=AM.ModelContext):
    """snp_diversity.py --sample_type pooled-samples with exactly the samples a and b selected (no id is part of another)."""
    argv = [indir, '--out', out, '--sample_type', 'pooled-samples', '--genomic_type', 'genome-wide', '--keep_samples', '%s,%s' % (a, b)] + opts
    args = cli.diversity_arguments(argv)
    cli.check_diversity_args(args)
    with contextlib.redirect_stdout(io.StringIO()):
        diversity.run_pipeline(args, make_context=make_context)
    return open(out).read()


def expected_table(argv):
    """What `snp_pairs.py argv` writes, by the model alone -> (table, tree or None)."""
    text, tree, _ = run_pairs(argv)
    return text, tree


# ---- 1. the model's pooled block against the oracle of the pooled scan -----------------------------------------------------------
SCAN_MODES = [dict(), dict(flags=abi.SITES_WEIGHT, site_prev=0.6), dict(site_prev=0.5), dict(flags=abi.SITES_ROUND, site_maf=0.1),
              dict(max_sites=25), dict(flags=abi.SITES_WEIGHT | abi.SITES_ROUND, site_prev=1.0, allele_support=0.7, site_ratio=2.0)]


@pytest.mark.parametrize("mode", SCAN_MODES)
def test_the_models_pooled_block_is_the_pooled_scan_of_the_two_columns(species, mode):
    d, _ = species
    t = abi.SitesTables(d)
    cols = [0, 2, 3, 5, 6]
    mean = t.mean_coverage[cols]
    mask = (np.random.default_rng(3).random(N_SITES) < 0.9).astype(np.uint8)
    kw = dict(site_depth=2, site_ratio=INF, allele_support=0.5, site_prev=0.0, site_maf=0.0, snp_maf=0.01, max_sites=-1, flags=0)
    kw.update(mode)
    got = M.sites_pair_diversity(t.freq_text, t.depth_text, mask, cols, mean, **kw)
    for i, j in itertools.combinations(range(len(cols)), 2):
        exp = AM.sites_scan(t.freq_text, t.depth_text, mask, [cols[i], cols[j]], [mean[i], mean[j]],
                            **dict(kw, flags=kw['flags'] | abi.SITES_SUMS | abi.SITES_POOLED))
        assert got['sites'][i, j] == exp['sites'][0, 0] and got['snps'][i, j] == exp['snps'][0, 0], (i, j)
        assert bits(got['pi'][i, j]) == bits(exp['pi'][0, 0]), (i, j)
    assert got['sites'][np.triu_indices(len(cols), 1)].min() > 0


# ---- 2. the command against the separate runs ----------------------------------------------------------------------------------------
OPTION_SETS = [
    [],
    ['--weight_by_depth', '--site_prev', '0.6'],
    ['--site_prev', '0.5'],
    ['--consensus', '--site_maf', '0.1'],
    ['--max_sites', '25'],
    ['--max_sites', '25', '--site_prev', '1.0'],
    ['--rand_sites', '0.7', '--seed', '5'],
    ['--site_list', 'sites.list'],
    ['--locus_type', 'CDS', '--site_type', '4D'],
]


def resolve(d, opts):
    return [os.path.join(d, o) if o == 'sites.list' else o for o in opts]


@pytest.mark.parametrize("opts", OPTION_SETS)
def test_every_row_is_a_snp_diversity_run_of_the_pair(species, tmp_path, opts):
    d, ids = species
    opts = resolve(d, opts)
    text, _, res = run_pairs([d, '--out', str(tmp_path / 'pairs.txt')] + opts)
    got = project(text)
    assert list(got) == list(itertools.combinations(ids, 2))
    for a, b in got:
        assert got[(a, b)] == separate_run(d, a, b, opts, str(tmp_path / 'pi.txt')), (a, b, opts)
    assert res['sites'].sum() > 0


def test_max_sites_is_every_pairs_own(species):
    """--max_sites 25 with --site_prev 1.0 (without a site filter every pair retains the same rows): pairs fill it at different rows,
    and the pairs of the thinned sample never fill it."""
    d, _ = species
    t = abi.SitesTables(d)
    rows = {}
    res = M.sites_pair_diversity(t.freq_text, t.depth_text, np.ones(N_SITES, np.uint8), list(range(N_SAMPLES)), t.mean_coverage, 2, INF, 0.5,
                                 1.0, 0.0, max_sites=25, _rows_out=rows)
    filled = {p: r[-1] for p, r in rows.items() if len(r) == 25}
    assert len(set(filled.values())) >= 2
    never = [p for p, r in rows.items() if len(r) < 25]
    assert never and all(THIN in p for p in never)
    assert all(res['sites'][p] == len(r) for p, r in rows.items())


# ---- 3. the identity between the two blocks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.SITES_ROUND])
def test_pooled_pi_is_the_mean_of_within_and_between(species, flags):
    """With --site_prev 1.0 and unweighted pooling every retained site is shared and p = (a + b) / 2, so in real arithmetic
    2 p (1 - p) = (2 a (1 - a) + 2 b (1 - b)) / 4 + (a (1 - b) + b (1 - a)) / 2.  A site adds a handful of roundings of terms no
    larger than 1 to either side."""
    d, _ = species
    t = abi.SitesTables(d)
    res = M.sites_pair_diversity(t.freq_text, t.depth_text, np.ones(N_SITES, np.uint8), list(range(N_SAMPLES)), t.mean_coverage, 2, INF, 0.5,
                                 1.0, 0.0, flags=flags)
    for i, j in itertools.combinations(range(N_SAMPLES), 2):
        sites = int(res['sites'][i, j])
        assert res['shared'][i, j] == sites
        assert abs(res['pi'][i, j] - ((res['w1'][i, j] + res['w2'][i, j]) / 4 + res['x'][i, j] / 2)) <= 16 * sites * 2.0 ** -53, (i, j)
    assert res['sites'].max() > 100


# ---- 4. formatting, refusals and the tree ------------------------------------------------------------------------------------------------
def test_rows_order_na_cells_and_the_shared_block(species, tmp_path):
    d, ids = species
    text, _, res = run_pairs([d, '--out', str(tmp_path / 'pairs.txt'), '--site_prev', '0.5'])
    header, rows = table(text)
    assert header == ['sample1', 'sample2', 'samples', 'sites', 'snps', 'pi', 'snps_kb', 'pi_bp', 'shared_sites', 'pi_bp_1', 'pi_bp_2', 'dxy', 'fst', 'da']
    assert [(r[0], r[1]) for r in rows] == list(itertools.combinations(ids, 2)) and all(r[2] == '2' for r in rows)
    for r, (i, j) in zip(rows, itertools.combinations(range(len(ids)), 2)):
        shared = int(res['shared'][i, j])
        assert r[8] == str(shared) and shared > 0
        p1, p2, dxy = float(res['w1'][i, j]) / shared, float(res['w2'][i, j]) / shared, float(res['x'][i, j]) / shared
        w = (p1 + p2) / 2.0
        assert r[9:12] == [repr(p1), repr(p2), repr(dxy)]
        assert r[12] == (repr(1.0 - w / dxy) if dxy != 0.0 else 'NA') and r[13] == repr(dxy - w)
    # no cell of any sample reaches --site_depth 61: every site is retained, none is shared
    text, _, res = run_pairs([d, '--out', str(tmp_path / 'pairs.txt'), '--site_depth', '61'])
    _, rows = table(text)
    assert all(r[3] == str(N_SITES) and r[8] == '0' and r[9:] == ['NA'] * 5 for r in rows) and res['shared'].sum() == 0


def test_fst_is_na_where_dxy_is_zero(tmp_path):
    frows = [['0', '0', '0.25'], ['0', '0', '0.5'], ['0', '0', '0.1']]
    d = write_rows_dir(str(tmp_path / 'sp'), ['a', 'b', 'c'], frows, [['5', '6', '7']] * 3)
    text, _, _ = run_pairs([d, '--out', str(tmp_path / 'pairs.txt')])
    _, rows = table(text)
    assert rows[0][:2] == ['a', 'b'] and rows[0][8:] == ['3', '0.0', '0.0', '0.0', 'NA', '0.0']
    assert rows[1][:2] == ['a', 'c'] and 'NA' not in rows[1] and float(rows[1][12]) == 1.0 - ((0.0 + float(rows[1][10])) / 2.0) / float(rows[1][11])


def _exits(argv, needle):
    with pytest.raises(SystemExit) as e:
        run_pairs(argv)
    assert needle in str(e.value), e.value


def test_refusals(species, tmp_path):
    d, ids = species
    out = ['--out', str(tmp_path / 'pairs.txt')]
    _exits([d] + out + ['--keep_samples', ids[1]], "a pair needs 2 samples; 1 selected")
    _exits([d] + out + ['--tree', str(tmp_path / 't.nwk'), '--keep_samples', '%s,%s' % (ids[0], ids[1])], "a tree needs at least 3 samples")
    _exits([d] + out + ['--site_depth', '1'], "--site_depth must be >=2")
    _exits([d] + out + ['--site_type', '4D'], "--locus_type must be CDS")
    _exits([d] + out + ['--tree', str(tmp_path / 't.nwk'), '--site_depth', '61'], "have no site at which both of them are kept")
    odd = write_rows_dir(str(tmp_path / 'odd'), ['a', 'b(1)', 'c'], [['0.1', '0.2', '0.3']] * 4, [['5', '5', '5']] * 4)
    _exits([odd] + out + ['--tree', str(tmp_path / 't.nwk')], "which a Newick label cannot hold")
    assert run_pairs([odd] + out)[0].count('\n') == 4          # (without a tree the id is a cell like any other)
    for option in (['--rand_reads', '5'], ['--replace_reads'], ['--genomic_type', 'per-gene'], ['--sample_type', 'per-sample']):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            cli.pairs_arguments([d] + out + option)
    with pytest.raises(SystemExit), contextlib.redirect_stdout(io.StringIO()) as buf:
        cli.pairs_arguments(['--help'])
    helped = buf.getvalue()
    assert '--rand_reads / --replace_reads are not offered' in helped and '--genomic_type / --sample_type are not offered' in helped


def test_a_bad_row_ends_the_command_with_file_and_line(tmp_path):
    f = [['0.1', '0.2', '0.3'] for _ in range(6)]
    f[4][1] = 'nan'
    d = write_rows_dir(str(tmp_path / 'sp'), ['a', 'b', 'c'], f, [['5', '5', '5']] * 6)
    out = ['--out', str(tmp_path / 'pairs.txt')]
    assert run_pairs([d] + out)[0].count('\n') == 4                                 # (without --consensus nan is a number)
    _exits([d] + out + ['--consensus', '--max_sites', '2'], "snps_freq.txt, line 6: sample b: the frequency is not a finite number")
    f[2][2] = '0.3x'
    d = write_rows_dir(str(tmp_path / 'sp2'), ['a', 'b', 'c'], f, [['5', '5', '5']] * 6)
    _exits([d] + out + ['--consensus'], "snps_freq.txt, line 4: sample c: the cell is not a number")


def test_the_tree_is_neighbour_joining_over_da(species, tmp_path):
    d, ids = species
    text, newick, res = run_pairs([d, '--out', str(tmp_path / 'pairs.txt'), '--tree', str(tmp_path / 'da.nwk'), '--site_prev', '0.5'])
    n = len(ids)
    da = np.zeros((n, n))
    _, rows = table(text)
    for r, (i, j) in zip(rows, itertools.combinations(range(n), 2)):
        da[i, j] = da[j, i] = float(r[13])
    assert np.array_equal(bits(da), bits(res['da'])) and np.array_equal(da, da.T) and not da.diagonal().any()
    assert newick == trees.newick(ids, TM.nj_tree(da)) == TM.newick(ids, TM.nj_tree(da))
    assert sorted(re.findall(r'sample_\d+', newick)) == sorted(ids)


def test_the_symbol_is_declared_bound_and_built_without_contraction():
    from midas_amd import build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    assert re.search(r"\bmidas_sites_pair_diversity\s*\(", src) and 'midas_sites_pair_diversity' in abi.SITES_SYMBOLS
    assert getattr(abi.load_library(), 'midas_sites_pair_diversity').argtypes is not None
    assert 'sites_pairs.hip' in build.SOURCES and '-ffp-contract=off' in build.SOURCE_FLAGS['sites_pairs.hip']
    assert os.path.exists(os.path.join(ROOT, 'scripts', 'snp_pairs.py'))
