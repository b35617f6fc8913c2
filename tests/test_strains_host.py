"""strain_tracking.py without a GPU: both commands with the sequential model of the device calls (tests/strains_model.py)
against the reference's own output (tests/golden/strain_vectors.json) -- output bytes, printed lines, parsed arguments --, what
the golden file must cover, every error exit, the usage screen, the native writers and the symbol list."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli, sites, strains
from tests import analyze_model as A
from tests import strains_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
SCRIPT = os.path.join(ROOT, 'scripts', 'strain_tracking.py')


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("strains")), VEC)


def argv_of(tree, program, case, out):
    return M.argv_of(tree, program, case, out, VEC['markers'])


def run(tree, program, case, out, make_context=M.ModelContext, extra=()):
    return M.run(tree, program, case, out, make_context, extra, VEC['markers'])


def check_case(tree, program, case, out, make_context=M.ModelContext, extra=()):
    M.check_case(tree, program, case, out, make_context, extra, VEC['markers'])


@pytest.mark.parametrize("k", range(len(VEC['id_markers'])))
def test_id_markers_with_the_model_writes_the_references_bytes(tree, tmp_path, k):
    check_case(tree, 'id_markers', VEC['id_markers'][k], str(tmp_path / 'markers.txt'))


@pytest.mark.parametrize("k", range(len(VEC['track_markers'])))
def test_track_markers_with_the_model_writes_the_references_bytes(tree, tmp_path, k):
    check_case(tree, 'track_markers', VEC['track_markers'][k], str(tmp_path / 'sharing.txt'))


def test_the_output_does_not_depend_on_group_rows_or_max_samples(tree, tmp_path):
    check_case(tree, 'id_markers', VEC['id_markers'][0], str(tmp_path / 'm.txt'), extra=['--group_rows', '33'])
    case = VEC['track_markers'][2]
    check_case(tree, 'track_markers', dict(case, args={}), str(tmp_path / 's.txt'), extra=['--group_rows', '33', '--max_samples', '2'])
    assert len(M.expected_out(case).splitlines()) == 1 + 14 * 13 // 2


def test_the_golden_covers_what_it_must():
    ids, tracks = VEC['id_markers'], VEC['track_markers']
    default = [c for c in ids if c['species'] == 'strains' and not c['options']][0]
    assert len(default['out'].splitlines()) - 1 >= 50
    shared = [int(r.split('\t')[4]) for c in tracks for r in M.expected_out(c).splitlines()[1:]]
    assert any(x > 0 for x in shared) and any(x == 0 for x in shared)
    sp = VEC['species']['strains']
    info = [r.split('\t') for r in sp['info'].splitlines()[1:]]
    assert any(r[4] == r[5] for r in info)
    freq = [r.split('\t')[1:] for r in sp['freq'].splitlines()[1:]]
    depth = [r.split('\t')[1:] for r in sp['depth'].splitlines()[1:]]
    cells = {(f, d) for fr, dr in zip(freq, depth) for f, d in zip(fr, dr)}
    assert ('0.5', '5') in cells and ('0.5', '7') in cells and round(0.5 * 5) == 2 and round(0.5 * 7) == 4
    assert any(d == '0' for _, d in cells)
    assert any(f == '0.1' for f, _ in cells) and any(f == '0.9' for f, _ in cells) and 0.1 >= 0.1 and not (1 - 0.9) >= 0.1
    # 0.1 passes as the minor allele and 0.9 fails as the major one: both sites are markers of their one sample
    rows = {r.split('\t')[0]: r.split('\t') for r in default['out'].splitlines()[1:]}
    for f in ('0.1', '0.9'):
        i = [k for k, fr in enumerate(freq) if f in fr][0]
        assert rows[info[i][0]][1] == info[i][5] and rows[info[i][0]][2] == '14'
    assert any(not A.is_fast_float(f) for f, _ in cells) and any(not A.is_fast_int(d) for _, d in cells)
    opts = [' '.join(c['options']) for c in ids]
    assert any('--samples' in o for o in opts) and any('--max_sites' in o for o in opts) and any('--allele_prev' in o for o in opts)
    assert any('--max_sites' in ' '.join(c['options']) for c in tracks) and any('--max_samples' in ' '.join(c['options']) for c in tracks)
    assert max(len(v['summary'].splitlines()) - 1 for v in VEC['species'].values()) > 128
    listed = [r.split('\t') for r in VEC['markers']['m_odd'].splitlines()[1:]]
    order = {r[0]: k for k, r in enumerate(info)}
    assert any(len(r) != 7 for r in listed)
    assert any(r[0] not in order for r in listed)
    assert any(r[0] in order and r[1] not in (info[order[r[0]]][4], info[order[r[0]]][5]) for r in listed if len(r) == 7)
    at = [order[r[0]] for r in VEC['markers']['m_out_of_order'].splitlines()[1:] for r in [r.split('\t')]]
    assert at != sorted(at)
    assert os.path.getsize(M.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(M.GOLDEN), 'merge_vectors.json'))


def test_every_sites_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(midas_sites_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(abi.SITES_SYMBOLS)
    for sym in ('midas_sites_id_markers', 'midas_sites_track_markers', 'midas_sites_write_markers', 'midas_sites_write_pairs'):
        assert sym in declared and getattr(abi.load_library(), sym).argtypes is not None
    assert abi.SITES_PAIR_TILE == int(re.search(r"#define MIDAS_SITES_PAIR_TILE (\d+)", src).group(1))
    assert abi.load_library().midas_snps_abi_version() == 4


def test_usage_screen_and_unrecognized_command():
    for argv in ([], ['-h'], ['--help']):
        r = subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == VEC['usage'] and r.stderr == ''
    r = subprocess.run([sys.executable, SCRIPT, 'markers'], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr == "\nError: Unrecognized command: 'markers'\n\n" and r.stdout == ''
    for program in cli.STRAIN_COMMANDS:
        r = subprocess.run([sys.executable, SCRIPT, program, '-h'], capture_output=True, text=True)
        assert r.returncode == 0 and 'Usage: strain_tracking.py %s [options]' % program in r.stdout
        for opt in ('--indir', '--out', '--min_freq', '--min_reads', '--max_sites', '--group_rows'):
            assert opt in r.stdout


def test_track_arguments_exits(tree, tmp_path):
    base = ['track_markers', '--indir', '%s/strains' % tree]
    for argv, message in ((['track_markers', '--indir', str(tmp_path / 'nowhere'), '--markers', '%s/m_default.txt' % tree, '--out', 'o'],
                           "Specified input directory '%s' does not exist" % (tmp_path / 'nowhere')),
                          (base + ['--markers', str(tmp_path / 'none.txt'), '--out', 'o'],
                           "Specified input file '%s' does not exist" % (tmp_path / 'none.txt')),
                          (base + ['--out', 'o'], "--markers is required"),
                          (base + ['--markers', '%s/m_default.txt' % tree], "--out is required")):
        with pytest.raises(SystemExit) as e:
            cli.track_markers_arguments(argv)
        assert e.value.code == "\nError: %s\n" % message
    # the script stops there, before the device is touched
    r = subprocess.run([sys.executable, SCRIPT] + base + ['--markers', str(tmp_path / 'none.txt'), '--out', 'o'], capture_output=True, text=True)
    assert r.returncode == 1 and "does not exist" in r.stderr
    with pytest.raises(SystemExit) as e:
        run(tree, 'track_markers', dict(species='strains', options=['--markers', 'm_header_only']), str(tmp_path / 'o'))
    assert e.value.code == "\nError: no marker alleles found in file: %s/m_header_only.txt\n" % tree
    with pytest.raises(SystemExit) as e:
        run(tree, 'id_markers', dict(species='strains', options=['--samples', 'nobody,s00']), str(tmp_path / 'o'))
    assert "no samples satisfied your selection criteria" in e.value.code
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'id_markers', dict(species='absent', options=[]), str(tmp_path / 'o'))
    assert 'snps_summary.txt' in e.value.code


def _edited(tmp_path, edits, summary=None):
    """The species 'strains' with cells replaced: edits = [(table, data row, field, text)]."""
    sp = dict(VEC['species']['strains'])
    for table, row, field, text in edits:
        rows = sp[table].split('\n')
        f = rows[1 + row].split('\t')
        f[field] = text
        rows[1 + row] = '\t'.join(f) if field >= 0 else text
        sp[table] = '\n'.join(rows)
    d = str(tmp_path / 'strains')
    M.write_species(d, sp)
    return d


def test_samples_is_list_membership_and_mean_coverage_zero_is_accepted(tmp_path):
    d = _edited(tmp_path, [('summary', 1, 4, '0')])
    t = sites.open_tables(d)
    assert list(sites.fetch_samples(t, keep_samples=['s001', 's01', 's0'], zero_depth_ok=True)) == ['s001']
    assert list(sites.fetch_samples(t, keep_samples=['s0021', 's003'])) == ['s003']
    assert list(sites.fetch_samples(t, keep_samples='s0021,s003')) == ['s002', 's003']  # the other commands' substring test is as it was ...
    with pytest.raises(SystemExit) as e:                                                # ... and they still refuse a mean_coverage of 0
        sites.fetch_samples(t, keep_samples='s001')
    assert "sample s001 has mean_coverage 0" in e.value.code
    _, printed = run(str(tmp_path), 'id_markers', dict(species='strains', options=['--samples', 's001,s002,s003']), str(tmp_path / 'o'))
    assert printed.endswith("total disriminative alleles found\n")


def test_sites_that_cannot_be_called_exit_with_file_line_and_letter(tmp_path):
    info = [r.split('\t') for r in VEC['species']['strains']['info'].splitlines()[1:]]
    freq = [r.split('\t')[1:] for r in VEC['species']['strains']['freq'].splitlines()[1:]]
    i = [k for k, fr in enumerate(freq) if fr.count('1') == 1 and set(fr) == {'0', '1'} and k > 20][0]
    s = freq[i].index('1')
    depth = VEC['species']['strains']['depth'].splitlines()[1 + i].split('\t')[1:]
    assert int(depth[s]) >= 3
    first_with_depth = [k for k, x in enumerate(depth) if A.abi_parse(x, 1) != 0][0]
    # a minor allele that is no letter, where a sample has it: the reference's KeyError
    d = _edited(tmp_path, [('info', i, 5, 'NA')])
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'id_markers', dict(species='strains', options=[]), str(tmp_path / 'o'))
    assert e.value.code == "\nError: %s/snps_info.txt, line %d: sample s%03d has the minor_allele 'NA', which is none of A, T, C, G\n" % (d, i + 2, s)
    # ... a run that ends before the site never sees it, and neither does one whose samples lack the allele
    run(str(tmp_path), 'id_markers', dict(species='strains', options=['--max_sites', str(i)]), str(tmp_path / 'o'))
    run(str(tmp_path), 'id_markers', dict(species='strains', options=['--samples', 's%03d' % ((s + 1) % 14)]), str(tmp_path / 'o'))
    d = _edited(tmp_path, [('info', i, 4, 'n')])
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'id_markers', dict(species='strains', options=[]), str(tmp_path / 'o'))
    assert e.value.code == "\nError: %s/snps_info.txt, line %d: sample s%03d has the major_allele 'n', which is none of A, T, C, G\n" \
        % (d, i + 2, first_with_depth)
    # round(inf): id_markers only where the frequency passes, track_markers at every cell of a matched site
    d = _edited(tmp_path, [('freq', i, 1 + s, 'inf')])
    for program, opts in (('id_markers', []), ('track_markers', ['--markers', 'm'])):
        with open(str(tmp_path / 'm.txt'), 'w') as f:
            f.write('site_id\tallele\n%s\t%s\n' % (info[i][0], info[i][5]))
        with pytest.raises(SystemExit) as e:
            run(str(tmp_path), program, dict(species='strains', options=[str(tmp_path / 'm.txt') if o == 'm' else o for o in opts]), str(tmp_path / 'o'))
        assert e.value.code == "\nError: %s/snps_freq.txt, line %d: sample s%03d: frequency x depth is not a finite number\n" % (d, i + 2, s)
    d = _edited(tmp_path, [('freq', i, 1 + s, 'nan')])
    run(str(tmp_path), 'id_markers', dict(species='strains', options=[]), str(tmp_path / 'o'))       # nan >= min_freq is False: no round()
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'track_markers', dict(species='strains', options=['--markers', str(tmp_path / 'm.txt')]), str(tmp_path / 'o'))
    assert "snps_freq.txt, line %d: sample s%03d: frequency x depth is not a finite number" % (i + 2, s) in e.value.code


@pytest.mark.parametrize("which, cell, what", [('freq', '0.5x', 'not a number'), ('depth', '3.0', 'not an integer')])
def test_malformed_cells_and_short_rows_exit_with_file_and_line(tmp_path, which, cell, what):
    d = _edited(tmp_path, [(which, 30, 4, cell)])
    with open(str(tmp_path / 'm.txt'), 'w') as f:
        f.write(VEC['markers']['m_default'])
    for program, opts in (('id_markers', []), ('track_markers', ['--markers', str(tmp_path / 'm.txt')])):
        with pytest.raises(SystemExit) as e:
            run(str(tmp_path), program, dict(species='strains', options=opts), str(tmp_path / 'o'))
        assert e.value.code == "\nError: %s/snps_%s.txt, line 32: sample s003: the cell is %s\n" % (d, which, what)
        # --max_sites counts rows read: the row behind the last one in use is still read, the one after it is not
        with pytest.raises(SystemExit):
            run(str(tmp_path), program, dict(species='strains', options=opts + ['--max_sites', '30']), str(tmp_path / 'o'))
        run(str(tmp_path), program, dict(species='strains', options=opts + ['--max_sites', '29']), str(tmp_path / 'o'))
    row = VEC['species']['strains'][which].split('\n')[31]
    d = _edited(tmp_path, [(which, 30, -1, '\t'.join(row.split('\t')[:6]))])
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'id_markers', dict(species='strains', options=[]), str(tmp_path / 'o'))
    assert e.value.code == "\nError: %s/snps_%s.txt, line 32: the row has fewer sample columns than the samples in use\n" % (d, which)
    run(str(tmp_path), 'id_markers', dict(species='strains', options=['--samples', 's000,s004']), str(tmp_path / 'o'))


def test_the_error_in_the_earlier_row_is_the_one_reported(tmp_path):
    """The reference converts a row and calls it before it reads the next: a letter that is no key in row 25 comes before a
    malformed cell in row 40, and a malformed cell in row 25 before a letter in row 40 -- at any group size."""
    freq = [r.split('\t')[1:] for r in VEC['species']['strains']['freq'].splitlines()[1:]]
    rows = [k for k, fr in enumerate(freq) if fr.count('1') == 1 and set(fr) == {'0', '1'} and k > 20][:2]
    first, second = rows
    for group_rows in ('0', '7', '1000'):
        d = _edited(tmp_path, [('info', first, 5, 'NA'), ('depth', second, 3, 'x')])
        with pytest.raises(SystemExit) as e:
            run(str(tmp_path), 'id_markers', dict(species='strains', options=['--group_rows', group_rows]), str(tmp_path / 'o'))
        assert "%s/snps_info.txt, line %d: " % (d, first + 2) in e.value.code and "minor_allele 'NA'" in e.value.code
        d = _edited(tmp_path, [('info', second, 5, 'NA'), ('depth', first, 3, 'x')])
        with pytest.raises(SystemExit) as e:
            run(str(tmp_path), 'id_markers', dict(species='strains', options=['--group_rows', group_rows]), str(tmp_path / 'o'))
        assert e.value.code == "\nError: %s/snps_depth.txt, line %d: sample s002: the cell is not an integer\n" % (d, first + 2)


def test_a_site_id_matched_twice_is_rejected(tmp_path):
    sp = VEC['species']['strains']
    info = sp['info'].split('\n')
    first = info[1].split('\t')
    second = info[2].split('\t')
    second[0] = first[0]
    d = _edited(tmp_path, [('info', 1, -1, '\t'.join(second))])
    with open(str(tmp_path / 'm.txt'), 'w') as f:
        f.write('site_id\tallele\n%s\t%s\n%s\t%s\nc1|9|A\tA\n' % (first[0], first[4], first[0], first[4]))
    with pytest.raises(SystemExit) as e:
        run(str(tmp_path), 'track_markers', dict(species='strains', options=['--markers', str(tmp_path / 'm.txt')]), str(tmp_path / 'o'))
    assert e.value.code == "\nError: %s/snps_info.txt, line 3: the site %s is listed twice\n" % (d, first[0])


def test_native_writers(tree, tmp_path):
    t = sites.open_tables('%s/strains' % tree)
    ids, samples = t.strings('site_id'), t.strings('sample_id')
    rows = np.array([[5, 0, 14, 1, 13, 0, 0], [219, 3, 2147483647, 0, 0, 7, 1]], np.int32)
    t.write_markers(str(tmp_path / 'm.txt'), rows)
    assert open(str(tmp_path / 'm.txt')).read() == 'site_id\tallele\tcount_samples\tcount_A\tcount_T\tcount_C\tcount_G\n' \
        '%s\tA\t14\t1\t13\t0\t0\n%s\tG\t2147483647\t0\t0\t7\t1\n' % (ids[5], ids[219])
    t.write_markers(str(tmp_path / 'm.txt'), np.zeros((0, 7), np.int32))
    assert open(str(tmp_path / 'm.txt')).read().count('\n') == 1
    with pytest.raises(abi.MidasSnpsError):
        t.write_markers(str(tmp_path / 'm.txt'), np.array([[220, 0, 1, 1, 1, 1, 1]], np.int32))
    both = np.array([[3, 1, 0], [0, 1 << 40, 2], [0, 0, 2]], np.int64)
    t.write_pairs(str(tmp_path / 'p.txt'), [0, 2, 13], both)
    assert open(str(tmp_path / 'p.txt')).read() == 'sample1\tsample2\tcount1\tcount2\tcount_both\tcount_either\n' \
        '%s\t%s\t3\t%d\t1\t%d\n%s\t%s\t3\t2\t0\t5\n%s\t%s\t%d\t2\t2\t%d\n' \
        % (samples[0], samples[2], 1 << 40, (1 << 40) + 2, samples[0], samples[13], samples[2], samples[13], 1 << 40, 1 << 40)
    with pytest.raises(abi.MidasSnpsError) as e:
        t.write_pairs(str(tmp_path / 'nowhere' / 'p.txt'), [0, 1, 2], both)
    assert 'cannot be written' in e.value.message
    with pytest.raises(abi.MidasSnpsError) as e:
        t.write_pairs(str(tmp_path / 'p.txt'), [0, 1, 14], both)
    assert 'does not exist' in e.value.message
