"""snp_diversity.py --rand_reads / --replace_reads / --seed without a GPU: the sequential model (tests/resample_model.py) against
the reference's own output and final generator state (tests/golden/resample_vectors.json) through the command's own layers, the
raw-stream restatement of the draws against np.random.choice itself, the command line, and the host arithmetic of the draw budget
(midas_amd/csrc/draw_plan.h, tests/cpp/draw_plan_check.cpp)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.analyze import cli
from tests import resample_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = VEC['cases']


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return M.write_tree(str(tmp_path_factory.mktemp("resample")), VEC)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_the_model_writes_the_references_bytes_and_leaves_its_state(tree, tmp_path, k):
    M.check_case(tree, CASES[k], str(tmp_path / 'pi.txt'))


def test_the_golden_covers_what_it_must():
    opts = [' '.join(c['options']) for c in CASES]
    for n in (1, 2, 3, 5, 8, 9, 33):
        assert any('--rand_reads %d --replace_reads' % n in o for o in opts), n
    assert any('--rand_reads' in o and '--replace_reads' not in o for o in opts)
    for need in ('per-gene', 'pooled-samples', '--weight_by_depth', '--consensus', '--max_sites', '--rand_sites', '--rand_samples'):
        assert any(need in o for o in opts), need
    assert any('per-gene' in o and 'pooled' in o for o in opts) and any('per-gene' in o and 'pooled' not in o for o in opts)
    n = {k: len(v['summary'].splitlines()) - 1 for k, v in VEC['species'].items()}
    assert sorted(n.values()) == [13, 150]
    for c in CASES:
        if '--replace_reads' in c['options']:
            N = int(c['options'][1])
            if N == 1 or '--consensus' in c['options']:
                assert c['raw_words'] == 0
            elif N >= 3:
                assert c['raw_words'] > 2 * 624
    a = VEC['species']['a13']
    rows = [r.split('\t')[1:] for r in a['freq'].splitlines()[1:]]
    assert all(c == '0' for c in rows[4]) and any('0.5' in r for r in rows)
    assert int(round(0.5 * 5)) == 2 and int(round(0.5 * 3)) == 2 and int(round(0.5 * 9)) == 4     # exact halves go to even
    # a sample that is not kept (depth below the raised --site_depth) with 0 < freq < 1 at a resampled site
    depths = [r.split('\t')[1:] for r in a['depth'].splitlines()[1:]]
    assert any(0 < float(f) < 1 and int(d) < 5 for fr, dr in zip(rows, depths) for f, d in zip(fr, dr))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 16, 17, 33, 100])
def test_the_raw_stream_is_np_random_choice(n):
    """The accepted words of the raw stream, N a cell, are the draws of the reference's own lines, cell after cell -- and the
    state behind the last accepted word is the state numpy is left in."""
    np.random.seed(5)
    start = np.random.get_state()
    rng = np.random.default_rng(n)
    freqs = [float('%.3g' % x) for x in rng.random(300)]
    exp = []
    for f in freqs:
        count_minor = int(round(f * n))
        alleles = np.random.choice([1] * count_minor + [0] * (n - count_minor), n, replace=True)
        exp.append(float(np.mean(alleles)))
    end = np.random.get_state()
    stream = M.RawStream(start)
    got = [M.resample_cell(f, n, True, stream) / n for f in freqs]
    assert got == exp
    st = stream.state() if stream.consumed else start
    assert int(st[2]) == int(end[2]) and np.array_equal(st[1], end[1])
    assert (stream.consumed == 0) == (n == 1)
    if n & (n - 1) == 0:
        assert stream.consumed == (300 * n if n > 1 else 0)         # a power of two accepts every word
    # without replacement all N reads are picked: the mean is count_minor / N whatever the permutation
    for f in freqs[:40]:
        count_minor = int(round(f * n))
        alleles = np.random.choice([1] * count_minor + [0] * (n - count_minor), n, replace=False)
        assert float(np.mean(alleles)) == M.resample_cell(f, n, False, None) / n


def test_masks():
    assert [M.draw_mask(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 2 ** 31 - 1)] == [0, 1, 3, 3, 7, 7, 15, 15, 31, 63, 2 ** 31 - 1]


def test_rand_reads_is_an_option_now(tree, tmp_path):
    args = cli.diversity_arguments(['%s/a13' % tree, '--rand_reads', '5'])
    cli.check_diversity_args(args, resampling=True)                  # (no exit)
    assert args['site_depth'] == 5 and args['rand_reads'] == 5 and args['replace_reads'] is False and args['seed'] is None
    assert cli.diversity_arguments(['%s/a13' % tree, '--rand_reads', '3', '--site_depth', '7'])['site_depth'] == 7
    args = cli.diversity_arguments(['%s/a13' % tree, '--rand_reads', '0', '--replace_reads'])        # 0 is "off", as in the reference
    cli.check_diversity_args(args, resampling=True)
    assert args['site_depth'] == 2
    for bad in ('-1', str(2 ** 31)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_diversity.py'), '%s/a13' % tree, '--rand_reads', bad],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and '--rand_reads' in r.stderr
    # the command itself gets past its checks with the option (and ends at the device, where there is none)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_diversity.py'), '%s/a13' % tree, '--rand_reads', '5', '--out',
                        str(tmp_path / 'o')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert 'not part of this build' not in r.stderr and '  rand_reads: 5\n' in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'snp_diversity.py'), '-h'], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and '--seed' in r.stdout and 'not part of this build' not in r.stdout
    # the printed block is the reference's: --seed is not in it, --site_depth is the raised one
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.print_args(cli.diversity_arguments(['%s/a13' % tree, '--rand_reads', '5', '--seed', '3']), 'snp_diversity.py')
    assert '  rand_reads: 5\n  replace_reads: False\n' in buf.getvalue() and '  site_depth: 5\n' in buf.getvalue() and 'seed' not in buf.getvalue()


def test_seed_makes_runs_equal_and_is_the_two_seed_calls(tree, tmp_path):
    case = [c for c in CASES if c['options'][:3] == ['--rand_reads', '9', '--replace_reads'] and '--rand_samples' in c['options']][0]
    outs = []
    for k in range(2):
        np.random.seed(1000 + k)                                     # whatever the streams held before
        random.seed(2000 + k)
        out = str(tmp_path / ('pi%d.txt' % k))
        args = cli.diversity_arguments(['%s/%s' % (tree, case['species'])] + case['options'] + ['--seed', str(case['seed']), '--out', out])
        cli.check_diversity_args(args, resampling=True)
        import contextlib
        import io
        from midas_amd.analyze import diversity
        with contextlib.redirect_stdout(io.StringIO()):
            diversity.run_pipeline(args, make_context=M.ModelContext)
        outs.append(open(out).read())
    assert outs[0] == outs[1] == case['out']
    # without --seed the streams are taken as they stand
    out = str(tmp_path / 'other.txt')
    M.run_case(tree, dict(case, seed=case['seed'] + 1), out)
    assert open(out).read() != case['out']


def test_the_new_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    lib = abi.load_library()
    for sym, names in (('midas_sites_scan_resampled', abi.SITES_SYMBOLS), ('midas_snps_mt19937_stream', abi.EXPORTED_SYMBOLS)):
        assert sym + '(' in header and sym in names and getattr(lib, sym).argtypes is not None
    from midas_amd import build
    assert 'mt19937_stream.hip' in build.SOURCES and 'sites_resample.h' in build.HEADERS and 'draw_plan.h' in build.HEADERS
    src = open(os.path.join(ROOT, 'midas_amd', 'csrc', 'sites_scan.hip')).read()
    assert src.count('rg.next(&g)') == 1                             # one group loop for both entry points


def test_draw_plan_properties(tmp_path):
    exe = str(tmp_path / "draw_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "midas_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "draw_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
