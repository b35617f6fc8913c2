"""`merge_midas.py genes` on the GPU box: midas_genes_merge against a numpy model with sequential fp64 sums (bit for bit),
column groups of any size giving the same bytes, samples with differing row orders, the CLI against the reference's text
(tests/golden/merge_genes_vectors.json), the run_midas.py genes -> merge_midas.py genes chain, and 2 / 3 ranks."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, synth
from tests import genes_merge_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _samples(rng, S, n, C, heavy=0, shared=True):
    base = np.sort(rng.integers(0, C, n)).astype(np.uint32)
    if heavy:
        base[rng.choice(n, heavy, replace=False)] = 3
    rng.shuffle(base)
    cl = [base if shared or s % 2 == 0 else rng.permutation(base) for s in range(S)]
    scale = 10.0 ** rng.integers(-6, 17, (S, n))
    cp = [rng.standard_normal(n) * scale[s] for s in range(S)]
    dp = [rng.random(n) * 10.0 ** rng.integers(-3, 17, n) for s in range(S)]
    rd = [rng.integers(0, 1 << 40, n) for s in range(S)]
    return cl, cp, dp, rd


def _same(a, b):
    for k in ('rows', 'reads', 'state'):
        assert np.array_equal(a[k], b[k]), k
    for k in ('copy', 'depth'):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64)), k


@pytest.mark.parametrize("S", [1, 3, 64, 65, 300])
def test_kernel_matches_sequential_model(ctx, S):
    rng = np.random.default_rng(S)
    n, C = (20000, 3000) if S < 300 else (4000, 900)
    cl, cp, dp, rd = _samples(rng, S, n, C, heavy=12000 if S < 300 else 1500)
    cp[0][cl[0] == 5] = 0.35                      # min_copy hit exactly
    res = ctx.genes_merge(cl, cp, dp, rd, C, 0.35)
    _same(res, M.model_merge(cl, cp, dp, rd, C, 0.35))
    assert (np.diff(res['rows'].astype(np.int64)) > 0).all()


def test_a_cluster_of_more_than_ten_thousand_rows(ctx):
    rng = np.random.default_rng(11)
    n, C, S = 30000, 50, 5
    cl = [np.where(rng.random(n) < 0.6, 7, rng.integers(0, C, n)).astype(np.uint32)] * S
    cp = [rng.random(n) * 10.0 ** rng.integers(-8, 17, n) * rng.choice([-1, 1], n) for _ in range(S)]
    dp = [rng.random(n) for _ in range(S)]
    rd = [rng.integers(0, 1000, n) for _ in range(S)]
    assert (cl[0] == 7).sum() > 10000
    _same(ctx.genes_merge(cl, cp, dp, rd, C, 0.35), M.model_merge(cl, cp, dp, rd, C, 0.35))


def test_column_groups_do_not_change_the_bytes(ctx):
    rng = np.random.default_rng(5)
    S, n, C = 40, 5000, 1200
    cl, cp, dp, rd = _samples(rng, S, n, C, heavy=800)
    runs = [ctx.genes_merge(cl, cp, dp, rd, C, 0.35, group_samples=g) for g in (1, 7, S, 0)]
    for r in runs[1:]:
        _same(runs[0], r)
    _same(runs[0], M.model_merge(cl, cp, dp, rd, C, 0.35))


def test_differing_row_orders_and_row_sets(ctx):
    rng = np.random.default_rng(9)
    S, n, C = 9, 6000, 2000
    cl, cp, dp, rd = _samples(rng, S, n, C, heavy=500, shared=False)
    # one sample with a row set of its own (fewer rows, clusters sample 0 lacks), one sharing sample 0's array
    cl[4] = rng.integers(0, C, 3000).astype(np.uint32)
    cp[4], dp[4], rd[4] = cp[4][:3000], dp[4][:3000], rd[4][:3000]
    cl[6] = cl[0]
    for g in (0, 2, 5):
        _same(ctx.genes_merge(cl, cp, dp, rd, C, 0.35, group_samples=g), M.model_merge(cl, cp, dp, rd, C, 0.35))


def test_bad_cluster_index_is_a_status(ctx):
    cl = [np.array([0, 1, 9], np.uint32)]
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.genes_merge(cl, [np.ones(3)], [np.ones(3)], [np.ones(3, np.int64)], 5, 0.35)
    assert e.value.status == abi.ERR_BAD_LAYOUT


def _cli(args, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'genes'] + args, capture_output=True,
                          text=True, cwd=ROOT, env=env, timeout=600)


@pytest.mark.parametrize("pid", ['75', '80', '85', '90', '95', '99'])
def test_cli_matches_the_reference_text(tmp_path, pid):
    db, dirs = M.write_golden_dataset(str(tmp_path / 'in'), VEC)
    out = str(tmp_path / 'out')
    r = _cli([out, '-i', ','.join(dirs), '-t', 'list', '-d', db, '--cluster_pid', pid, '--threads', '4'])
    assert r.returncode == 0, r.stderr
    M.check_outputs(out, VEC, pid)


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_ranks_sharing_one_gpu_write_the_single_process_files(tmp_path, n_ranks):
    db, dirs = M.write_golden_dataset(str(tmp_path / 'in'), VEC)
    out = str(tmp_path / 'out')
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'genes', out, '-i', ','.join(dirs), '-t', 'list', '-d', db]
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=dict(base, RANK=str(k), LOCAL_RANK="0", WORLD_SIZE=str(n_ranks), LOCAL_WORLD_SIZE=str(n_ranks),
                                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29650 + n_ranks)))
             for k in range(n_ranks)]
    for k, p in enumerate(procs):
        o, e = p.communicate(timeout=600)
        assert p.returncode == 0, (k, o, e[-3000:])
    M.check_outputs(out, VEC, '95')


def _write_gene_info(db, ds):
    for sp in ds['species_ids']:
        genes = [g for g, s in zip(ds['gene_ids'], ds['gene_species']) if s == sp]
        with open(os.path.join(db, 'pan_genomes', sp, 'gene_info.txt'), 'w') as h:
            h.write('gene_id\tgenome_id\tcentroid_99\tcentroid_95\tcentroid_90\tcentroid_85\tcentroid_80\tcentroid_75\n')
            for k, g in enumerate(genes):
                h.write('%s\t%s.rep\t%s\t%s\t%s\t%s\t%s\t%s\n' % (g, sp, g, genes[k - k % 2], genes[k - k % 3], genes[k - k % 4],
                                                                genes[k - k % 5], genes[0]))


def test_run_midas_then_merge_midas_genes_chain(tmp_path):
    ds = synth.make_pangenome_dataset(n_species=2, genes_per_species=60, n_reads=12000, seed=31)
    db = str(tmp_path / 'db')
    fq = str(tmp_path / 'reads.fq')
    with open(fq, 'w') as h:
        h.write("@r1\nACGT\n+\nIIII\n")
    rng = np.random.default_rng(3)
    dirs = []
    for k in range(3):
        idx = np.sort(rng.choice(ds['refid'].size, ds['refid'].size * (k + 2) // 5, replace=False))
        part = dict(ds, reads=synth.take_reads(ds['reads'], idx), refid=ds['refid'][idx])
        d = str(tmp_path / ('sample_%d' % k))
        synth.write_pangenome_sample(d, db, part)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_midas.py'), 'genes', d, '--call_genes', '-d', db,
                            '-1', fq], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        dirs.append(d)
    _write_gene_info(db, ds)
    out = str(tmp_path / 'out')
    r = _cli([out, '-i', ','.join(dirs), '-t', 'list', '-d', db, '--sample_depth', '0', '--min_copy', '0.5'])
    assert r.returncode == 0, r.stderr
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import merge_midas
    finally:
        sys.path.pop(0)
    from midas_amd.merge import genes
    cpu = str(tmp_path / 'cpu')
    args = dict(program='genes', outdir=cpu, input=','.join(dirs), intype='list', db=db, min_samples=1, species_id=None,
                max_species=None, sample_depth=0.0, max_samples=None, cluster_pid='95', min_copy=0.5, threads=2)
    merge_midas.check_arguments(args)
    genes.run_pipeline(args, make_context=M.NumpyGenesContext)
    for sp in ds['species_ids']:
        for name in M.MATRICES + ('summary',):
            a = open(os.path.join(out, sp, 'genes_%s.txt' % name)).read()
            assert a == open(os.path.join(cpu, sp, 'genes_%s.txt' % name)).read(), (sp, name)
            assert len(a.splitlines()) > 1
