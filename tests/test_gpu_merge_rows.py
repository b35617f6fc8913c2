"""snps_freq.txt / snps_depth.txt formatted on the device (merge_rows.hip): midas_merge_write_matrix_device and
midas_merge_sites_tables against text built here from Python's own '{0:.3g}'.format(float(m) / d) and str(d), and against the
host writer (abi.write_merge_matrix) on the same arrays, byte for byte; then `merge_midas.py snps` on the device path."""
import os
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.merge import merge, snps as msnps
from tests.test_gpu_merge import INFO_HEADER, VARIANTS, oracle_text, ctx, dataset  # noqa: F401  (ctx, dataset: fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CAP = '0.004'      # MIDAS_SNPS_MERGE_TEXT_MB: 4 KiB of text a batch


def cells(depth, minor):
    """[S, n] arrays -> [S, n] object array of the cells' text, each distinct (m, d) formatted once by Python."""
    if minor is None:
        u, inv = np.unique(depth, return_inverse=True)
        return np.array([str(int(d)) for d in u], dtype=object)[inv].reshape(depth.shape)
    key = (minor.astype(np.uint64) << np.uint64(32)) | depth.astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    text = []
    for k in u.tolist():
        m, d = k >> 32, k & 0xFFFFFFFF
        text.append('{0:.3g}'.format(float(m) / d if d > 0 else 0.0))
    return np.array(text, dtype=object)[inv].reshape(depth.shape)


def expected(header, keep, depth, minor, base, c=None):
    c = cells(depth, minor) if c is None else c
    return (header + "".join("%d\t%s\n" % (base + i + 1, "\t".join(c[:, i])) for i in np.asarray(keep).tolist())).encode()


def check(ctx, tmp_path, depth, minor, keep, base=0, header="", name="t", c=None):
    """Both writers on the same arrays: the device's file == Python's text == the host writer's file.  (c: cells(depth, minor),
    for a caller that checks the same arrays several times.)"""
    dev, host = str(tmp_path / (name + ".dev")), str(tmp_path / (name + ".host"))
    abi.write_merge_matrix_device(ctx, dev, header, keep, depth, minor, site_id_base=base)
    abi.write_merge_matrix(host, header, keep, depth, minor, threads=2, site_id_base=base)
    got = open(dev, 'rb').read()
    assert got == expected(header, keep, depth, minor, base, c), name
    assert got == open(host, 'rb').read(), name
    assert not [f for f in os.listdir(str(tmp_path)) if '.tmp.' in f]
    return got


def grid(pairs, n_samples):
    """(m, d) pairs laid out as [n_samples, n_sites] minor / depth arrays, padded with (0, 0)."""
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n = -(-pairs.shape[0] // n_samples)
    full = np.zeros((n * n_samples, 2), np.uint32)
    full[:pairs.shape[0]] = pairs
    return np.ascontiguousarray(full[:, 1].reshape(n, n_samples).T), np.ascontiguousarray(full[:, 0].reshape(n, n_samples).T)


def test_every_small_pair(ctx, tmp_path):
    d = np.repeat(np.arange(1201), np.arange(1201) + 1)
    m = np.concatenate([np.arange(k + 1) for k in range(1201)])
    depth, minor = grid(np.stack([m, d], 1), 64)
    assert depth.shape[0] == 64 and 11200 < depth.shape[1] < 11400
    check(ctx, tmp_path, depth, minor, np.arange(depth.shape[1]))


TIE_FAMILIES = [2 * 10 ** k for k in range(3, 10)] + [16 * 10 ** k for k in range(4)] + [32, 64, 80, 16384, 2 ** 20, 2 ** 31]


def test_ties(ctx, tmp_path):
    """Denominators with exact three-digit ties, some representable as doubles (half to even) and some not (the double's side)."""
    pairs = np.concatenate([np.stack([np.arange(1, min(d, 40000) + 1), np.full(min(d, 40000), d)], 1) for d in TIE_FAMILIES])
    for (m, d), want in {(9985, 10000): '0.999', (1999, 2000): '1', (1, 32): '0.0312', (3, 32): '0.0938'}.items():
        assert '{0:.3g}'.format(float(m) / d) == want
    named = [(9985, 10000), (1999, 2000), (1, 32), (3, 32)]
    depth, minor = grid(np.concatenate([np.array(named), pairs]), 16)
    got = check(ctx, tmp_path, depth, minor, np.arange(depth.shape[1]))
    assert got.split(b'\n')[0].split(b'\t')[:5] == [b'1', b'0.999', b'1', b'0.0312', b'0.0938']


def test_exponent_border_and_extremes(ctx, tmp_path):
    pairs = [(99949, 10 ** 9), (99950, 10 ** 9), (99951, 10 ** 9), (1, 10000), (1, 10240), (1, 4294967294), (0, 0), (0, 17), (17, 17),
             (4294967294, 4294967294), (4294967293, 4294967294), (5, 0)]
    depth, minor = grid(pairs, 1)
    got = check(ctx, tmp_path, depth, minor, np.arange(len(pairs))).decode().split('\n')
    vals = [row.split('\t')[1] for row in got[:-1]]
    assert vals[:3] == ['9.99e-05', '0.0001', '0.0001'] and vals[3] == '0.0001' and vals[4] == '9.77e-05' and vals[5] == '2.33e-10'
    assert vals[6:] == ['0', '0', '1', '1', '1', '0']
    check(ctx, tmp_path, depth.reshape(3, 4), minor.reshape(3, 4), np.arange(4), name="three")


def test_depth_table_values(ctx, tmp_path):
    vals = np.array([0, 9, 10, 99999, 2 ** 31, 4294967294, 100000, 4294967295, 1, 999999999, 1000000000, 7], np.uint32)
    got = check(ctx, tmp_path, vals.reshape(1, -1), None, np.arange(vals.size)).decode().split('\n')
    assert [row.split('\t')[1] for row in got[:-1]] == [str(int(v)) for v in vals]
    check(ctx, tmp_path, vals.reshape(4, 3), None, np.arange(3), name="four")


def shape_arrays(S, n, seed):
    """Depths and minor counts of every width: small, around a byte, around 2^16, up to 2^32 - 2."""
    rng = np.random.default_rng(seed)
    top = np.array([1, 12, 300, 70000, 4294967294], np.uint64)[rng.integers(0, 5, (S, n))]
    depth = (rng.integers(0, 2 ** 62, (S, n)).astype(np.uint64) % (top + np.uint64(1))).astype(np.uint32)
    minor = (rng.integers(0, 2 ** 62, (S, n)).astype(np.uint64) % (depth.astype(np.uint64) + np.uint64(1))).astype(np.uint32)
    minor[rng.random((S, n)) < 0.3] = 0
    return depth, minor


def keeps(n):
    return [np.zeros(0, np.int64), np.arange(n), np.array([n - 1]), np.arange(0, n, 7)]


def run_shapes(ctx, tmp_path, S, sizes, keep_kinds=(0, 1, 2, 3)):
    k = 0
    for n in sizes:
        depth, minor = shape_arrays(S, n, 1000 * S + n)
        cf, cd = cells(depth, minor), cells(depth, None)
        for kk in keep_kinds:
            base = (0, 99990, 10 ** 12)[k % 3]           # ids cross 9 -> 10 and 99 999 -> 100 000
            header = ("" if k % 2 else "site_id\t" + "\t".join("s%d" % s for s in range(S)) + "\n")
            keep = keeps(n)[kk]
            check(ctx, tmp_path, depth, minor, keep, base, header, name="f_%d_%d" % (n, kk), c=cf)
            check(ctx, tmp_path, depth, None, keep, base, header, name="d_%d_%d" % (n, kk), c=cd)
            k += 1


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257, 1500])
def test_row_shapes(ctx, tmp_path, S):
    run_shapes(ctx, tmp_path, S, [1, 63, 64, 65, 1000])


@pytest.mark.parametrize("S", [65, 1500])
def test_batch_borders(ctx, tmp_path, monkeypatch, S):
    """A 4 KiB cap on a batch's text: a handful of rows a batch at 65 samples, and at 1500 samples every row (4 to 16 KB) longer
    than the cap -- a batch by itself.  The bytes do not change."""
    monkeypatch.setenv('MIDAS_SNPS_MERGE_TEXT_MB', SMALL_CAP)
    run_shapes(ctx, tmp_path, S, [1, 63, 64, 65, 1000])
    if S == 1500:
        depth, minor = shape_arrays(S, 65, 1000 * S + 65)
        assert min(len(r) for r in expected("", np.arange(65), depth, minor, 0).split(b'\n')[:-1]) > 4096


def test_upload_chunk_borders(ctx, tmp_path, monkeypatch):
    """The arrays go up in chunks of sites (a developer knob makes them small): kept rows on both sides of every border."""
    monkeypatch.setenv('MIDAS_SNPS_MERGE_CHUNK_SITES', '100')
    depth, minor = shape_arrays(5, 1000, 3)
    for kk, keep in enumerate([np.arange(1000), np.arange(0, 1000, 7), np.array([99, 100, 199, 200, 999]), np.array([450]), np.array([5, 5, 5, 700])]):
        check(ctx, tmp_path, depth, minor, keep, 10 ** 12, "h\n", name="f%d" % kk)
        check(ctx, tmp_path, depth, None, keep, 0, "", name="d%d" % kk)


def test_arguments_the_device_cannot_take(ctx, tmp_path):
    depth, minor = shape_arrays(3, 50, 1)
    path = str(tmp_path / "x.txt")
    with pytest.raises(abi.MidasSnpsError) as e:
        abi.write_merge_matrix_device(ctx, path, "", np.array([0, 50]), depth, minor)
    assert e.value.status == abi.ERR_INVALID_ARG
    bad = minor.copy()
    bad[1, 7] = depth[1, 7] = 5
    bad[1, 7] = 6
    with pytest.raises(abi.MidasSnpsError) as e:
        abi.write_merge_matrix_device(ctx, path, "h\n", np.arange(50), depth, bad)
    assert e.value.status == abi.ERR_INVALID_ARG and "minor count" in e.value.message
    assert os.listdir(str(tmp_path)) == []          # nothing under the final name, no temporary file left


# ---- the fused call ------------------------------------------------------------------------------------------------------------

def fused_check(ctx, tmp_path, args, counts, mean, base=0, header="site_id\tx\n", name="m"):
    prm = abi.MergeParams.from_args(args)
    ref = ctx.merge_sites(prm, counts, mean)
    fp, dp = str(tmp_path / (name + "_freq.txt")), str(tmp_path / (name + "_depth.txt"))
    got = ctx.merge_sites_tables(prm, counts, mean, fp, dp, header, site_id_base=base)
    for k in ('major', 'minor', 'snp_type', 'flag', 'count_samples', 'pooled'):
        assert np.array_equal(got[k], ref[k]), k
    keep = np.nonzero(ref['flag'] == 0)[0]
    assert got['n_keep'] == len(keep) and got['kernel_ms'] > 0
    hf, hd = str(tmp_path / (name + "_freq.host")), str(tmp_path / (name + "_depth.host"))
    abi.write_merge_matrix(hf, header, keep, ref['depth'], ref['minor_count'], threads=2, site_id_base=base)
    abi.write_merge_matrix(hd, header, keep, ref['depth'], None, threads=2, site_id_base=base)
    assert open(fp, 'rb').read() == open(hf, 'rb').read()
    assert open(dp, 'rb').read() == open(hd, 'rb').read()
    assert open(fp, 'rb').read() == expected(header, keep, ref['depth'], ref['minor_count'], base)
    assert not [f for f in os.listdir(str(tmp_path)) if '.tmp.' in f]
    return len(keep)


MEAN5 = [12.3, 11.0, 13.75, 9.5, 12.0]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_tables_match_merge_sites_and_the_host_writers(ctx, dataset, tmp_path, variant):
    args = dict(abi.DEFAULT_MERGE_ARGS, **VARIANTS[variant])
    kept = fused_check(ctx, tmp_path, args, [c.astype(np.uint32) for c in dataset['counts']], MEAN5, base=(0, 10 ** 12)[variant % 2])
    assert kept > 0 or variant > 1        # (a variant whose filters keep no site writes the headers alone)


def many_samples(n_samples, n=700):
    rng = np.random.default_rng(100 + n_samples)
    counts = []
    for s in range(n_samples):
        depth = rng.poisson(9.0, n)
        c = np.zeros((n, 4), np.int64)
        ref = rng.integers(0, 4, n)
        alt = (ref + 1 + rng.integers(0, 3, n)) % 4
        na = np.where(rng.random(n) < 0.2, rng.binomial(depth, 0.4), 0)
        c[np.arange(n), ref] = depth - na
        c[np.arange(n), alt] += na
        counts.append(c)
    for i in range(0, n, 9):          # counts past a byte, past 2^16 and near 2^31: every width of a depth cell
        counts[i % n_samples][i, i % 4] = (256 + 37 * i, 70000 + i, 2 ** 31 - 1 - i)[(i // 9) % 3]
    return [c.astype(np.uint32) for c in counts], [9.0 + 0.1 * s for s in range(n_samples)]


@pytest.mark.parametrize("n_samples", [1, 20, 65, 129])
def test_every_merge_kernel_family_feeds_the_formatter(ctx, tmp_path, n_samples):
    """1 and 20 samples: rows in registers; 65: a byte per count; 129: several waves per site."""
    counts, mean = many_samples(n_samples)
    # (depths are Poisson(9) against means of 9-22: most samples pass a site's depth filters, so most sites reach site_prev)
    args = dict(abi.DEFAULT_MERGE_ARGS, site_prev=0.5, snp_type=['any'])
    assert fused_check(ctx, tmp_path, args, counts, mean) > 350


def test_chunks_and_batches(ctx, dataset, tmp_path, monkeypatch):
    """No small input fills a chunk (the smallest holds 1024 sites of 4 GiB / (16 B x samples)): a developer knob cuts the
    6000 sites into chunks of 1000, and the text cap cuts every chunk's rows into batches."""
    monkeypatch.setenv('MIDAS_SNPS_MERGE_CHUNK_SITES', '1000')
    args = dict(abi.DEFAULT_MERGE_ARGS, snp_type=['any'], site_prev=0.0)
    counts = [c.astype(np.uint32) for c in dataset['counts']]
    assert fused_check(ctx, tmp_path, args, counts, MEAN5, name="chunks") == 6000
    monkeypatch.setenv('MIDAS_SNPS_MERGE_TEXT_MB', SMALL_CAP)
    assert fused_check(ctx, tmp_path, args, counts, MEAN5, base=99990, name="both") == 6000
    assert fused_check(ctx, tmp_path, dict(abi.DEFAULT_MERGE_ARGS), counts, MEAN5, name="core") > 0


def test_zero_mean_depth_is_reported_as_by_merge_sites(ctx, dataset, tmp_path):
    counts = [c.astype(np.uint32) for c in dataset['counts'][:2]]
    prm = abi.MergeParams.from_args(abi.DEFAULT_MERGE_ARGS)
    with pytest.raises(abi.MidasSnpsError) as ref:
        ctx.merge_sites(prm, counts, [10.0, 0.0])
    fp, dp = str(tmp_path / "freq.txt"), str(tmp_path / "depth.txt")
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.merge_sites_tables(prm, counts, [10.0, 0.0], fp, dp, "h\n")
    assert (e.value.status, e.value.message, e.value.read_index) == (ref.value.status, ref.value.message, ref.value.read_index)
    assert e.value.status == abi.ERR_MERGE_ZERO_MEAN_DEPTH
    assert os.listdir(str(tmp_path)) == []


# ---- the command ---------------------------------------------------------------------------------------------------------------

class _Shared:
    """The module's context, handed to run_pipeline: its close() leaves the context to the fixture."""
    def __init__(self, c):
        self.c = c

    def __enter__(self):
        return self.c

    def __exit__(self, *a):
        return False


def command_args(monkeypatch, outdir, dataset, *extra):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import merge_midas
    finally:
        sys.path.pop(0)
    monkeypatch.setattr(sys, 'argv', ['merge_midas.py', 'snps', outdir, '-i', os.path.dirname(dataset['samples'][0]), '-t', 'dir',
                                      '-d', dataset['db']] + list(extra))
    merge_midas.get_program()
    args = merge_midas.snps_arguments()
    merge_midas.check_arguments(args)
    return args


def read_tables(d):
    return tuple(open(os.path.join(d, 'snps_%s.txt' % k), 'rb').read() for k in ('info', 'freq', 'depth'))


def forbid_host_writer(monkeypatch):
    monkeypatch.setattr(abi, 'write_merge_matrix', lambda *a, **k: pytest.fail("the host writer was called"))


@pytest.mark.parametrize("flags,merge_args,max_sites", [
    ([], dict(abi.DEFAULT_MERGE_ARGS), None),
    (['--all_sites', '--max_sites', '777'], dict(abi.DEFAULT_MERGE_ARGS, snp_type=['any'], site_prev=0.0), 777),
])
def test_command_writes_the_tables_from_the_device(ctx, dataset, tmp_path, monkeypatch, capsys, flags, merge_args, max_sites):
    out = str(tmp_path / "merged")
    args = command_args(monkeypatch, out, dataset, *flags)
    monkeypatch.setenv('MIDAS_SNPS_MERGE_WRITERS', 'device')
    forbid_host_writer(monkeypatch)
    msnps.run_pipeline(args, make_context=lambda: _Shared(ctx))
    info, freq, depth = oracle_text(dataset, merge_args, max_sites=max_sites)
    assert len(info) > 20 and (max_sites is None or len(info) == max_sites)
    ids = "\t".join("sample_%d" % (k + 1) for k in range(5))
    got = read_tables(os.path.join(out, 'sp1'))
    assert got[0].decode() == INFO_HEADER + "".join(info)
    assert got[1].decode() == "site_id\t" + ids + "\n" + "".join(freq)
    assert got[2].decode() == "site_id\t" + ids + "\n" + "".join(depth)
    assert "%d sites, %d written (" % (6000 if max_sites is None else max_sites, len(info)) in capsys.readouterr().out


def test_host_switch_and_parts(ctx, dataset, tmp_path, monkeypatch):
    """MIDAS_SNPS_MERGE_WRITERS=device takes the device writers, =host and no setting the host writers, the bytes are the same; two parts by row range (site ids counted from
    the table's first row, the header in part 0 only, an empty third part) joined equal the whole-table run."""
    flags = ['--all_sites']
    whole = str(tmp_path / "whole")
    args = command_args(monkeypatch, whole, dataset, *flags)
    sp = merge.select_species(args, 'snps')[0]
    called = []
    real = abi.write_merge_matrix
    monkeypatch.setattr(abi, 'write_merge_matrix', lambda *a, **k: (called.append(1), real(*a, **k))[1])
    monkeypatch.setenv('MIDAS_SNPS_MERGE_WRITERS', 'device')
    assert msnps.merge_species(sp, args, ctx)[:2] == (6000, 6000) and not called
    want = read_tables(os.path.join(whole, 'sp1'))
    # the switch
    host = str(tmp_path / "host")
    hargs = command_args(monkeypatch, host, dataset, *flags)
    monkeypatch.setenv('MIDAS_SNPS_MERGE_WRITERS', 'host')
    msnps.merge_species(merge.select_species(hargs, 'snps')[0], hargs, ctx)
    assert len(called) == 2 and read_tables(os.path.join(host, 'sp1')) == want
    monkeypatch.delenv('MIDAS_SNPS_MERGE_WRITERS')      # no setting: the host writers
    msnps.merge_species(merge.select_species(hargs, 'snps')[0], hargs, ctx)
    assert len(called) == 4 and read_tables(os.path.join(host, 'sp1')) == want
    monkeypatch.setenv('MIDAS_SNPS_MERGE_WRITERS', 'device')
    # parts
    parts = str(tmp_path / "parts")
    pargs = command_args(monkeypatch, parts, dataset, *flags)
    psp = merge.select_species(pargs, 'snps')[0]
    for k, rows in enumerate([(0, 2501), (2501, 6000), (6000, 6000)]):
        msnps.merge_species(psp, pargs, ctx, rows, part=k)
    assert len(called) == 4
    first = open(os.path.join(parts, 'sp1', 'snps_freq.txt.part001'), 'rb').read()
    assert first.startswith(b'2502\t') and open(os.path.join(parts, 'sp1', 'snps_depth.txt.part002'), 'rb').read() == b''
    msnps.join_parts(psp, pargs, 3)
    assert read_tables(os.path.join(parts, 'sp1')) == want
