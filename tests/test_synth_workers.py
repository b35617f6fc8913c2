"""make_dataset(workers > 1) -- what bench.py uses -- generates the chunks of reads in threads, each from the generator state the
serial loop would have reached there.  The arrays must be the serial ones, bit for bit, and stay so when the plan of those
states is wrong (a chunk that started elsewhere is run again)."""
import numpy as np
import pytest

from midas_amd import synth

CASES = [dict(n_species=2, contigs_per_species=3, contig_len=30011, n_reads=60000, seed=5, var_len=True, lowercase_frac=0.05,
              chunk=4096),
         dict(n_species=1, contigs_per_species=4, contig_len=20000, n_reads=50001, seed=9, chunk=4000)]


def _same(a, b):
    (c1, r1), (c2, r2) = a, b
    for k in ("length", "species", "read_begin", "ref"):
        assert np.array_equal(getattr(c1, k), getattr(c2, k)), k
    d1, d2 = r1.as_dict(), r2.as_dict()
    assert d1.keys() == d2.keys()
    for k in d1:
        assert d1[k].dtype == d2[k].dtype and np.array_equal(d1[k], d2[k]), k


@pytest.mark.parametrize("cfg", CASES)
def test_threads_make_the_serial_arrays(cfg):
    _same(synth.make_dataset(**cfg), synth.make_dataset(workers=4, **cfg))


def test_a_wrong_plan_still_makes_the_serial_arrays(monkeypatch):
    calls = []
    real = synth._parallel_chunks

    def counted(rng, bounds, L, reads_chunk, workers):
        def chunk(g, lo, hi):
            calls.append(lo)
            reads_chunk(g, lo, hi)
        real(rng, bounds, L, chunk, workers)
    monkeypatch.setattr(synth, "_parallel_chunks", counted)
    monkeypatch.setattr(synth, "_rejected", lambda rng_excl, bits: [])     # the plan ignores every rejection
    cfg = CASES[1]
    got = synth.make_dataset(workers=4, **cfg)
    assert len(calls) > len(range(0, cfg["n_reads"], cfg["chunk"]))       # chunks were run again
    monkeypatch.undo()
    _same(synth.make_dataset(**cfg), got)


@pytest.mark.parametrize("rng_excl", [3, 4, 5, 7, 18, 28])
def test_rejected_values_follow_numpys_bounded_draws(rng_excl):
    x = np.arange(1 << 16, dtype=np.uint64)
    assert sorted(synth._rejected(rng_excl, 16)) == np.flatnonzero(((x * rng_excl) & 0xFFFF) < (1 << 16) % rng_excl).tolist()
    vals = synth._rejected(rng_excl, 32)
    assert len(set(vals)) == len(vals) and all((v * rng_excl) % (1 << 32) < (1 << 32) % rng_excl for v in vals)
