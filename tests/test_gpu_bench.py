"""bench.py's N > 1 code on ONE real GPU: two processes that share device 0 and talk over gloo (MIDAS_BENCH_ONE_GPU=1; RCCL refuses
two ranks on one device) -- the launch, the rank arithmetic, the timed region with its all-gather, the configs3_strong block and
the one JSON line are the ones the driver's `torch.distributed.run --nproc-per-node N bench.py --gpus N` goes through."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_of_bench_py_on_one_gpu():
    port = _free_port()
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    procs = []
    for k in range(2):
        env = dict(base, RANK=str(k), LOCAL_RANK=str(k), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MIDAS_BENCH_ONE_GPU="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c2", "--steps", "5",
                                       "--warmup", "2", "--sustain-seconds", "0", "--no-pmc"],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT))
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=1500)
        assert p.returncode == 0, e[-3000:]
        outs.append(o)
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not [ln for ln in outs[1].splitlines() if ln.startswith("{")]        # rank 0 prints the one line
    d = json.loads(lines[0])
    # N > 1: the line's own value is configs[3] -- BASELINE's multi-GPU configuration, ONE sample dealt to the ranks (strong) --
    # and the per-rank configs[2]-style replicas are a block of their own
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "strong" and d["unit"] == "sites/s"
    assert d["config"]["workload"].startswith("configs[3]") and d["config"]["sites_per_gpu"] == 200000000
    c3 = d["configs3_strong"]
    assert c3["ranks"] == 2 and c3["scaling"] == "strong" and c3["total_sites"] == 400000000 and c3["reads_counted_once"] is True
    assert len(c3["per_rank_ms_per_step"]) == 2 and c3["partition"]["weight_max_over_mean"] < 1.1
    assert d["value"] == c3["value"] and d["ms_per_step"] == c3["ms_per_step"] and c3["steps"] == 5
    # the whole job: every site of the sample, K times, over the slowest rank's time
    assert abs(d["value"] - 400000000 * 5 / (d["ms_per_step"] * 5 / 1e3)) / d["value"] < 1e-6
    assert 0.0 < d["roofline"]["frac"] < 1.0 and len(d["per_rank_ms_per_step"]) == 2
    w = d["weak_replicas"]
    assert w["scaling"] == "weak" and w["sites_per_gpu"] == 15000000 and "roofline" in w
    assert abs(w["value"] - 2 * 15000000 * 5 / (w["ms_per_step"] * 5 / 1e3)) / w["value"] < 1e-6


def test_dump_outputs_hold_the_last_timed_steps_results(tmp_path):
    """A plain one-GPU run with --dump-outputs: the line's headline fields, nothing of --full, and .npy files that hold what the
    C oracle computes for the same seeded inputs (the sampled sites, every site's sums per contig, the per-species counters)."""
    import numpy as np
    from midas_amd import abi, synth
    from oracle import c_oracle
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "4", "--warmup", "1",
                        "--sustain-seconds", "0", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 4 and d["unit"] == "sites/s" and d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 15000000 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    assert not {"cpu_baseline", "parity_vs_oracle", "resident_packed", "merge50", "stage_e2e", "bam_decode"} & set(d)
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert set(files) == {"site_index.npy", "counts.npy", "ref_allele.npy", "counts_per_contig.npy", "species_stats.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
    contigs, reads = synth.make_dataset(workers=4, **synth.CONFIGS["c2"])
    st, _, oc, oa, os_ = c_oracle.pileup(abi.Thresholds.from_args(abi.DEFAULT_ARGS), contigs, reads)
    assert st == 0
    idx = files["site_index.npy"].astype(np.int64)
    assert idx.size > 500000 and np.all(np.diff(idx) > 0) and idx[-1] < contigs.n_sites
    assert np.array_equal(files["counts.npy"], oc[idx].astype(np.float64))
    assert np.array_equal(files["ref_allele.npy"], oa[idx].astype(np.float32))
    off = contigs.site_offsets()
    assert np.array_equal(files["counts_per_contig.npy"], np.add.reduceat(oc.astype(np.uint64), off[:-1], axis=0).astype(np.float64))
    assert np.array_equal(files["species_stats.npy"], os_.astype(np.float64))
