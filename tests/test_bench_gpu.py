"""Config 5 (BASELINE.json configs[4]: 1 B pairs, C5 options, 8 GPUs, RCCL Stats reduce) as far as
one GPU goes: bench.py runs rank 7's full 125 M-pair shard (global pair indices 875 M .. 1 B) on
this GPU through a real (world-1) RCCL process group, so the accumulator all-reduce of the
product path runs on hardware, and its post-timing parity sample of that shard must agree with
the oracle (the checker).  The driver's 8-GPU SCALE run launches the same code with 8 ranks."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_config5_rank7_shard_through_rccl():
    import bench

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench.free_port()))
    cmd = [sys.executable, "-u", os.path.join(REPO, "bench.py"), "--config", "C5", "--pairs", "125000000",
           "--shard", "7/8", "--pg", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--engine-pairs", "0", "--paths-pairs", "0", "--sample-pairs", "1000000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=840, env=env, cwd=REPO)
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["pairs_per_gpu"] == 125_000_000
    assert out["config"]["first_index"] == 875_000_000
    assert "process group (nccl) closed" in r.stderr
    s = out["parity_sample"]
    assert s["ok"] and s["full_run_records_equal"] and s["sample_run_acc_equal"], s
    assert out["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(oracle, tmp_path):
    """A plain `bench.py --dump-outputs DIR` run (no side legs) on 600,000 pairs, whose 1.2 M records are
    more than the dump's sample: the accumulator block and the sampled records of the last timed
    step, written as float arrays, equal the oracle's over the same synthetic pairs."""
    import numpy as np

    import bench
    from batch_util import synth_pack
    from fqtool_amd import abi
    from sample_parity import oracle_parallel

    n = 600_000
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--pairs", str(n),
           "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["roofline"]["frac"] > 0
    for leg in ("parity_sample", "engine", "paths", "e2e", "cpu_baseline"):
        assert out[leg] is None, leg
    pk = synth_pack(oracle, n, True, first=0)
    pk.batch()
    ores, oacc = oracle_parallel(oracle, bench.config_params(abi, "C3"), pk._tiled, pk.len1, pk.len2, n, pk.stride)
    acc = np.load(tmp_path / "accumulator.npy")
    assert acc.dtype == np.float64 and np.array_equal(acc, oacc.astype(np.float64))
    idx = np.load(tmp_path / "record_index.npy")
    assert np.array_equal(idx, bench.sample_rows(2 * n, bench.DUMP_RECORDS).astype(np.float64))
    rec = np.load(tmp_path / "records.npy")
    assert rec.dtype == np.float32 and rec.shape == (bench.DUMP_RECORDS, len(abi.RESULT_DTYPE_FIELDS))
    want = ores[idx.astype(np.int64)]
    for j, (f, _) in enumerate(abi.RESULT_DTYPE_FIELDS):
        assert np.array_equal(rec[:, j], want[f].astype(np.float32)), f
