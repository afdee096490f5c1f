"""bench.py contract on CPU/gloo: `--gpus N` without a launcher spawns N rank
processes itself (reference: mp.spawn, model_parallel.py:160-162) and rank 0
prints ONE JSON line whose n_gpus is the real world size; `--parallel pipe`
runs the pipeline across those ranks."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--dtype", "fp32",
                        "--no-channels-last", "--steps", "1", "--warmup", "1", *extra],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    err = "\n".join(l for l in r.stderr.splitlines() if "hostname of the client" not in l and "[Gloo]" not in l)
    assert r.returncode == 0, err[-6000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_spawns_ranks_ddp():
    res = _run("--gpus", "2", "--model", "resnet18", "--batch-size", "2", "--image-size", "32")
    assert res["n_gpus"] == 2 and res["config"]["ranks"] == 2
    assert res["config"]["launcher"] == "bench-spawn"
    assert res["config"]["global_batch"] == 4 and res["scaling"] == "weak"
    assert res["config"]["grad_comm"] == "process_group"


def test_bench_pipe_two_stages():
    res = _run("--gpus", "2", "--parallel", "pipe", "--model", "mobilenetv2", "--batch-size", "8",
               "--micro-batches", "2", "--schedule", "gpipe")
    assert res["n_gpus"] == 2 and res["config"]["parallelism"] == "pipe2"
    assert res["config"]["global_batch"] == 8 and res["scaling"] == "strong"
    assert len(res["config"]["stage_partition"]) == 2
    assert res["ms_per_step"] > 0


def test_bench_syncbn_four_ranks():
    """DDP + SyncBatchNorm through bench.py on 4 gloo ranks: the moment
    all-reduces run across ranks (rehearse more ranks on CPU)."""
    res = _run("--gpus", "4", "--parallel", "syncbn", "--model", "resnet18", "--batch-size", "2",
               "--image-size", "32")
    assert res["n_gpus"] == 4 and res["config"]["ranks"] == 4
    assert res["config"]["sync_bn"] is True and res["config"]["parallelism"] == "ddp-syncbn4"
    assert res["config"]["global_batch"] == 8


def test_bench_pipe_reference_four_way_naive():
    """The reference's own experiment: MobileNetV2 cut 4 ways exactly as
    model_parallel.py:103,129,144 does, naive (one batch, serial ring) schedule."""
    res = _run("--gpus", "4", "--parallel", "pipe", "--model", "mobilenetv2", "--batch-size", "8",
               "--micro-batches", "1", "--schedule", "naive", "--partition", "reference")
    assert res["n_gpus"] == 4 and res["config"]["parallelism"] == "pipe4"
    assert res["config"]["schedule"] == "naive" and len(res["config"]["stage_partition"]) == 4
    assert res["ms_per_step"] > 0


def test_bench_dump_outputs_repeat_and_plain_run_is_lean(tmp_path):
    """--dump-outputs writes loss.npy (float32 [2], under 64 MB): the losses of
    two steps of the timed path from the rewound, seeded state.  With --warmup 1
    --steps 1 the run's own two steps started from that state, so the second
    dumped loss must equal the run's final loss: that holds only if the rewind
    put back the weights AND the optimizer state (momentum) of the start.  The
    state being rewound, the file is the same whatever --steps / --warmup were
    (the CPU path is deterministic).  A plain run carries none of the --full
    accounting."""
    import numpy as np

    args = ("--model", "resnet18", "--batch-size", "2", "--image-size", "32")
    res = [_run(*args, "--dump-outputs", str(tmp_path / "a")),
           _run(*args, "--dump-outputs", str(tmp_path / "b"), "--steps", "2", "--warmup", "2")]
    assert [r["steps"] for r in res] == [1, 2]  # a later --steps wins in argparse
    for r in res:
        assert r["ms_per_step"] > 0 and r["config"]["full"] is False
        assert not {"routes_per_step", "ddp_buckets", "ddp_comm", "rank_step_ms"} & set(r["config"])
    assert os.listdir(tmp_path / "a") == ["loss.npy"] == os.listdir(tmp_path / "b")
    a, b = (np.load(tmp_path / d / "loss.npy") for d in "ab")
    assert a.dtype == np.float32 and a.shape == (2,) and np.isfinite(a).all() and a.nbytes <= 64 * 2 ** 20
    assert np.array_equal(a, b), (a, b)
    # final_loss is printed to 4 decimals
    assert abs(float(a[1]) - res[0]["config"]["final_loss"]) <= 1e-4, (a, res[0]["config"]["final_loss"])
    # the update between the two steps shows: the second loss is not the first ...
    assert abs(float(a[1]) - float(a[0])) > 1e-3, a
    # ... and four training steps moved the loss the timed steps saw away from both
    assert min(abs(res[1]["config"]["final_loss"] - float(x)) for x in b) > 1e-3


def test_bench_full_accounting_does_not_count_the_dump_steps(tmp_path):
    """bench.py --full --dump-outputs: the dump's extra steps come after every
    counter is read, so the --full figures per timed step are those of the same
    run without the dump (2 gloo ranks: one buffer broadcast per dtype group per
    forward, the routes of the timed steps only)."""
    args = ("--gpus", "2", "--model", "resnet18", "--batch-size", "2", "--image-size", "32", "--full",
            "--steps", "2")
    plain, dumped = _run(*args), _run(*args, "--dump-outputs", str(tmp_path / "d"))
    assert os.listdir(tmp_path / "d") == ["loss.npy"]
    for r in (plain, dumped):
        b = r["config"]["ddp_buckets"]
        assert b["buffer_broadcasts_per_step"] == b["buffer_dtype_groups"] > 0, b
        assert r["config"]["routes_per_step"], r["config"]
    assert dumped["config"]["routes_per_step"] == plain["config"]["routes_per_step"]
    assert dumped["config"]["ddp_buckets"] == plain["config"]["ddp_buckets"]
    assert dumped["config"]["peak_mem_gb"] == plain["config"]["peak_mem_gb"]


def test_bench_dump_outputs_refuses_captured_steps():
    """Captured steps replay cached weight copies that the rewind would leave
    stale: --dump-outputs names the conflict for --graph, --dp-graphs and
    captured pipeline stages on a GPU, and for nothing else."""
    import bench
    from distributed_model_parallel_amd.train.step import StepConfig

    for cfg in (StepConfig(graph=True), StepConfig(parallel="dp", dp_graphs=True), StepConfig(parallel="pipe")):
        assert "--dump-outputs" in bench.dump_conflict(cfg, "cuda"), cfg
        assert bench.dump_conflict(cfg, "cpu") is None, cfg
    for cfg in (StepConfig(), StepConfig(parallel="syncbn"), StepConfig(parallel="dp"), StepConfig(parallel="none"),
                StepConfig(parallel="pipe", pipe_graphs=False)):
        assert bench.dump_conflict(cfg, "cuda") is None, cfg


def test_bench_ddp_label_and_single_rank_comm_flag():
    res = _run("--model", "resnet18", "--batch-size", "2", "--image-size", "32", "--single-rank-comm")
    assert res["config"]["parallelism"] == "ddp1" and res["config"]["single_rank_comm"] is True
    # at world size 1 the forced path goes through the process-group backend on CPU
    assert res["config"]["grad_comm"] == "process_group"
