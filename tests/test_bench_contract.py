"""CPU checks of bench.py's host-side contract (no GPU): --steps K times exactly K steps
laid out as training rounds, and the roofline `traffic` / MFMA-busy figures resolve to the
committed PMC summaries of the same workload under profiles/. One GPU test runs a plain
`bench.py --dump-outputs` end to end on a two-frame pool."""
import json
import os

import pytest

import bench


def test_rounds_cover_whole_training_rounds():
    # one whole round of n_step + 1 steps by default; --steps K times exactly K steps, in
    # rounds of 501 (the last one partial): (rounds started, timed steps)
    assert bench.rounds_for(None, 501) == (1, 501)
    assert bench.rounds_for(5, 501) == (1, 5)
    assert bench.rounds_for(501, 501) == (1, 501)
    assert bench.rounds_for(502, 501) == (2, 502)
    assert bench.rounds_for(1002, 501) == (2, 1002)
    with pytest.raises(SystemExit):
        bench.rounds_for(-1, 501)


class _CountingTrainer:
    """run_steps' view of a trainer on the CPU: reset_state() starts a round."""

    def __init__(self):
        self.rounds = []

    def reset_state(self, P=None):
        self.rounds.append(0)


def test_run_steps_times_exactly_the_requested_steps(monkeypatch):
    """run_steps calls the step exactly W + K times, re-initialises after the warm-up and at
    every 501-step round boundary, and returns the last step's output (host logic only: the
    device synchronisation and the phase events are stubbed)."""
    import torch

    class _Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

        def elapsed_time(self, other):
            return 1.0

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    for warmup, steps, want_rounds in ((2, 5, [5]), (0, 501, [501]), (3, 1005, [501, 501, 3])):
        fs, calls = _CountingTrainer(), []

        def step_fn(it, fs=fs, calls=calls):
            calls.append(it)
            if fs.rounds:
                fs.rounds[-1] += 1
            return {"it": it}

        dt, t_w, t_enq, out, prof = bench.run_steps(step_fn, fs, None, warmup, steps, 501, 1, None, phases=(20, 100))
        assert len(calls) == warmup + steps
        assert fs.rounds == want_rounds
        assert out == {"it": steps - 1}
        n_first = min(steps, 501)
        assert sum(int(k.split("_")[2]) - int(k.split("_")[1]) for k in prof) == n_first


def test_pmc_traffic_resolves_committed_headline_summary():
    t, src = bench.pmc_traffic("k_scatter", "headline", 64)
    assert t is not None and t > 0, src
    js = json.load(open(os.path.join(bench.ROOT, src)))
    assert js["_workload"] == "headline:64"
    assert js["k_scatter"]["traffic_bytes"] == t
    # a workload without a committed PMC pass reports None and says so
    t2, why = bench.pmc_traffic("k_scatter", "headline", 7)
    assert t2 is None and "no PMC pass" in why


def test_pmc_mfma_resolves_committed_summary():
    e = bench.pmc_mfma()
    assert e is not None
    # the MLP backward, and the forward's MLP kernel (k_mlp_fwd, or k_colour with the sigma net
    # inside the encode kernel)
    assert 0.0 < e["k_mlp_bwd"]["mfma_util"] < 1.0
    assert any(0.0 < e.get(k, {}).get("mfma_util", 0.0) < 1.0 for k in ("k_mlp_fwd", "k_colour"))
    assert e["source"].startswith("profiles/")


def test_algorithmic_bytes_per_unit_match_survey():
    # SURVEY §8d per-unit figures the roofline is priced with
    assert bench.ENC_FWD_B == 588
    assert bench.GRID_BWD_B == 1100
    assert bench.MLP_FWD_FLOP == 17792


def _bench(*argv, env_extra=None):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(bench.ROOT, "bench.py"), *argv], capture_output=True,
                          text=True, env=env, timeout=300)


def test_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus N` with no launcher starts the N ranks itself (a torch.distributed.run
    child process) and prints rank 0's JSON line with n_gpus = N (launch plumbing, --dry-run: gloo,
    no GPU)."""
    p = _bench("--gpus", "2", "--dry-run")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    js = json.loads(lines[0])
    assert js["n_gpus"] == 2 and js["dry_run"]


def test_gpus_must_match_external_launcher():
    p = _bench("--gpus", "4", "--dry-run", env_extra={"WORLD_SIZE": "2", "RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr
    p = _bench("--gpus", "1", "--dry-run")
    assert p.returncode == 0 and json.loads(p.stdout.strip())["n_gpus"] == 1


def test_stalled_rank_ends_every_rank_nonzero_within_timeout():
    """a rank that stalls in the exchange must not hang the job. With the
    collective timeout at 3 s and rank 1 stalling before its second collective, `bench.py --gpus 2
    --dry-run` (the same init_distributed / exchange.collective path the training exchange takes)
    exits non-zero well inside the stall, and the failing rank names its rank, step and phase."""
    import time
    t0 = time.time()
    p = _bench("--gpus", "2", "--dry-run",
               env_extra={"NOF_DRY_RUN_STALL_RANK": "1", "NOF_COLLECTIVE_TIMEOUT_S": "3"})
    dt = time.time() - t0
    assert p.returncode != 0, p.stderr[-2000:]
    assert dt < 11.0 + 30.0, dt          # the stall is 12 s; torch.distributed.run start-up included
    assert "rank 0 step 1 phase all_reduce" in p.stderr, p.stderr[-3000:]
    assert "dry_run" not in p.stdout


@pytest.mark.gpu
def test_plain_run_times_requested_steps_and_dumps_outputs(cuda_device, tmp_path):
    """A plain `bench.py --steps 3 --warmup 1 --dump-outputs DIR` (two-frame pool): the result line
    reports exactly 3 timed steps with ms_per_step and none of the --full measurements, and DIR
    holds the last step's outputs as finite float32 arrays."""
    import numpy as np
    d = tmp_path / "dump"
    p = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--pool-frames", "2", "--dump-outputs", str(d))
    assert p.returncode == 0, p.stderr[-2000:]
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["steps"] == 3 and js["warmup"] == 1 and js["n_gpus"] == 1
    assert js["ms_per_step"] > 0 and js["unit"] == "rays/s" and js["higher_is_better"] is True
    # value = rays per step / step time; ms_per_step is rounded to 3 decimals, value to 1
    rel = 0.0005 / js["ms_per_step"] + 1e-6
    assert abs(js["value"] - js["config"]["rays_per_step"] / (js["ms_per_step"] * 1e-3)) <= 2 * rel * js["value"]
    for k in ("kernels", "roofline", "other_execution", "config2", "parity_mode", "config1", "cpu_baseline"):
        assert k not in js, k
    files = sorted(os.listdir(d))
    assert files == ["fs_rgb_loss.npy", "loss_terms.npy"]
    arrays = {f: np.load(d / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert arrays["loss_terms.npy"].shape == (8,) and arrays["fs_rgb_loss.npy"].shape == (1,)
    assert abs(float(arrays["loss_terms.npy"][:4].sum()) - js["loss"]) <= 1e-4 * abs(js["loss"]) + 1e-5
