"""bench.py's output contract (one JSON line with the driver's fields + roofline + cpu_baseline),
its single clock, and its self-launch of N ranks."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)                      # a clean environment: no launcher above us
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True,
                         text=True, timeout=900, env=e)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_json_contract_small_batch():
    d = run_bench("--boards", "65536", "--steps", "40", "--warmup", "5", "--cpu-budget", "2", "--no-legs", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "cpu_baseline", "clock", "regions", "host_wall_ms_per_step"):
        assert k in d, k
    assert d["metric"] == "env_steps_per_sec" and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 == d["ranks_seen"] and d["steps"] == 40 and d["warmup"] == 5 and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["config"]["replay_matches_recording"] is True
    assert d["regions"] >= 5
    r = d["roofline"]
    sb = d["config"]["state_bytes_per_board"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["algorithmic_bytes_per_board_step"] == 2 * sb + 7
    assert r["algorithmic_bytes_per_launch"] == (2 * sb + 7) * 65536
    # ONE clock: value, ms_per_step and the roofline fraction are the same measurement
    assert abs(d["value"] - 65536 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    assert abs(d["value"] * (2 * sb + 7) / 8e12 - r["frac"]) / r["frac"] < 1e-9
    assert abs(r["launch_us"] - d["ms_per_step"] * 1e3) < 1e-9
    assert d["host_wall_ms_per_step"] >= d["ms_per_step"] * 0.98
    assert (r["traffic"] is None) == (r["traffic_source"] is None)
    # the committed PMC figure says whether it was collected on the step-kernel sources this run was built from
    assert r["traffic_measured_on_this_build"] in (True, False, None) and (r["traffic"] is None) == (r["traffic_measured_on_this_build"] is None)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "steps/s" and c["cores"] >= 1 and c["value"] > 1e6
    assert c["python_interpreter_steps_per_s"] > 1e4
    # a one-thread figure, the box's nproc and CPU model beside the all-threads one
    assert 1e6 < c["threads1"] <= c["value"] * 1.05 and c["nproc"] >= c["cores"] and isinstance(c["cpu_model"], str)
    # ... and the all-host-cores pass (os.cpu_count() threads) beside the GPU's 16-core share
    assert c["threads_all_cores"] == c["nproc"] and c["threads_all"] > c["threads1"]
    assert 1 <= c["cpus_allowed"] <= c["nproc"] and "cgroup_cpu_max" in c      # why all cores may read lower than the share
    assert "threads_all" in c["sample"] and "threads1" in c["sample"]
    assert "legs" not in d


def test_bench_modes_agree_on_the_episode_counters():
    common = ("--boards", "16384", "--steps", "30", "--warmup", "5", "--no-cpu-baseline", "--no-legs")
    a = run_bench(*common)
    b = run_bench(*common, "--mode", "random")
    c = run_bench(*common, "--mode", "gym")
    f = run_bench(*common, "--mode", "random-fused", "--fused-steps", "8")        # 30 steps = launches of 8 + 8 + 8 + 6
    assert (a["config"]["episodes_finished"] == b["config"]["episodes_finished"] == c["config"]["episodes_finished"]
            == f["config"]["episodes_finished"] > 0)
    assert b["config"]["replay_matches_recording"] is True and c["config"]["replay_matches_recording"] is True
    assert f["config"]["replay_matches_recording"] is True and f["steps"] == 30
    assert f["roofline"]["kernel"].startswith("step_random_fused_kernel")
    sb = c["config"]["state_bytes_per_board"]
    assert c["roofline"]["algorithmic_bytes_per_board_step"] == 2 * sb + 7 + 30


def test_bench_gpus_2_starts_its_own_two_ranks():
    """`python bench.py --gpus 2` with a clean environment must itself start 2 ranks (here both on the
    one GPU of the box, rendezvous over gloo) and report what the process group saw."""
    d = run_bench("--gpus", "2", "--boards", "32768", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                  env={"QTTT_DIST_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2
    assert d["config"]["self_launched"] is True and d["config"]["dist_backend"] == "gloo"
    assert d["config"]["boards_total"] == 65536
    assert d["config"]["board_offset_last_rank"] == 32768          # shard 1 starts at global board B
    assert d["config"]["parallelism"] == "shard2"
    assert d["config"]["replay_matches_recording"] is True
    assert abs(d["value"] - 2 * 32768 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    g = d["returns_gather"]                                         # the optional exchange, off the step path
    assert g["boards_gathered"] == 65536 and g["bytes_per_rank"] == 4 * 32768 and g["ms"] > 0


def test_bench_default_line_carries_the_legs():
    """the --full line carries the other BASELINE configurations and modes, measured
    in the same process on the same clock, and the whole run stays short."""
    import time
    t0 = time.time()
    d = run_bench("--steps", "20", "--warmup", "5", "--cpu-budget", "2", "--full")
    assert time.time() - t0 < 120
    assert d["config"]["boards_per_gpu"] == 1 << 20 and d["config"]["mode"] == "replay"
    legs = {l["name"]: l for l in d["legs"]}
    sb = d["config"]["state_bytes_per_board"]
    for name in ("config2_4096_boards", "config3_262144_boards", "beyond_infinity_cache_16777216_boards",
                 "gym_1048576_boards", "random_1048576_boards", "random_fused_1048576_boards",
                 "random_fused_262144_boards", "random_fused_4096_boards", "config5_expand_rollout_65536_pairs"):
        assert name in legs, name
    for name in ("observe", "export", "import", "turn", "check_win", "node_info", "state_keys", "node_info_python_key",
                 "expand", "expand_python_key", "rollout", "encode"):
        assert "row_%s_1048576_boards" % name in legs, name
    assert legs["row_export_1048576_boards"]["algorithmic_bytes_per_board"] == sb + 37
    for l in d["legs"]:
        assert l["regions"] >= 5 and 0 < l["frac"] < 1 and l["achieved_GBps"] > 0
        if "us_per_step" in l:
            assert l["replay_matches_recording"] is True, l["name"]
            assert abs(l["steps_per_s"] - l["boards"] / (l["us_per_step"] * 1e-6)) / l["steps_per_s"] < 1e-9
    sb = d["config"]["state_bytes_per_board"]
    assert legs["beyond_infinity_cache_16777216_boards"]["algorithmic_bytes_per_board_step"] == 2 * sb + 7
    assert 16777216 * (2 * sb) > 256 << 20                                     # the state alone exceeds the Infinity Cache
    assert legs["gym_1048576_boards"]["algorithmic_bytes_per_board_step"] == 2 * sb + 7 + 30
    c5 = legs["config5_expand_rollout_65536_pairs"]
    assert c5["us_per_unit_with_10_playouts_per_leaf"] < c5["us_per_unit"] + 9 * 9.0      # ten playouts per leaf: one launch, not ten
    assert c5["us_per_unit"] < c5["us_per_unit_as_three_launches"]                        # one launch beats the composition
    assert 1.0 < c5["children_per_pair"] < 1.6
    # the native position key costs a fraction of the CPython-exact one
    assert legs["row_node_info_1048576_boards"]["us_per_launch"] < 0.8 * legs["row_node_info_python_key_1048576_boards"]["us_per_launch"]
    assert legs["row_expand_1048576_boards"]["us_per_launch"] < 0.85 * legs["row_expand_python_key_1048576_boards"]["us_per_launch"]
    # both roofline fractions in the line: against the spec and against the achievable copy rate, and the same
    # kernel beyond the Infinity Cache
    r = d["roofline"]
    assert r["achievable_peak"] == 6290.0 and abs(r["frac_of_achievable"] - r["achieved"] / 6290.0) < 1e-9
    assert r["state_resident_in_infinity_cache"] is True
    bc = r["beyond_cache"]
    assert bc["boards"] == 16777216 and abs(bc["frac"] - legs["beyond_infinity_cache_16777216_boards"]["frac"]) < 1e-12
    assert bc["working_set_MB"] > 256
    f = legs["random_fused_262144_boards"]
    assert f["bound"] == "valu" and f["steps_per_launch"] == 64 and f["us_per_step"] < legs["config3_262144_boards"]["us_per_step"]
    assert 0.3 < f["issue_frac"] < 1.0 and 0.5 < legs["random_fused_1048576_boards"]["issue_frac"] < 1.05


def test_bench_line_survives_a_failing_returns_gather():
    """the gather of per-board returns is optional bookkeeping; when it raises (here: injected on
    both ranks) the line still prints, rc 0, with the scaling value intact and the error inside it.  And
    QTTT_BENCH_NO_GATHER=1 skips it."""
    common = ("--gpus", "2", "--boards", "32768", "--steps", "20", "--warmup", "5", "--no-cpu-baseline")
    d = run_bench(*common, env={"QTTT_DIST_BACKEND": "gloo", "QTTT_BENCH_FAIL_GATHER": "1"})
    assert d["n_gpus"] == 2 == d["ranks_seen"] and d["value"] > 0 and d["config"]["replay_matches_recording"] is True
    assert "injected failure" in d["returns_gather"]["error"] and "ms" not in d["returns_gather"]
    assert abs(d["value"] - 2 * 32768 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    e = run_bench(*common, env={"QTTT_DIST_BACKEND": "gloo", "QTTT_BENCH_NO_GATHER": "1"})
    assert e["returns_gather"] == {"skipped": "QTTT_BENCH_NO_GATHER=1"} and e["ranks_seen"] == 2


def test_bench_line_survives_a_returns_gather_that_never_returns():
    """The single-shot 8-GPU run must not lose its value to a collective that hangs (an RCCL this code has never run on
    that node): the exchange runs under a deadline.  Here rank 1 never joins it (injected), rank 0 blocks in the gather;
    after QTTT_BENCH_GATHER_TIMEOUT both give up, rank 0 prints the line with the error inside, every rank leaves with 0."""
    import time
    t0 = time.time()
    d = run_bench("--gpus", "2", "--boards", "32768", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                  env={"QTTT_DIST_BACKEND": "gloo", "QTTT_BENCH_HANG_GATHER": "rank1", "QTTT_BENCH_GATHER_TIMEOUT": "8"})
    assert time.time() - t0 < 150
    assert d["n_gpus"] == 2 == d["ranks_seen"] and d["value"] > 0 and d["config"]["replay_matches_recording"] is True
    assert "TimeoutError" in d["returns_gather"]["error"] and "ms" not in d["returns_gather"]
    assert len(d["per_rank_ms_per_step"]) == 2 and d["config"]["episodes_finished"] > 0
    assert abs(d["value"] - 2 * 32768 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9


def test_bench_total_boards_is_strong_scaling():
    """BASELINE config 4's shape: a fixed total sharded over the ranks (here 2 ranks on the one GPU over gloo,
    an odd total so the shards differ by one board)."""
    d = run_bench("--gpus", "2", "--total-boards", "65537", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                  env={"QTTT_DIST_BACKEND": "gloo"})
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 == d["ranks_seen"]
    assert d["config"]["boards_total"] == 65537 and d["config"]["boards_per_gpu"] == 32769
    assert d["config"]["board_offset_last_rank"] == 32769
    assert d["config"]["replay_matches_recording"] is True
    assert abs(d["value"] - 65537 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    assert d["returns_gather"]["boards_gathered"] == 65537
    one = run_bench("--total-boards", "65537", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-legs")
    assert one["scaling"] == "strong" and one["config"]["boards_per_gpu"] == 65537
    assert one["config"]["episodes_finished"] == d["config"]["episodes_finished"]     # the same boards, whatever the sharding


def test_bench_rccl_branch_with_one_rank():
    """The N > 1 code path on the real backend: process group on RCCL ("nccl"), device barrier,
    all_reduce of the clock / the rank count / the episode counters, the returns gather — with the
    one rank a one-GPU box can give it (two ranks on one GPU are refused by RCCL itself)."""
    d = run_bench("--boards", "65536", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-legs",
                  env={"QTTT_DIST_FORCE": "1", "QTTT_DIST_BACKEND": "nccl"})
    assert d["n_gpus"] == 1 == d["ranks_seen"] and d["config"]["dist_backend"] == "nccl"
    assert d["config"]["control_backend"] == "gloo"              # bookkeeping over gloo, the exchange over RCCL
    assert d["returns_gather"]["backend"] == "nccl" and d["returns_gather"]["boards_gathered"] == 65536
    assert d["returns_gather"]["bring_up_ms"] > 0                # the first device collective: RCCL really came up
    assert d["config"]["replay_matches_recording"] is True
    # the layout of rounds 1 - 4 (everything on RCCL, eager communicator) stays available
    c = run_bench("--boards", "65536", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-legs",
                  env={"QTTT_DIST_FORCE": "1", "QTTT_DIST_BACKEND": "nccl", "QTTT_BENCH_CONTROL": "nccl"})
    assert c["config"]["control_backend"] == "nccl" and c["returns_gather"]["boards_gathered"] == 65536
    assert c["config"]["episodes_finished"] == d["config"]["episodes_finished"]
    e = run_bench("--boards", "65536", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-legs")
    assert e["config"]["dist_backend"] is None and e["returns_gather"] is None
    assert e["config"]["episodes_finished"] == d["config"]["episodes_finished"]


def test_bench_refuses_more_ranks_than_gpus_on_rccl():
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "QTTT_DIST_BACKEND"):
        e.pop(k, None)
    import torch
    n = torch.cuda.device_count() + 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--boards", "4096",
                          "--steps", "5", "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True,
                         timeout=600, env=e)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_bench_under_torchrun_two_ranks():
    """The driver's own launch line for N > 1: python -m torch.distributed.run ... bench.py --gpus 2
    (ranks from the environment, no self-launch), here with both ranks on the one GPU over gloo."""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    e = dict(os.environ, QTTT_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--boards", "16384", "--steps", "10", "--warmup", "2"],
                         capture_output=True, text=True, timeout=900, env=e)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["config"]["self_launched"] is False
    assert "cpu_baseline" not in d                                      # rank 0 at N = 1 only


def test_bench_two_ranks_on_rccl_when_two_gpus_are_visible():
    """The real N > 1 path — one rank per GPU, process group on RCCL, device barrier, device all_reduces and the
    returns gather over xGMI.  Needs two GPUs: skipped on the one-GPU boxes this suite normally runs on (DESIGN.md §8
    lists these calls as never executed with world > 1 until a node runs this test or the driver's SCALE bench)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL refuses two ranks on one device)")
    d = run_bench("--gpus", "2", "--boards", "262144", "--steps", "20", "--warmup", "5", "--no-cpu-baseline")
    assert d["n_gpus"] == 2 == d["ranks_seen"] and d["config"]["dist_backend"] == "nccl"
    assert d["config"]["replay_matches_recording"] is True and d["scaling"] == "weak"
    assert d["returns_gather"]["backend"] == "nccl" and d["returns_gather"]["boards_gathered"] == 2 * 262144
    s = run_bench("--gpus", "2", "--total-boards", "524288", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                  "--mode", "random-fused")
    assert s["scaling"] == "strong" and s["config"]["boards_per_gpu"] == 262144 and s["ranks_seen"] == 2
    one = run_bench("--boards", "524288", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-legs")
    assert one["config"]["episodes_finished"] == d["config"]["episodes_finished"]      # the same 524 288 boards, sharded or not


def test_plain_run_times_exactly_the_steps_asked_and_nothing_else():
    """A plain run: one region of exactly --steps timed steps, no legs, no CPU baseline, the headline fields."""
    d = run_bench("--boards", "65536", "--steps", "30", "--warmup", "3")
    assert d["steps"] == 30 and d["warmup"] == 3 and d["regions"] == 1
    assert "legs" not in d and "cpu_baseline" not in d and "configs" not in d
    assert d["metric"] == "env_steps_per_sec" and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u64" and d["ms_per_step"] > 0
    assert abs(d["value"] - 65536 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    assert d["config"]["replay_matches_recording"] is True


def test_dump_outputs_are_reproducible_and_chunking_does_not_change_them(tmp_path):
    """--dump-outputs: the last timed step's reward / terminated and the boards after it, float32, identical from run
    to run; a recording cap of 16 steps (the stream recorded and replayed in chunks) computes the same."""
    import numpy as np
    common = ("--boards", "65536", "--steps", "100", "--warmup", "7")
    a = run_bench(*common, "--dump-outputs", str(tmp_path / "a"))
    b = run_bench(*common, "--dump-outputs", str(tmp_path / "b"))
    c = run_bench(*common, "--dump-outputs", str(tmp_path / "c"), env={"QTTT_BENCH_RECORD_BYTES": str(8 * 65536 * 16)})
    names = sorted(os.listdir(tmp_path / "a"))
    assert "reward.npy" in names and "terminated.npy" in names and "board_board.npy" in names
    assert sorted(os.listdir(tmp_path / "b")) == names == sorted(os.listdir(tmp_path / "c"))
    total = 0
    for n in names:
        x = np.load(tmp_path / "a" / n)
        total += x.nbytes
        assert x.dtype == np.float32 and x.shape[0] == 65536, n
        assert np.array_equal(x, np.load(tmp_path / "b" / n)) and np.array_equal(x, np.load(tmp_path / "c" / n)), n
    assert total <= 64 << 20
    for d in (a, b, c):
        assert d["config"]["replay_matches_recording"] is True and d["steps"] == 100
    assert a["config"]["episodes_finished"] == c["config"]["episodes_finished"] > 0
