"""-m gpu: bench.py end to end -- the JSON contract of the single-process line and the N = 2 data-parallel path launched the way the
driver launches it (python -m torch.distributed.run ... bench.py --gpus 2), over gloo on the one GPU of the test box (RCCL refuses two
ranks on one device; everything but the transport is the production path: per-rank batches, the two overlapped collectives, the
1/world prescale, max-over-ranks timing).  Reduced batch and step counts: the figures mean nothing here, the plumbing does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json_line(text):
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            return json.loads(line)
    raise AssertionError("no JSON line in:\n" + text[-2000:])


def test_bench_single_process_line_contract():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--blocks", "3", "--pairs", "16", "--full", "--no-extras",
                        "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json_line(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "timing"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["dtype"] == "f16" and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert len(out["timing"]["block_ms_per_step"]) == 3
    assert abs(out["value"] - 2 * 16 * 3 * 3.0 / (out["ms_per_step"] * 3 / 1e3)) < 1e-6 * out["value"]
    roof = out["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and 0 < roof["frac"] < 1 and "kernel_symbol" in roof and "source" in roof
    assert set(roof["families_serial"]) == {"vm_conv_fwd", "vm_conv_dgrad", "vm_conv_wgrad"}


def test_bench_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """A plain run times exactly --steps steps (one block), carries no side figures, and --dump-outputs writes what its last step
    computed: float32 arrays of the documented shapes, finite, at most 64 MB, and the same bits from a second run with the same
    arguments (seeded inputs and weights, deterministic step)."""
    pairs = 16
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--pairs", str(pairs), "--dump-outputs",
                            str(tmp_path / tag)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(_last_json_line(r.stdout))
    out = lines[0]
    assert out["steps"] == 3 and out["timing"]["blocks"] == 1 and len(out["timing"]["block_ms_per_step"]) == 1
    assert abs(out["timing"]["block_ms_per_step"][0] - out["ms_per_step"]) < 1e-3 * out["ms_per_step"] + 1e-4
    assert abs(out["value"] - 2 * pairs * 3 * 3.0 / (out["ms_per_step"] * 3 / 1e3)) < 1e-6 * out["value"]
    for key in ("roofline", "precision", "extras", "cpu_baseline"):
        assert key not in out, key
    shapes = {"loss_acc": (2,), "pred": (pairs,), "emb": (2 * pairs, 64)}
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in ("loss_acc", "pred", "emb", "params", "adam_m", "adam_v", "bn_moving"))
    total = 0
    for n in names:
        x, x2 = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        total += x.nbytes
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        assert x.shape == shapes.get(n[:-4], x.shape), n
        assert np.array_equal(x, x2), n
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "a" / "loss_acc.npy")[0]) == out["config"]["final_loss"]


def test_bench_counts_the_dominant_launch_traffic_in_the_run():
    """roofline.traffic is COUNTED by the run that reports it: bench.py, at the headline batch, runs the two
    rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) on a child process of itself and folds them with tools/pmc_traffic.py; the
    committed figure of another box rides along and must agree."""
    import shutil
    if shutil.which("rocprofv3") is None and not os.path.exists("/opt/rocm/bin/rocprofv3"):
        pytest.skip("no rocprofv3 on this box")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("ROCP_", "ROCPROF"))}
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--blocks", "1", "--full", "--no-extras", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    roof = _last_json_line(r.stdout)["roofline"]
    if not roof.get("traffic_source", "").startswith("counted in this run"):   # the line says why and carries the committed figure instead
        pytest.skip("rocprofv3 --pmc did not run on this box: " + str(roof.get("traffic_source")))
    assert 0.95 * roof["algorithmic_bytes"] < roof["traffic"] < 1.3 * roof["algorithmic_bytes"]
    assert roof["traffic_committed"] is None or abs(roof["traffic"] / roof["traffic_committed"] - 1.0) < 0.05
    v = roof["vendor_gemm"]
    assert v["ms"] > 0 and v["m_n_k"] == [256 * roof["launch_shape"]["L"], v["m_n_k"][1], v["m_n_k"][2]]


@pytest.mark.parametrize("launch", ["self"])
def test_bench_two_ranks_over_gloo(launch):
    """Plain ``python bench.py --gpus 2`` -- no RANK in the environment: bench.py spawns the two ranks itself by re-executing its own
    command line under ``python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 ...``, i.e. the
    driver's documented N > 1 form is what actually runs underneath (a separate ``torchrun`` case would time the same path twice;
    ``launch="torchrun"`` still works when run by hand).  The line must say n_gpus 2."""
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    port = str(29500 + (os.getpid() + 13) % 2000)
    tail = ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--blocks", "2", "--pairs", "16"]
    cmd = [sys.executable] + ([] if launch == "self" else ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                                           "--master-addr", "127.0.0.1", "--master-port", port]) + tail
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json_line(r.stdout)
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["config"]["global_pairs"] == 32
    assert out["config"]["final_loss"] == out["config"]["final_loss"] and abs(out["config"]["final_loss"]) < 10   # finite
    dp = out["data_parallel"]
    assert dp["backend"] == "gloo" and dp["world_size"] == 2 and len(dp["rank_ms_per_step"]) == 2
    assert abs(dp["collectives_per_step"] - 2.0) < 1e-9 and dp["flat_gradient_bytes"] > 4_000_000
    assert dp["replicas_bit_identical_after_timed_steps"] is True and dp["rccl_version"] is None and len(dp["rank_devices"]) == 2
    assert dp["distinct_devices"] == 1 and {d["rank"] for d in dp["rank_devices"]} == {0, 1}     # the rehearsal shares the one GPU, and says so
    assert "extras" not in out and "cpu_baseline" not in out     # rank 0 at N = 1 only
    assert r.stdout.count('"metric"') == 1                        # ONE line, from rank 0


def test_bench_refuses_more_ranks_than_devices():
    """``--gpus`` beyond the visible devices (RCCL transport) is an error line and a non-zero exit, never an n_gpus-1 record."""
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "VOICEMAP_DIST_BACKEND")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    out = _last_json_line(r.stdout)
    assert out["value"] is None and "device" in out["error"]


def test_bench_two_ranks_over_rccl_on_one_device_end_loudly():
    """VERDICT r5 next #7a: the RCCL transport itself with two ranks on the ONE device of the test box (VOICEMAP_DIST_SHARE_DEVICE).
    RCCL refuses a communicator with two ranks on one GPU: what must happen then is an error (a non-zero exit with the transport's or
    the watchdog's message) inside the watchdog's limit -- never a hang.  If a future RCCL accepts the sharing, the line must be a
    complete N = 2 line over "nccl"."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VOICEMAP_DIST_SHARE_DEVICE="1", VOICEMAP_DIST_WATCHDOG_S="45")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "VOICEMAP_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--blocks", "1", "--pairs", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    log = os.path.join(ROOT, "gpurun_out", "rccl_two_ranks_one_device.log")
    try:
        os.makedirs(os.path.dirname(log), exist_ok=True)
        with open(log, "w") as f:
            f.write("rc=%d\n--- stdout\n%s\n--- stderr (tail)\n%s\n" % (r.returncode, r.stdout[-4000:], r.stderr[-6000:]))
    except OSError:
        pass
    if r.returncode == 0:
        out = _last_json_line(r.stdout)
        assert out["n_gpus"] == 2 and out["data_parallel"]["backend"] == "nccl" and out["data_parallel"]["replicas_bit_identical_after_timed_steps"]
    else:
        text = (r.stdout + r.stderr).lower()
        # the refusal must be RCCL's own (reached through init_process_group("nccl") and the first barrier) or the watchdog's
        assert "duplicate gpu" in text or "watchdog: no progress" in text, r.stderr[-3000:]


def test_rccl_one_rank_runs_the_data_parallel_step():
    """RCCL itself under the production data-parallel step, on the one GPU a test box has: a one-rank "nccl" process group with the
    gradient hook forced on (tools/probe/rccl_one_rank.py).  The early all-reduce rides the side stream behind the weight-gradient GEMMs,
    the late one sits in the optimizer hook, replayed steps issue both from their host-call slots -- and a sum over one rank being the
    identity, parameters, Adam slots and gradients must equal an un-hooked engine's bit for bit."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join("tools", "probe", "rccl_one_rank.py"), "small", "8", "7"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = _last_json_line(r.stdout)
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["same_bits"] and out["finite"]
    assert out["collectives_per_step"] == 2 and out["replayed_programs"] >= 1
