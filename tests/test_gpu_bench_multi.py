"""`bench.py --gpus 2` through its three partitionings, launched the way the driver launches it (torch.distributed.run,
one process per rank) but with both ranks on this one GPU over gloo (MKB_BENCH_ONE_DEVICE=1): a functional check of the
N > 1 entry path -- rank bookkeeping, the cross-rank consistency probe, the JSON line -- not a scaling number."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("parallelism,scaling", [("dims", "weak"), ("rows", "weak"), ("table-rows", "weak"), ("rows", "strong"),
                                                 ("table-rows", "strong")])
def test_bench_two_ranks_on_one_device(parallelism, scaling):
    from conftest import ROOT

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MKB_BENCH_ONE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--config", "wn18rr-rotate", "--parallelism", parallelism, "--scaling", scaling, "--no-extras"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0 and d["unit"] == "triples/s" and d["scaling"] == scaling
    assert d["config"]["global_batch"] == (2048 if scaling == "weak" else 1024)
    want = {"dims": "dims2", "rows": "dp2", "table-rows": "table-rows2"}[parallelism]
    assert d["config"]["parallelism"].startswith(want), d["config"]["parallelism"]


def test_bench_default_partitioning_is_table_rows_and_reports_the_others():
    """No --parallelism: the north_star partitioning is the line's value; with --full, dims and rows ride in the same line
    under other_partitionings."""
    from conftest import ROOT

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MKB_BENCH_ONE_DEVICE="1")
    env.pop("MKB_BENCH_PARALLELISM", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--config", "wn18rr-rotate", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["parallelism"].startswith("table-rows2") and "partitioning_failures" not in d
    assert set(d["other_partitionings"]) == {"dims", "rows"} and all(v["value"] > 0 for v in d["other_partitionings"].values())
    assert "extras_error" not in d, d["extras_error"]
    # ... and the other way round: another partitioning as the line's value, the row-sharded step among the extras (measured
    # without the kernel-class probe: its timed batches must follow the warm-up batches without a gap -- the step plans the next
    # batch's routes, a skipped batch is an error there; round 4 found the extras ending in exactly that error)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--config", "wn18rr-rotate", "--parallelism", "dims", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["parallelism"].startswith("dims2") and "extras_error" not in d, d.get("extras_error")
    assert set(d["other_partitionings"]) == {"table-rows", "rows"} and all(v["value"] > 0 for v in d["other_partitionings"].values())


def test_bench_table_rows_code_path_on_one_rank():
    """--force-parallelism: the row-sharded step at world 1 (no collective): what one rank computes per step."""
    from conftest import ROOT

    cmd = [sys.executable, str(ROOT / "bench.py"), "--steps", "4", "--warmup", "2", "--config", "yago310-rotate", "--parallelism",
           "table-rows", "--force-parallelism", "--no-traffic"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["parallelism"].startswith("table-rows1") and d["value"] > 0


@pytest.mark.parametrize("timeout", [None, "0.2"])
def test_bench_safety_line_of_the_row_sharded_step(timeout):
    """N > 1: a short measurement with the collectives in torch.distributed runs in front of the library-issued form and rides
    the line (``torch_distributed_form``); a watchdog prints it as the line when the main measurement does not finish in time
    (forced here with a timeout no measurement can meet).  One device, gloo: MKB_BENCH_FORCE_SAFETY=1 switches the path on."""
    from conftest import ROOT

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MKB_BENCH_ONE_DEVICE="1", MKB_BENCH_FORCE_SAFETY="1")
    env.pop("MKB_BENCH_PARALLELISM", None)
    if timeout:
        env["MKB_BENCH_MAIN_TIMEOUT"] = timeout
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "60" if timeout else "4", "--warmup", "2",
           "--config", "wn18rr-rotate", "--no-extras"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["parallelism"].startswith("table-rows2")
    if timeout:
        assert "did not finish in time" in d["error"] and d["steps"] == 40
    else:
        assert "error" not in d and d["torch_distributed_form"]["value"] > 0 and d["steps"] == 4


def test_bench_line_reports_the_median_window_and_every_window():
    """The timed region is the --steps steps split into R back-to-back windows; ms_per_step / value are the MEDIAN window (an
    actual window: the lower median for an even count) and nothing is dropped: every window is listed with its instruments."""
    from conftest import ROOT

    cmd = [sys.executable, str(ROOT / "bench.py"), "--steps", "36", "--warmup", "2", "--windows", "6", "--config", "wn18rr-rotate", "--no-traffic"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 36 and d["warmup"] == 2 and d["windows"] == 6 and len(d["windows_ms"]) == 6 == len(d["windows_detail"])
    assert d["windows_steps"] == [6] * 6 and all(w["steps"] == 6 for w in d["windows_detail"])  # the 36 timed steps, no more
    per_step = sorted(w / 6 for w in d["windows_ms"])
    assert abs(d["ms_per_step"] - per_step[2]) < 1e-6 * per_step[2] + 1e-5, (d["ms_per_step"], per_step)  # lower median of six
    assert abs(d["value"] - 1024 * 129 / (d["ms_per_step"] / 1e3)) < 1e-3 * d["value"]                   # B * (K + 1) per step
    for w in d["windows_detail"]:
        assert {"ms", "host_enqueue_ms", "device_ms", "largest_submit_gap_ms", "largest_submit_gap_at_step", "gc_ms"} <= set(w)
        assert 0 < w["host_enqueue_ms"] <= w["ms"] + 1e-3 and 0 < w["device_ms"] <= w["ms"] + 0.5
    assert d["t_host_ms_per_step"] > 0 and isinstance(d["gc_collections_during_windows"], list)


def test_bench_plain_run_leaves_the_extras_to_full():
    """A plain headline run prints the line and its in-region roofline only; --full adds the measurements the value does not
    need (here the step variants: the others have their own --no-* switches, and take a rocprofv3 pass, training or the CPU)."""
    from conftest import ROOT

    extras = {"mrr", "step_variants", "cpu_baseline"}
    lines = {}
    for name, flags in (("plain", []), ("full", ["--full", "--no-traffic", "--mrr-epochs", "0", "--no-cpu-baseline"])):
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", *flags]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        lines[name] = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert plain["steps"] == 4 and plain["value"] > 0 and not extras & set(plain)
    assert plain["roofline"]["launches"] > 0 and plain["roofline"]["traffic"] is None
    assert set(full) & extras == {"step_variants"} and all(v["value"] > 0 for v in full["step_variants"].values())


def test_bench_dump_outputs_of_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float32 / float64 .npy files, 64 MB at most, the same inputs on every
    run with the same arguments -- two runs draw the same negatives and end on the same tables."""
    import numpy as np

    from conftest import ROOT

    dumps = []
    for run in ("a", "b"):
        d_out = tmp_path / run
        cmd = [sys.executable, str(ROOT / "bench.py"), "--steps", "7", "--warmup", "2", "--config", "wn18rr-rotate", "--no-traffic",
               "--dump-outputs", str(d_out)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 7 and sum(d["windows_steps"]) == 7 and d["dump_outputs"]["dir"] == str(d_out)
        arrays = {p.stem: np.load(p) for p in d_out.glob("*.npy")}
        assert set(arrays) == set(d["dump_outputs"]["arrays"]) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["loss"].item() == np.float32(d["loss"])
        assert arrays["negative_score"].shape == (1024, 128) and arrays["negative_sample"].shape == (1024, 128)
        assert arrays["entity_embedding"].shape == (len(arrays["entity_embedding_rows"]), 1000)  # a row sample of the 40,943 rows
        dumps.append(arrays)
    a, b = dumps
    assert set(a) == set(b)
    for name in ("negative_sample", "entity_embedding_rows"):
        assert np.array_equal(a[name], b[name]), name
    for name in set(a) - {"negative_sample", "entity_embedding_rows"}:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-5, atol=1e-6, err_msg=name)
