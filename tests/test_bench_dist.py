"""bench.py's multi-process path (rendezvous, barrier, max-over-ranks timing, aggregated value) without GPUs: two ranks under
torch.distributed.run with the gloo backend, the kernels running in the CPU emulator build (ORBX_BENCH_LIB).  The numbers mean nothing; the
protocol is what is tested: one JSON line from rank 0, n_gpus = 2, value = units of BOTH ranks / the slowest rank's time."""
import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.environ.get("ORBX_EMU_LIB") or os.path.join(ROOT, "tests", "emu", "liborbx_emu.so")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_bench_two_ranks_gloo(emu_lib):
    env = dict(os.environ)
    env.update(ORBX_BENCH_BACKEND="gloo", ORBX_BENCH_LIB=EMU_SO, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "1", "--handles", "1", "--full", "--no-cpu-baseline", "--min-seconds", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0): %r" % r.stdout[-1000:]
    assert r.stdout.strip().splitlines()[-1].startswith("{"), "the JSON line is the last line of stdout: %r" % r.stdout[-500:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["warmup"] == 1 and res["scaling"] == "weak" and res["unit"] == "stereo pairs/s"
    # whole-job aggregate: 2 ranks x 1 pair x 2 steps over the (max over ranks) time
    assert abs(res["value"] - 2 * 1 * 2 / (res["ms_per_step"] * 2 * 1e-3)) < 0.06            # (value is rounded to 0.1)
    assert res["roofline"]["kernel"] in res["stage_ms_alone"] and res["roofline"]["avg_launch_ms"] > 0
    assert "cpu_baseline" not in res and "h2d_inclusive" not in res          # rank-0 / N = 1 extras only
    assert res["config"]["parallelism"].startswith("independent streams, 2 GPU")
    pr = res["per_rank"]                                                     # every rank's own rate: a straggler is visible in the line
    assert len(pr["values"]) == 2 and pr["min"] == min(pr["values"]) and pr["max"] == max(pr["values"]) and abs(2 * pr["min"] - res["value"]) < 0.2


def test_bench_launches_its_own_ranks(emu_lib):
    """`python bench.py --gpus 2` WITHOUT a launcher must start two ranks itself (round-2 review: the flag was parsed and ignored), print
    n_gpus = 2, say which library produced the line, and with --allgather carry the collective's own time (BASELINE.json configs[4])."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(ORBX_BENCH_BACKEND="gloo", ORBX_BENCH_LIB=EMU_SO, OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "1", "--handles", "1", "--full", "--no-cpu-baseline",
           "--allgather", "--min-seconds", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0): %r" % r.stdout[-1000:]
    assert r.stdout.strip().splitlines()[-1].startswith("{"), "the JSON line is the last line of stdout: %r" % r.stdout[-500:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["repeats"] == 1 and res["timed_steps"] == 2
    assert res["config"]["library"].startswith("liborbx_emu.so") and "override" in res["config"]["library"]
    ag = res["allgather"]
    assert ag["backend"] == "gloo" and ag["ms_per_batch_alone"] > 0 and ag["bytes_gathered_per_rank"] == 2 * ag["bytes_per_rank"]
    assert "all-gather" in res["config"]["parallelism"] and 0.0 < res["config"]["fast_corner_density_t7"] < 1.0


def test_bench_refuses_more_ranks_than_gpus():
    """with the RCCL backend one process per GPU is the rule: asking for more GPUs than the node shows is an error, not a silent 1-GPU run"""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "ORBX_BENCH_BACKEND"):
        env.pop(k, None)
    import torch
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(max(n, 2))], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "one process per GPU" in r.stderr and not any(l.startswith("{") for l in r.stdout.splitlines())


import pytest


@pytest.mark.gpu
def test_bench_two_ranks_share_one_gpu(hip_lib):
    """Pre-flight of the multi-GPU run on a 1-GPU box: `bench.py --gpus 2` with the HIP library, two processes on GPU 0,
    rendezvous / barriers / max over ranks over gloo (RCCL refuses two ranks on one device).  The ranks share the GPU, so the whole-job value is about
    the 1-rank rate, not twice it; what is checked is the protocol with the real library and that no rank starves."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ORBX_BENCH_LIB"):
        env.pop(k, None)
    env.update(ORBX_BENCH_BACKEND="gloo")
    common = ["--steps", "20", "--warmup", "5", "--pairs", "64", "--handles", "2", "--full", "--no-cpu-baseline", "--no-h2d", "--no-other-configs", "--no-latency", "--min-seconds", "1"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-4000:]
    r1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + common, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-4000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r2 = json.loads(lines[0])
    assert r2["n_gpus"] == 2 and r2["config"]["library"] == "liborbx_hip.so" and r2["parity_check"]["identical"] is True
    assert 0.6 * r1["value"] < r2["value"] < 1.5 * r1["value"], (r1["value"], r2["value"])             # one GPU's worth of work, shared
    pr = r2["per_rank"]
    assert len(pr["values"]) == 2 and pr["min"] > 0.25 * r1["value"], pr                                # nobody starves


@pytest.mark.gpu
def test_bench_four_ranks_share_one_gpu_in_16_cores(hip_lib):
    """Pre-flight of the driver's multi-GPU scaling run under its real host constraints: `bench.py --gpus 4` with the HIP library -
    four processes x four handles on GPU 0, confined to 16 cores (what the GPU boxes grant), rendezvous / barriers / max over ranks over gloo - with and
    without the descriptor all-gather.  The ranks share one GPU, so the whole-job value is about one GPU's; checked: the protocol, parity, no rank starves,
    the host side of the ranks fits the cores, and the whole command stays far inside the driver's 1 800 s.  Four ranks, not eight: the GPU machines the
    suite runs on admit six processes with the device open, and this process holds it too (world size 8: test_bench_eight_ranks_gloo)."""
    import time
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ORBX_BENCH_LIB"):
        env.pop(k, None)
    env.update(ORBX_BENCH_BACKEND="gloo", OMP_NUM_THREADS="1")
    cpus = sorted(os.sched_getaffinity(0))[:16]
    out = {}
    for name, extra in (("plain", []), ("allgather", ["--allgather"])):
        cmd = ["taskset", "-c", ",".join(str(c) for c in cpus), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "20", "--warmup", "5", "--pairs", "32",
               "--full", "--no-cpu-baseline", "--no-h2d", "--no-other-configs", "--no-latency", "--min-seconds", "2"] + extra
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=1500)
        wall = time.time() - t0
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        res = json.loads(lines[0]); out[name] = res
        assert res["n_gpus"] == 4 and res["config"]["library"] == "liborbx_hip.so" and res["parity_check"]["identical"] is True
        pr = res["per_rank"]
        assert len(pr["values"]) == 4 and pr["min"] > 0.5 * pr["max"], pr                               # nobody starves
        hc = res["host_cpu"]
        assert len(hc["cpu_ms_per_step_per_rank"]) == 4 and hc["cpu_cores_busy_all_ranks"] < len(cpus), hc
        assert wall < 600, wall
    assert out["allgather"]["allgather"]["backend"] == "gloo" and out["allgather"]["allgather"]["ms_per_batch_alone"] > 0


def test_bench_eight_ranks_gloo(emu_lib):
    """The driver's world size without GPUs: `bench.py --gpus 8 --allgather --full` launching its own ranks, gloo, the kernels in the CPU emulator build -
    one JSON line, eight per-rank rates and host figures, value = units of all ranks / the slowest rank's time, the all-gather over eight ranks, parity."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(ORBX_BENCH_BACKEND="gloo", ORBX_BENCH_LIB=EMU_SO, OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--pairs", "1", "--handles", "1", "--full", "--no-cpu-baseline",
           "--allgather"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["timed_steps"] == 2 and res["parity_check"]["identical"] is True
    assert abs(res["value"] - 8 * 1 * 2 / (res["ms_per_step"] * 2 * 1e-3)) < 0.06
    pr = res["per_rank"]
    assert len(pr["values"]) == 8 and pr["min"] == min(pr["values"]) and pr["max"] == max(pr["values"]) and abs(8 * pr["min"] - res["value"]) < 0.5
    assert len(res["host_cpu"]["cpu_ms_per_step_per_rank"]) == 8
    ag = res["allgather"]
    assert ag["backend"] == "gloo" and ag["ms_per_batch_alone"] > 0 and ag["bytes_gathered_per_rank"] == 8 * ag["bytes_per_rank"]

def test_bench_plain_run_times_its_steps_and_dumps_outputs(emu_lib, tmp_path):
    """Without --full a run times exactly --steps steps and carries the headline figures only; --dump-outputs writes what the last timed step
    computed as float32 .npy files, the same from run to run, and those are what a direct extraction of the same seeded input gives."""
    from orb_slam3_detailed_comments_amd import ORBextractor, synth
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ORBX_BENCH_BACKEND"):
        env.pop(k, None)
    env.update(ORBX_BENCH_LIB=EMU_SO, OMP_NUM_THREADS="1")
    dumps = []
    for run in range(2):
        d = tmp_path / str(run)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "1", "--handles", "2", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0]
        res = json.loads(lines[0])
        assert res["steps"] == 3 and res["timed_steps"] == 3 and res["repeats"] == 1 and res["step_ms"]["n"] == 3
        assert abs(res["ms_per_step"] * 3 - res["timed_seconds"] * 1e3) < 0.2                   # (timed_seconds is rounded to 0.1 ms)
        assert res["higher_is_better"] is True and res["dtype"] == "u8" and res["unit"] == "stereo pairs/s" and res["value"] > 0
        assert not any(k in res for k in ("roofline", "stage_ms_alone", "h2d_inclusive", "latency", "other_configs", "cpu_baseline")) and res["parity_check"] is None
        arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d) if f != ".gitignore"}
        assert sorted((d / ".gitignore").read_text().split("\n")[1:-1]) == sorted([".gitignore"] + [k + ".npy" for k in arrays])
        assert all(a.dtype == np.float32 for a in arrays.values()) and sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert {"keypoints", "descriptors", "keypoint_counts", "u_right", "depth", "stereo_matches", "units"} <= set(arrays)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys() and all(dumps[0][k].tobytes() == dumps[1][k].tobytes() for k in dumps[0])
    a = dumps[0]
    L, R = synth.stereo_pair(752, 480, seed=0)                    # bench.py's first pair of rank 0
    got = ORBextractor(1200, 1.2, 8, 20, 7, lib=emu_lib).extract_batch(np.stack([L, R]))
    for side in range(2):
        kps, desc = got[side][1], got[side][2]
        n = len(kps)
        assert a["keypoint_counts"][0, side] == n and a["keypoints"].shape[:2] == (1, 2)
        assert np.array_equal(a["descriptors"][0, side, :n], desc.astype(np.float32)) and not a["descriptors"][0, side, n:].any()
        assert np.array_equal(a["keypoints"][0, side, :n, 0], kps["x"]) and np.array_equal(a["keypoints"][0, side, :n, 5], kps["octave"].astype(np.float32))


def _fake_outputs(kind, P, cap, rng):
    """output buffers as bench.py's fetch fills them, random where the library would write"""
    from orb_slam3_detailed_comments_amd import KP_DTYPE
    nimg = 2 * P if kind in ("stereo", "fisheye") else P
    return dict(k=rng.integers(0, 256, (nimg, cap, KP_DTYPE.itemsize), dtype=np.uint8), d=rng.integers(0, 256, (nimg, cap, 32), dtype=np.uint8),
                n=rng.integers(0, cap, nimg).astype(np.int32), m=rng.integers(0, cap, nimg).astype(np.int32), u=rng.normal(size=(P, cap)).astype(np.float32),
                z=rng.normal(size=(P, cap)).astype(np.float32), nm=rng.integers(0, cap, P).astype(np.int32), l2r=rng.integers(-1, cap, (P, cap)).astype(np.int32),
                r2l=rng.integers(-1, cap, (P, cap)).astype(np.int32), p3=rng.normal(size=(P, cap, 3)).astype(np.float32),
                lp_asg=rng.integers(-1, 5000, (P, cap)).astype(np.int32), lp_nm=rng.integers(0, cap, P).astype(np.int32))


def _npy(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


@pytest.mark.parametrize("kind", ["stereo", "mono", "fisheye", "rgbd"])
def test_bench_dump_samples_units_beyond_the_limit(kind, tmp_path, monkeypatch):
    """Every configuration's dump: one array per output, unit first, entries past an image's keypoint count zeroed.  Outputs larger than the limit
    (.npy headers included): a fixed sample of whole units is written (the same one every time), units.npy names them, and the files fit the limit."""
    import bench
    P, cap = 10, 40
    o = _fake_outputs(kind, P, cap, np.random.default_rng(5))
    full = tmp_path / "full"
    bench.dump_outputs(str(full), kind, P, o)
    a = _npy(full)
    names = {"keypoints", "descriptors", "keypoint_counts", "monocular_counts", "units"} | {
        "stereo": {"u_right", "depth", "stereo_matches"}, "mono": set(), "fisheye": {"left_to_right", "right_to_left", "depth", "points3d", "stereo_matches"},
        "rgbd": {"u_right", "depth", "local_point_assignments", "local_point_matches"}}[kind]
    assert set(a) == names and all(v.dtype == np.float32 and len(v) == P for v in a.values())
    paired = kind in ("stereo", "fisheye")
    for p in range(P):
        for side in range(2 if paired else 1):
            n = o["n"][side * P + p]
            kp, ds = (a["keypoints"][p, side], a["descriptors"][p, side]) if paired else (a["keypoints"][p], a["descriptors"][p])
            assert not kp[n:].any() and not ds[n:].any() and np.array_equal(ds[:n], o["d"][side * P + p, :n].astype(np.float32))
        for k in ("depth", "u_right", "left_to_right", "local_point_assignments"):
            if k in a:
                assert not a[k][p, o["n"][p]:].any()
    per_unit = sum(v[0].nbytes for v in a.values())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * per_unit + 4096 * len(a))
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), kind, P, o)
    units = np.load(tmp_path / "a" / "units.npy")
    assert len(units) == 4 and np.all(np.diff(units) > 0) and np.array_equal(units, np.load(tmp_path / "b" / "units.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a") if f.endswith(".npy")) <= bench.DUMP_LIMIT_BYTES
    for k, v in _npy(tmp_path / "a").items():
        assert v.tobytes() == a[k][units.astype(int)].tobytes(), k


@pytest.mark.parametrize("config", ["mono", "fisheye", "rgbd"])
def test_bench_dump_other_configs(config, emu_lib, tmp_path):
    """--dump-outputs on the other configurations' real output buffers (emulator build, one unit per step): the run succeeds and every output is
    written, unit first."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ORBX_BENCH_BACKEND"):
        env.pop(k, None)
    env.update(ORBX_BENCH_LIB=EMU_SO, OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "2", "--warmup", "1", "--pairs", "1", "--handles", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    a = _npy(tmp_path)
    want = {"mono": {"keypoints"}, "fisheye": {"left_to_right", "right_to_left", "points3d"}, "rgbd": {"u_right", "local_point_assignments"}}[config]
    assert want <= set(a) and all(v.dtype == np.float32 and len(v) == 1 for v in a.values())
    assert a["keypoint_counts"].min() > 0
