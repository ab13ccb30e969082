"""bench.py's command line: a plain run times exactly --steps steps in one block, --full adds the other measurements and
checks, --dump-outputs writes the frame of the last timed step as float32 / float64 .npy files.  CPU: the argument defaults
and the dump format; GPU: a plain run of C1 dumps the oracle's committed image (tests/golden/c1_oracle.json), and --full
still reports what it did before it was an option."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (imports neither torch nor the native libraries at module level)

FULL_ONLY = ("timed_frames_verified", "paths_per_s_latency", "fine_mpixels_per_s", "one_frame_at_a_time", "stage_ms",
             "stage_roofline", "roofline", "cpu_baseline")


def test_plain_run_times_exactly_steps_and_full_keeps_the_block_protocol():
    a = bench.parse_args(["--steps", "17", "--warmup", "2"])
    assert (a.steps, a.warmup, a.blocks, a.min_seconds, a.full, a.dump_outputs) == (17, 2, 1, 0.0, False, None)
    a = bench.parse_args(["--full"])
    assert (a.blocks, a.min_seconds, a.full) == (5, 1.0, True)
    a = bench.parse_args(["--full", "--blocks", "2", "--min-seconds", "0", "--dump-outputs", "d"])
    assert (a.blocks, a.min_seconds, a.dump_outputs) == (2, 0.0, "d")


def _random_image(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, 4), dtype=np.float32).astype(np.float16)


def test_dump_outputs_small_image_is_written_whole(tmp_path):
    img = _random_image(64, 48, 1)
    bump = np.array([0, 5, 0, 373, 194, 194, 0, 70], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path), img, bump)
    assert sorted(os.listdir(tmp_path)) == ["bump.npy", "image.npy", "image_row_sum.npy"]
    got = np.load(tmp_path / "image.npy")
    assert got.dtype == np.float32 and got.shape == (64, 48, 4)
    assert np.array_equal(got.astype(np.float16).view(np.uint16), img.view(np.uint16))
    b = np.load(tmp_path / "bump.npy")
    assert b.dtype == np.float64 and b.tolist() == bump.tolist()
    rs = np.load(tmp_path / "image_row_sum.npy")
    assert rs.dtype == np.float64 and rs.shape == (64, 4)
    assert np.allclose(rs, img.astype(np.float64).sum(axis=1), rtol=0, atol=1e-9)


def test_dump_outputs_large_image_is_a_fixed_sample(tmp_path):
    h, w = 1100, 1000  # more than bench.DUMP_PIXELS pixels
    assert h * w > bench.DUMP_PIXELS
    img = _random_image(h, w, 2)
    bump = np.arange(8, dtype=np.uint32)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), img, bump)
    bench.dump_outputs(str(b), _random_image(h, w, 3), bump)
    names = sorted(os.listdir(a))
    assert names == ["bump.npy", "image_row_sum.npy", "image_sample.npy", "image_sample_index.npy"]
    assert sum(os.path.getsize(a / n) for n in names) < 64 << 20
    for n in names:
        assert np.load(a / n).dtype in (np.float32, np.float64), n
    idx = np.load(a / "image_sample_index.npy")
    assert np.array_equal(idx, np.load(b / "image_sample_index.npy"))  # the sample does not depend on the pixels
    assert idx.size == bench.DUMP_PIXELS
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < h * w and np.array_equal(idx, np.floor(idx))
    sample = np.load(a / "image_sample.npy")
    assert sample.dtype == np.float32 and sample.shape == (idx.size, 4)
    assert np.array_equal(sample, img.reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    assert np.load(a / "image_row_sum.npy").shape == (h, 4)


def _run_bench(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_c1_frame_of_the_oracle(built, tmp_path):
    out = tmp_path / "out"
    j = _run_bench(["--gpus", "1", "--scene", "c1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)], 600)
    assert (j["steps"], j["warmup"], j["blocks"], len(j["block_ms_per_step"]), j["full"]) == (7, 2, 1, 1, False)
    assert j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "Mpixels/s" and j["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in j]
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "c1_oracle.json")))
    img = np.load(out / "image.npy")
    assert img.dtype == np.float32 and img.shape == (512, 512, 4)
    assert hashlib.sha256(img.astype(np.float16).view(np.uint16).tobytes()).hexdigest() == want["image"]
    assert np.load(out / "bump.npy").tolist() == want["bump"]


@pytest.mark.gpu
def test_bench_full_run_still_reports_its_extras(built):
    j = _run_bench(["--gpus", "1", "--scene", "c1", "--steps", "5", "--warmup", "1", "--full"], 600)
    assert j["full"] is True and j["steps"] == 5 and j["blocks"] >= 5
    assert all(k in j for k in FULL_ONLY)
    assert j["stage_ms"] and j["roofline"]["avg_ms"] > 0 and j["cpu_baseline"]["value"] > 0
    assert j["one_frame_at_a_time"]["ms_per_step"] > 0
