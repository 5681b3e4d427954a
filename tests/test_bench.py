"""bench.py's command line: what a plain run prints, what --dump-outputs
writes and what --full adds."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_KEYS = {"verified", "roofline", "single_frame", "stages", "configs2_4k", "configs4_8192",
             "cpu_baseline"}


def _bench():
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    return bench


def test_dump_outputs_files(tmp_path, monkeypatch):
    """dump_outputs: one float32 file per frame holding the JPEG's bytes (a
    fixed sorted sample of positions when the string is over the frame's
    share of the budget), the lengths and the iteration counts as float64."""
    bench = _bench()
    rng = np.random.default_rng(5)
    jpegs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 1000, 64)]
    stats = [types.SimpleNamespace(iterations=i) for i in (22, 27, 3)]
    # 3 frames, 4 bytes per element -> a share of 256 elements per frame
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4 * 256)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b" / "nested")]
    for d in dirs:
        bench.dump_outputs(d, jpegs, stats, 0, 1)
    assert sorted(os.listdir(dirs[0])) == ["iterations.npy", "jpeg_0.npy", "jpeg_1.npy",
                                           "jpeg_2.npy", "jpeg_bytes.npy"]
    total = 0
    for name in os.listdir(dirs[0]):
        a = np.load(os.path.join(dirs[0], name))
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(os.path.join(dirs[1], name)))  # same sample every time
        total += a.nbytes
    assert total <= 3 * 4 * 256 + 2 * 3 * 8
    assert np.array_equal(np.load(os.path.join(dirs[0], "jpeg_bytes.npy")), [300, 1000, 64])
    assert np.array_equal(np.load(os.path.join(dirs[0], "iterations.npy")), [22, 27, 3])
    whole = np.load(os.path.join(dirs[0], "jpeg_2.npy"))
    assert whole.dtype == np.float32 and np.array_equal(whole, np.frombuffer(jpegs[2], np.uint8))
    for f in (0, 1):
        part = np.load(os.path.join(dirs[0], "jpeg_%d.npy" % f))
        src = np.frombuffer(jpegs[f], np.uint8)
        assert part.shape == (256,)
        idx = np.sort(np.random.default_rng(f).choice(src.size, 256, replace=False))
        assert np.array_equal(part, src[idx])
    # a second rank's files stand beside rank 0's
    bench.dump_outputs(dirs[0], jpegs[:1], stats[:1], 1, 2)
    assert os.path.exists(os.path.join(dirs[0], "jpeg_0_rank1.npy"))


def _run_bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_full_run_adds_the_side_legs():
    """--full (small frames; the 4K, 8192x8192 and CPU legs switched off by
    their own options) adds the known-answer check and the isolated frame."""
    line = _run_bench("--steps", "1", "--warmup", "0", "--width", "96", "--height", "80",
                      "--frames-per-step", "1", "--full", "--no-uhd-frame", "--no-large-frame",
                      "--no-cpu-baseline")
    assert PLAIN_KEYS <= set(line)
    assert {"verified", "roofline", "single_frame", "stages"} <= set(line), sorted(line)
    assert line["verified"]["frames"] == line["verified"]["bit_exact"]
    assert line["single_frame"]["iterations"] == line["config"]["search_iterations"][0]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gz, tmp_path):
    """A plain run (small frames, 2 timed steps after 1 warm-up) prints the
    headline keys and none of --full's legs, and --dump-outputs holds the
    last timed step's JPEG bytes: those of gz.process on the same frames."""
    w, h, q, n = 96, 80, 95, 2
    out_dir = str(tmp_path / "dump")
    line = _run_bench("--steps", "2", "--warmup", "1", "--width", str(w), "--height", str(h),
                      "--quality", str(q), "--frames-per-step", str(n), "--dump-outputs", out_dir)
    assert PLAIN_KEYS <= set(line) and not FULL_KEYS & set(line), sorted(line)
    assert (line["steps"], line["warmup"]) == (2, 1)
    assert len(line["config"]["search_iterations"]) == 2 * n  # --steps timed steps, no more
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - n * w * h / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * line["value"]
    params = gz.Params.for_quality(q)
    sizes = np.load(os.path.join(out_dir, "jpeg_bytes.npy"))
    iters = np.load(os.path.join(out_dir, "iterations.npy"))
    assert sizes.dtype == np.float64 and iters.dtype == np.float64
    for f in range(n):
        # the last of the 3 steps (index 2) encodes seeds 1000 + 2 * 100 + f on rank 0
        data, st = gz.process(gz.synthetic_frame(1200 + f, w, h), w, h, params, return_stats=True)
        got = np.load(os.path.join(out_dir, "jpeg_%d.npy" % f))
        assert got.dtype == np.float32
        assert np.array_equal(got, np.frombuffer(data, np.uint8))
        assert sizes[f] == len(data) and iters[f] == st.iterations
