"""bench.py's plain run and --dump-outputs: the files hold the frame the last
timed step left in the caller's buffers (float32, under the size budget, a
fixed pixel sample when the frame is larger), and a plain run reports the
headline figures only, leaving everything else to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _rgba(c):
    return np.stack([(c >> s) & 0xFF for s in (0, 8, 16, 24)], axis=-1).astype(np.float32)


def _caller_t(got):
    """t as the caller's buffer holds it: +inf where nothing was hit."""
    return np.where(got["hit"] == 1, got["t"], np.float32(np.inf))


def _frame(h, w, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    t = rng.random((h, w), dtype=np.float32)
    t[rng.random((h, w)) < 0.5] = np.inf
    return c, t


def _dump(tmp_path, c, t):
    bench.dump_outputs(str(tmp_path), torch.from_numpy(c.view(np.int32)), torch.from_numpy(t))
    return {n[:-4]: np.load(tmp_path / n) for n in sorted(os.listdir(tmp_path))}


def test_dump_whole_frame(tmp_path):
    c, t = _frame(7, 13, 1)
    got = _dump(tmp_path, c, t)
    assert sorted(got) == ["color", "hit", "t"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["color"], _rgba(c)) and np.array_equal(got["hit"], np.isfinite(t))
    assert (~np.isfinite(t)).any() and np.array_equal(_caller_t(got), t)


def test_dump_samples_a_frame_over_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    c, t = _frame(31, 17, 2)  # 527 pixels x 24 B > 4000 B
    a = _dump(tmp_path / "a", c, t)
    b = _dump(tmp_path / "b", c, t)
    assert sorted(a) == ["color", "hit", "pixel_index", "t"]
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and np.array_equal(idx, b["pixel_index"])  # the same pixels every run
    ii = idx.astype(np.int64)
    assert 0 < len(ii) < c.size and np.all(np.diff(ii) > 0) and ii[0] >= 0 and ii[-1] < c.size
    assert np.array_equal(a["color"], _rgba(c.reshape(-1)[ii])) and np.array_equal(_caller_t(a), t.reshape(-1)[ii])
    assert all(np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 4000
    # a whole-frame dump into the same directory leaves no stale index behind
    monkeypatch.setattr(bench, "DUMP_BYTES", 60_000_000)
    assert sorted(_dump(tmp_path / "a", c, t)) == ["color", "hit", "t"]


@pytest.mark.parametrize("w,h", sorted({(w, h) for _, w, h, *_ in bench.WORKLOADS.values()}))
def test_real_frames_fit_the_budget(tmp_path, w, h):
    """Every frame size the workloads use: the files on disk, headers included, stay under 64 MB."""
    bench.dump_outputs(str(tmp_path), torch.zeros((h, w), dtype=torch.int32), torch.zeros((h, w)))
    names = sorted(os.listdir(tmp_path))
    assert names == (["color.npy", "hit.npy", "t.npy"] if w * h <= 1920 * 1080 else
                     ["color.npy", "hit.npy", "pixel_index.npy", "t.npy"])
    assert sum(os.path.getsize(tmp_path / n) for n in names) <= 64_000_000


def test_inputs_unpack_elsewhere_when_the_tree_is_read_only(rt, tmp_path, monkeypatch):
    """A checkout whose data/_unpacked was never filled and cannot be written:
    the benchmark unpacks into a private directory and names it to its child
    processes; one that build() filled, or that can be written, is used as it is."""
    data = rt.data
    tree = tmp_path / "tree" / "_unpacked"
    (tmp_path / "tree").mkdir()
    monkeypatch.setattr(data, "UNPACKED", str(tree))
    monkeypatch.delenv("RTAMD_DATA_DIR", raising=False)
    monkeypatch.setattr("tempfile.tempdir", str(tmp_path / "tmp"))
    (tmp_path / "tmp").mkdir()
    bench.use_writable_data_dir()
    assert data.UNPACKED == str(tree) and "RTAMD_DATA_DIR" not in os.environ  # writable: left alone
    real_access = os.access
    monkeypatch.setattr(os, "access", lambda p, m: False if str(p).startswith(str(tmp_path / "tree")) else
                        real_access(p, m))
    bench.use_writable_data_dir()
    priv = data.UNPACKED
    assert os.path.dirname(priv) == str(tmp_path / "tmp") and os.environ["RTAMD_DATA_DIR"] == priv
    assert os.stat(priv).st_mode & 0o777 == 0o700
    p = data.path("cube.obj")
    assert os.path.dirname(p) == priv and os.path.getsize(p) > 0 and not tree.exists()
    # a process started by that one takes the directory from the environment: the package
    # reads it at import, and the benchmark assigns it as well
    code = "import sys; sys.path.insert(0, sys.argv[1]); from rtamd import data; print(data.UNPACKED)"
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(os.path.dirname(rt.__file__))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == priv, r.stderr[-500:]
    monkeypatch.setattr(data, "UNPACKED", str(tree))
    bench.use_writable_data_dir()
    assert data.UNPACKED == priv
    # a tree that holds every input is used even when it cannot be written
    monkeypatch.delenv("RTAMD_DATA_DIR")
    monkeypatch.setattr(data, "UNPACKED", str(tree))
    tree.mkdir()
    for f in data.FILES:
        (tree / f).write_bytes(b"x")
    bench.use_writable_data_dir()
    assert data.UNPACKED == str(tree) and "RTAMD_DATA_DIR" not in os.environ


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_frame(gpu, tmp_path):
    steps, warmup = 3, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    _, W, H, *_ = bench.WORKLOADS["bunny"]
    assert d["metric"] == bench.METRIC and d["unit"] == "Mrays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same wall time (ms_per_step is rounded to 1e-4 ms)
    assert d["value"] == pytest.approx(W * H / (d["ms_per_step"] * 1e3), rel=0.5e-4 / d["ms_per_step"] + 1e-3)
    for k in ("roofline", "extra", "cpu_baseline", "drop_in", "frame_latency", "frame_check", "detail_file"):
        assert k not in d, k  # --full's
    # the dump is the last timed frame: orbit frame warmup + steps - 1, rendered here on its own
    scene, _ = gpu.workloads.scene_for("stanford-bunny.obj")
    try:
        scene.set_plane(None)
        c = np.zeros((H, W), np.uint32)
        t = np.full((H, W), np.inf, np.float32)
        scene.render(bench.orbit_params(warmup + steps, W, H)[-1], c, t, clear=True)
    finally:
        scene.close()
    assert sorted(os.listdir(tmp_path / "o")) == ["color.npy", "hit.npy", "t.npy"]
    got = {n: np.load(tmp_path / "o" / f"{n}.npy") for n in ("color", "hit", "t")}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["color"], _rgba(c)) and np.array_equal(_caller_t(got), t)
    assert 0 < got["hit"].mean() < 1  # the bunny covers part of the frame
