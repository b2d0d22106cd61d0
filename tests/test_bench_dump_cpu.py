"""bench.py --dump-outputs on the host: the file format, and the fixed, seeded
pixel sample a frame over the size limit is cut down to."""
import numpy as np
import torch

import bench


def frame(W, H):
    return torch.arange(W * H * 3, dtype=torch.float32) * 0.5


def test_dump_outputs_writes_the_whole_frame_as_float32(tmp_path):
    W, H = 7, 5
    bench.dump_outputs(str(tmp_path / "a" / "b"), frame(W, H), W, H)  # creates the directory
    a = np.load(tmp_path / "a" / "b" / "framebuffer.npy")
    assert a.dtype == np.float32 and a.shape == (H, W, 3)
    assert np.array_equal(a.reshape(-1), frame(W, H).numpy())


def test_dump_outputs_samples_a_frame_over_the_limit(tmp_path, monkeypatch):
    W, H = 33, 17
    monkeypatch.setattr(bench, "DUMP_MAX_FLOATS", 300)
    bench.dump_outputs(str(tmp_path / "x"), frame(W, H), W, H)
    bench.dump_outputs(str(tmp_path / "y"), frame(W, H), W, H)
    x, y = np.load(tmp_path / "x" / "framebuffer.npy"), np.load(tmp_path / "y" / "framebuffer.npy")
    assert x.dtype == np.float32 and x.shape == (100, 3) and np.array_equal(x, y)  # the same pixels every run
    pix = (x[:, 0] / 1.5).astype(np.int64)  # channel 0 of pixel p holds 0.5 * 3p
    assert np.all(np.diff(pix) > 0) and pix.max() < W * H  # distinct pixels, ascending
    assert np.array_equal(x, frame(W, H).numpy().reshape(-1, 3)[pix])


def test_dump_limit_is_under_64_mb():
    assert bench.DUMP_MAX_FLOATS * 4 + 128 <= 64 * 10 ** 6
