"""Batch moments and the variance-guided filter, the parts that need no GPU: the numpy
restatements batch_moments_numpy and denoise_var_numpy against what they must mean, the batch windows,
the library's new symbols and defaults against the header, and the command line's usage errors before
any device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bdpt_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bdpt_amd.h")
CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")


def test_symbols_and_defaults_match_the_header():
    L = bdpt_amd.lib()
    for name in ("bdpt_batch_moments", "bdpt_batch_moments_host", "bdpt_denoise_var", "bdpt_denoise_var_host"):
        assert getattr(L, name).argtypes
    text = open(HEADER).read()
    it = int(re.search(r"^#define BDPT_DENOISE_VAR_ITERATIONS\s+(\d+)\s*$", text, re.M).group(1))
    sc = float(re.search(r"^#define BDPT_DENOISE_VAR_SIGMA_COLOR\s+([0-9.]+)f\s*$", text, re.M).group(1))
    d, base = bdpt_amd.denoise_var_settings(), bdpt_amd.DenoiseSettings()
    assert (d.iterations, d.sigma_color) == (it, sc)
    assert (d.sigma_normal, d.sigma_depth, d.demodulate) == (base.sigma_normal, base.sigma_depth, base.demodulate)
    # the argument checks come before any device call (a null context is refused, not dereferenced)
    one = np.zeros(8, np.float32)
    p = bdpt_amd.DenoiseSettings().c(1.0)
    assert L.bdpt_batch_moments_host(None, 1, 1, 2, one.ctypes.data, None, one.ctypes.data) == bdpt_amd.ERR_INVALID
    assert L.bdpt_denoise_var_host(None, 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, None,
                                   ctypes.byref(p)) == bdpt_amd.ERR_INVALID


def test_batch_windows_partition_the_window():
    W = bdpt_amd.SampleWindow
    assert bdpt_amd.batch_windows(8, 4) == [W(0, 4, 2), W(1, 4, 2), W(2, 4, 2), W(3, 4, 2)]
    wins = bdpt_amd.batch_windows(64, 3, W(5, 2, 12))
    assert wins == [W(5, 6, 4), W(7, 6, 4), W(9, 6, 4)]
    assert sorted(k for w in wins for k in w.samples()) == list(W(5, 2, 12).samples())
    for n in (1, 65, 0, -2):
        with pytest.raises(ValueError, match="n_batches"):
            bdpt_amd.batch_windows(64, n)
    for spp, n, w in ((9, 4, None), (8, 4, W(0, 1, 6)), (8, 4, W(0, 1, 0))):
        with pytest.raises(ValueError, match="count"):
            bdpt_amd.batch_windows(spp, n, w)


def test_batch_moments_numpy_is_the_sum_and_the_scaled_sample_variance():
    rng = np.random.default_rng(7)
    for K in (2, 3, 8):
        planes = rng.standard_normal((K, 6, 5, 3)).astype(np.float32) * 3 + 1
        s, v = bdpt_amd.batch_moments_numpy(planes, np.float64)
        p64 = planes.astype(np.float64)
        assert np.allclose(s, p64.sum(0), rtol=1e-13, atol=1e-13)
        assert np.allclose(v, K * p64.var(0, ddof=1), rtol=1e-6, atol=0)  # (c = K / (K - 1) is formed in float32)
        s32, v32 = bdpt_amd.batch_moments_numpy(planes)
        assert s32.dtype == np.float32 and v32.dtype == np.float32
        assert np.allclose(s32, s, rtol=1e-5, atol=1e-5) and np.allclose(v32, v, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError, match="n_batches"):
        bdpt_amd.batch_moments_numpy(np.zeros((1, 2, 2, 3), np.float32))


def test_batch_moments_numpy_estimates_the_variance_of_the_sum():
    """K planes of N(0, 1): S has variance K, so mean(var) / K estimates 1 with standard error
    sqrt(2 / ((K - 1) N)) (a chi-square of (K - 1) N degrees of freedom); six of them allowed."""
    K, N = 4, 30000
    planes = np.random.default_rng(12345).standard_normal((K, N // 3 // 100, 100, 3)).astype(np.float32)
    assert planes[0].size == N
    _, v = bdpt_amd.batch_moments_numpy(planes)
    assert abs(v.astype(np.float64).mean() / K - 1) <= 6 * np.sqrt(2 / ((K - 1) * N))


def flat_guides(H, W):
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 2.0, 1.0
    return aov


def test_denoise_var_numpy_keeps_a_constant_image():
    H, W = 20, 24
    rgb = np.empty((H, W, 3), np.float32)
    rgb[:] = (0.25, 1.5, 3.0)
    var = np.random.default_rng(1).random((H, W, 3)).astype(np.float32)
    for demodulate in (False, True):
        s = bdpt_amd.DenoiseSettings(iterations=4, sigma_color=1.0, demodulate=demodulate)
        out, v = bdpt_amd.denoise_var_numpy(rgb, var, flat_guides(H, W), s)
        assert np.abs(out / rgb - 1).max() <= 1e-12
        assert (v > 0).all() and v.max() < (3 * 4 if demodulate else 3)  # a weighted mean of U, shrunk


def test_denoise_var_numpy_zero_variance_keeps_a_checkerboard():
    H, W = 20, 24
    yy, xx = np.mgrid[:H, :W]
    rgb = np.where(((yy + xx) % 2 == 0)[..., None], np.float32([0.2, 0.4, 0.8]), np.float32([1.0, 0.5, 0.1]))
    rgb = rgb.astype(np.float32)
    for demodulate in (False, True):
        s = bdpt_amd.DenoiseSettings(iterations=3, sigma_color=4.0, demodulate=demodulate)
        out, v = bdpt_amd.denoise_var_numpy(rgb, np.zeros_like(rgb), flat_guides(H, W), s)
        assert np.abs(out / rgb - 1).max() <= 1e-6  # every other colour is 1e10 "deviations" away: exp(-80)
        assert (v == 0).all()


def test_denoise_var_numpy_shrinks_a_constant_variance_by_the_kernel_energy():
    """Flat guides, huge sigmas: every weight is 1, and one iteration multiplies a constant V by
    (sum h^2)^2 = (70 / 256)^2 wherever all 25 taps are inside (sum h^2 of [1, 4, 6, 4, 1] / 16 = 70 / 256)."""
    H, W = 20, 24
    rgb = np.random.default_rng(2).random((H, W, 3)).astype(np.float32)
    var = np.full((H, W, 3), 0.5, np.float32)
    s = bdpt_amd.DenoiseSettings(iterations=1, sigma_color=1e30, sigma_normal=1e30, sigma_depth=1e30, demodulate=False)
    _, v = bdpt_amd.denoise_var_numpy(rgb, var, flat_guides(H, W), s)
    assert np.allclose(v[2:-2, 2:-2], 1.5 * (70 / 256) ** 2, rtol=1e-12, atol=0)
    assert (v[0, :] > v[2, 2]).all()  # fewer taps at the border: less averaging


def test_denoise_var_numpy_zero_iterations():
    H, W = 9, 11
    rng = np.random.default_rng(3)
    rgb, var = rng.random((H, W, 3)).astype(np.float32), rng.random((H, W, 3)).astype(np.float32)
    s = bdpt_amd.DenoiseSettings(iterations=0, demodulate=False)
    out, v0 = bdpt_amd.denoise_var_numpy(rgb, var, flat_guides(H, W), s, norm=2.0)
    assert np.array_equal(out, rgb.astype(np.float64) * 2.0)
    U = var.astype(np.float64).sum(-1) * 4.0
    k = np.array([1, 2, 1]) / 4
    y, x = 4, 5  # an interior pixel: the full 3 x 3 kernel, which sums to 1
    want = sum(k[dy + 1] * k[dx + 1] * U[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert abs(v0[y, x] / want - 1) <= 1e-12
    want = sum(k[dy + 1] * k[dx + 1] * U[dy, dx] for dy in (0, 1) for dx in (0, 1)) / (9 / 16)  # the corner: 4 taps
    assert abs(v0[0, 0] / want - 1) <= 1e-12


def test_cli_batches_usage_errors_before_any_device(tmp_path):
    """Every misuse names its flag and is refused before a device is opened (none is visible) and before
    anything is written."""
    import variants

    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 6))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    cases = (
        (["--batches", "1"], "--batches"), (["--batches", "65"], "--batches"), (["--batches", "x"], "--batches"),
        (["--batches", "4"], "--batches"),  # spp 6 is no multiple of 4
        (["--batches", "2", "--sample-window", "0:1:3"], "--batches"),
        (["--batches", "2", "--sample-window", "0:1:0"], "--batches"),
        (["--denoise-var"], "--denoise-var"), (["--denoise-var=9", "--batches", "2"], "--denoise-var"),
        (["--denoise-var=", "--batches", "2"], "--denoise-var"), (["--denoise-varx", "--batches", "2"], "--denoise-var"),
        (["--denoise-var", "--denoise", "--batches", "2"], "--denoise-var"),
        (["--batches", "2", "--gpus", "2"], "--batches"), (["--batches", "2", "--devices", "0,1"], "--batches"),
        (["--batches", "2", "--layers", "3"], "--batches"), (["--batches", "2", "--light-groups"], "--batches"),
        (["--batches", "2", "--strategies"], "--batches"),
    )
    for flags, named in cases:
        r = subprocess.run([CLI, str(toml)] + flags, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode != 0 and named in r.stderr, (flags, r.stderr)
        assert "hip" not in r.stderr.lower() and "bdpt_ctx_create" not in r.stderr, (flags, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["scene.toml"]
