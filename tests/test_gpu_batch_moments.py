"""Sample batches, their per-pixel moments (bdpt_batch_moments) and the variance-guided filter
(bdpt_denoise_var) on the GPU: the batches against the windows they are, the moments
against the float32 loop of batch_moments_numpy bit for bit, the filter against denoise_var_numpy in
float64 with the float32 restatement as the yardstick of the tolerance, and the command line's files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import gpu_available
from test_config_exr import decode_exr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

TOL = 1e-4  # the suite's per-pixel relative L2 (tests/test_gpu_parity.py)
W, H = 40, 28


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(a - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-8)


def integrator(width, height, spp, cls=bdpt_amd.BDPTIntegrator):
    sc = variants.SCENES["hardlight"]
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=width, height=height, spp=spp,
                          rr_depth=sc["rr_depth"])
    it = cls(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    it.init()
    return it


_cache = {}


def batches(K):
    """HardLight 40 x 28 at 24 spp as K batches (24 = 2 * 3 * 4: every K of the moments test divides it);
    rendered once per K."""
    if ("planes", K) not in _cache:
        it = integrator(W, H, 24)
        _cache["planes", K] = (it, it.render_batches(K).copy())
    return _cache["planes", K]


def inputs(norm):
    """8 samples per pixel of HardLight 40 x 28 in 8 batches with their moments and feature buffers: the
    whole 8-spp frame (norm 1), or the first half of a 16-spp frame through a window (norm 2). Rendered
    once, never changed."""
    if ("inputs", norm) not in _cache:
        it = integrator(W, H, 8 * norm)
        window = None if norm == 1 else bdpt_amd.SampleWindow(0, 1, 8)
        planes = it.render_batches(8, window=window)
        s, v = it.batch_moments(planes)
        it.render_aov(window=window)
        _cache["inputs", norm] = (it, s.copy(), v.copy(), it.aov.copy())
    return _cache["inputs", norm]


# ---------------------------------------------------------------- batches
def test_gpu_batches_are_the_windows_and_sum_to_the_frame():
    it = integrator(W, H, 8)
    planes = it.render_batches(4).copy()
    assert planes.shape == (4, H, W, 3) and planes.dtype == np.float32
    frame = it.render_frame().copy()
    e = rel_l2(planes.astype(np.float64).sum(0), frame).max()
    it.init()
    one = it.render_frame(window=bdpt_amd.SampleWindow(1, 4, 2)).copy()
    e1 = rel_l2(planes[1], one).max()
    print(f"sum of 4 batches against render_frame: {e:.3e}; plane 1 against its window: {e1:.3e}")
    assert e <= TOL and e1 <= TOL
    assert np.abs(planes[0] - planes[1]).max() > 0  # independent samples, not copies


def test_gpu_batches_of_the_path_tracer_sum_to_its_frame():
    it = integrator(W, H, 8, bdpt_amd.PathTracerIntegrator)
    planes = it.render_batches(4).copy()
    frame = it.render_frame().copy()
    e = rel_l2(planes.astype(np.float64).sum(0), frame).max()
    print(f"path tracer, sum of 4 batches against render_frame: {e:.3e}")
    assert e <= TOL
    assert np.abs(frame).max() > 0


def test_gpu_batches_refuse_bad_counts_before_any_render():
    it = integrator(W, H, 8)
    for n in (1, 65):
        with pytest.raises(ValueError, match="n_batches"):
            it.render_batches(n)
    with pytest.raises(ValueError, match="count"):
        it.render_batches(3)  # 8 spp
    with pytest.raises(ValueError, match="count"):
        it.render_batches(4, window=bdpt_amd.SampleWindow(0, 1, 6))
    with pytest.raises(ValueError, match="count"):
        it.render_batches_device(3, 0)
    assert it.batches is None


# ---------------------------------------------------------------- moments
def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("K", [2, 3, 8])
def test_gpu_batch_moments_have_the_bits_of_the_float32_loop(K):
    it, planes = batches(K)
    s, v = it.batch_moments(planes)
    rs, rv = bdpt_amd.batch_moments_numpy(planes, np.float32)
    assert np.array_equal(s, rs) and np.array_equal(v, rv)
    assert it.rgb is s and it.var is v
    assert v.min() >= 0 and v.max() > 0
    st = it.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0
    if K == 8:  # the same sum as the layers' compose with every bit set
        assert np.array_equal(s, it.compose_layers(planes, range(K)))


def test_gpu_batch_moments_synthetic_frame_of_extremes():
    """37 x 5 (555 floats a plane: no multiple of a block or of the 16-byte path) of zeros, 1e-20 (whose
    squares are float32 denormals) and 1e6, in every mixture across 3 planes."""
    it, _ = batches(2)
    rng = np.random.default_rng(5)
    planes = rng.choice(np.float32([0.0, 1e-20, 1e6]), size=(3, 5, 37, 3)).astype(np.float32)
    planes[:, 0, 0] = 0.0
    planes[:, 0, 1] = 1e-20
    planes[:, 0, 2] = 1e6
    s, v = it.batch_moments(planes)
    rs, rv = bdpt_amd.batch_moments_numpy(planes, np.float32)
    assert np.array_equal(s, rs) and np.array_equal(v, rv)
    assert same_bits(v[0, 0], np.zeros(3)) and same_bits(v[0, 2], np.zeros(3))


def test_gpu_batch_moments_device_form_null_sum_and_determinism():
    import torch

    it, planes = batches(8)
    s, v = it.batch_moments(planes)
    s2, v2 = it.batch_moments(planes)
    assert np.array_equal(s, s2) and np.array_equal(v, v2)
    dev = torch.device("cuda", 0)
    tp = torch.from_numpy(planes).to(dev)
    ts, tv = torch.zeros((H, W, 3), device=dev), torch.zeros((H, W, 3), device=dev)
    torch.cuda.synchronize()
    it.batch_moments_device(tp.data_ptr(), 8, W, H, ts.data_ptr(), tv.data_ptr())
    it.synchronize()
    assert np.array_equal(ts.cpu().numpy(), s) and np.array_equal(tv.cpu().numpy(), v)
    tv.zero_()
    torch.cuda.synchronize()
    it.batch_moments_device(tp.data_ptr(), 8, W, H, 0, tv.data_ptr())  # out_sum = NULL
    it.synchronize()
    assert np.array_equal(tv.cpu().numpy(), v)
    only_var = np.zeros((H, W, 3), np.float32)
    bdpt_amd._check(bdpt_amd.lib().bdpt_batch_moments_host(it._h, W, H, 8, planes.ctypes.data, None, only_var.ctypes.data))
    assert np.array_equal(only_var, v)


def test_gpu_batch_moments_refusals():
    it, planes = batches(2)
    L = bdpt_amd.lib()
    big = np.zeros((66, H, W, 3), np.float32)
    s, v = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)

    def refused(what, *args):
        assert L.bdpt_batch_moments_host(it._h, *args) == bdpt_amd.ERR_INVALID, what
        assert what.encode() in L.bdpt_last_error(), (what, L.bdpt_last_error())

    refused("n_batches", W, H, 1, big.ctypes.data, s.ctypes.data, v.ctypes.data)
    refused("n_batches", W, H, 65, big.ctypes.data, s.ctypes.data, v.ctypes.data)
    refused("n_batches * width * height", 32768, 32768, 2, big.ctypes.data, s.ctypes.data, v.ctypes.data)
    refused("width/height", 0, H, 2, big.ctypes.data, s.ctypes.data, v.ctypes.data)
    refused("planes", W, H, 2, None, s.ctypes.data, v.ctypes.data)
    refused("out_var must not be NULL", W, H, 2, big.ctypes.data, s.ctypes.data, None)
    refused("out_sum overlaps planes", W, H, 2, big.ctypes.data, big[1].ctypes.data, v.ctypes.data)
    refused("out_var overlaps planes", W, H, 2, big.ctypes.data, s.ctypes.data, big[0, 3:].ctypes.data)
    refused("out_var overlaps out_sum", W, H, 2, big.ctypes.data, s.ctypes.data, s.ctypes.data)
    assert L.bdpt_batch_moments(it._h, W, H, 65, big.ctypes.data, None, v.ctypes.data, None) == bdpt_amd.ERR_INVALID
    with pytest.raises(bdpt_amd.BdptError, match="n_batches"):
        it.batch_moments(big[:1])


# ---------------------------------------------------------------- filter vs formula
# Worst figures of the float32 restatement (denoise_var_numpy, dt = float32) against the float64 one on
# the inputs above (dumped from the GPU, measured on the host), keyed (iterations, demodulate, norm):
# (per-pixel relative L2 of out, |out_var difference| over max out_var). The test allows 4 x that, the
# margin of tests/test_gpu_denoise.py: the device's exp and division differ from numpy's by a few ulp. The
# GPU's own figures on that run were 0.4 to 1.4 x these for out and 0.9 to 1.6 x for out_var.
F32_VS_F64 = {
    (1, 0, 1): (1.348e-06, 2.213e-07), (1, 1, 1): (1.286e-06, 2.222e-07), (3, 0, 1): (2.927e-06, 2.337e-07),
    (3, 1, 1): (4.208e-06, 4.394e-07), (5, 0, 1): (2.925e-06, 2.337e-07), (5, 1, 1): (4.228e-06, 4.394e-07),
    (1, 0, 2): (5.695e-07, 2.322e-07), (1, 1, 2): (3.925e-07, 2.077e-07), (3, 0, 2): (1.832e-06, 2.875e-07),
    (3, 1, 2): (1.685e-06, 2.827e-07), (5, 0, 2): (1.810e-06, 2.875e-07), (5, 1, 2): (1.661e-06, 2.827e-07),
}
SIGMAS = dict(sigma_color=2.0, sigma_normal=0.3, sigma_depth=0.1)  # the formula test's own (not the defaults' business)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_gpu_denoise_var_matches_the_formula(iterations, demodulate, norm):
    it, rgb, var, aov = inputs(norm)
    s = bdpt_amd.DenoiseSettings(iterations=iterations, demodulate=bool(demodulate), **SIGMAS)
    out, ov = it.denoise_var(rgb, var, aov, samples_done=8, return_variance=True, settings=s)
    ref, rv = bdpt_amd.denoise_var_numpy(rgb, var, aov, s, norm=norm)
    f32, fv = bdpt_amd.denoise_var_numpy(rgb, var, aov, s, norm=norm, dt=np.float32)
    err, err_v = rel_l2(out, ref).max(), np.abs(ov - rv).max() / rv.max()
    e32, e32_v = rel_l2(f32, ref).max(), np.abs(fv - rv).max() / rv.max()
    print(f"iterations {iterations} demodulate {demodulate} norm {norm}: GPU {err:.3e} / {err_v:.3e}, "
          f"float32 numpy here {e32:.3e} / {e32_v:.3e}")
    assert np.isfinite(out).all() and np.isfinite(ov).all() and rv.max() > 0
    bound, bound_v = F32_VS_F64[(iterations, demodulate, norm)]
    assert err <= 4 * bound
    assert err_v <= 4 * bound_v


# ---------------------------------------------------------------- properties
def flat_guides(cov=1.0):
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 2.0, 1.0
    return aov * np.float32(cov)


def test_gpu_denoise_var_zero_iterations_is_the_scaled_input_and_v0():
    it, rgb, var, aov = inputs(2)
    out, v0 = it.denoise_var(rgb, var, aov, samples_done=8, return_variance=True, iterations=0, demodulate=False)
    assert np.array_equal(out, rgb * np.float32(2))
    assert np.array_equal(it.denoise_var(rgb, var, aov, samples_done=8, iterations=0), out)  # out_var = NULL
    _, ref = bdpt_amd.denoise_var_numpy(rgb, var, aov, bdpt_amd.DenoiseSettings(iterations=0, demodulate=False), norm=2.0)
    # positive terms only, so the relative errors of the ~20 float32 roundings on the way add: 20 * 2^-24
    # (miss pixels without variance have V_0 = 0 on both sides, hence no quotient)
    assert (np.abs(v0 - ref) <= 20 * 2.0 ** -24 * ref).all() and ref.max() > 0
    _, v0d = it.denoise_var(rgb, var, aov, samples_done=8, return_variance=True, iterations=0, demodulate=True)
    _, refd = bdpt_amd.denoise_var_numpy(rgb, var, aov, bdpt_amd.DenoiseSettings(iterations=0, demodulate=True), norm=2.0)
    assert (np.abs(v0d - refd) <= 20 * 2.0 ** -24 * refd).all() and refd.max() > 0


def test_gpu_denoise_var_keeps_a_constant_image():
    it, _, var, _ = inputs(1)
    rgb = np.empty((H, W, 3), np.float32)
    rgb[:] = (0.25, 1.5, 3.0)
    for demodulate in (False, True):
        out = it.denoise_var(rgb, var, flat_guides(), iterations=5, demodulate=demodulate)
        assert np.abs(out / rgb - 1).max() <= 1e-6


def test_gpu_denoise_var_zero_variance_keeps_a_checkerboard():
    it, _, _, _ = inputs(1)
    yy, xx = np.mgrid[:H, :W]
    rgb = np.where(((yy + xx) % 2 == 0)[..., None], np.float32([0.2, 0.4, 0.8]), np.float32([1.0, 0.5, 0.1]))
    rgb = rgb.astype(np.float32)
    for demodulate in (False, True):
        out, ov = it.denoise_var(rgb, np.zeros_like(rgb), flat_guides(), return_variance=True, iterations=3,
                                 sigma_color=4.0, demodulate=demodulate)
        assert np.abs(out / rgb - 1).max() <= 1e-6
        assert (ov == 0).all()


def test_gpu_denoise_var_shrinks_a_constant_variance_by_the_kernel_energy():
    """Flat guides and huge sigmas: every weight is 1, so one iteration multiplies the constant V = 1.5 by
    (70 / 256)^2 wherever all 25 taps are inside the image."""
    it, rgb, _, _ = inputs(1)
    var = np.full((H, W, 3), 0.5, np.float32)
    _, ov = it.denoise_var(rgb, var, flat_guides(), return_variance=True, iterations=1, demodulate=False,
                           sigma_color=1e15, sigma_normal=1e15, sigma_depth=1e15)
    assert np.abs(ov[2:-2, 2:-2] / (1.5 * (70 / 256) ** 2) - 1).max() <= 1e-6
    assert (ov[0] > ov[2, 2]).all()


def test_gpu_denoise_var_miss_pixels_do_not_mix_with_hits():
    it, _, var, _ = inputs(1)
    aov = flat_guides()
    rgb = np.full((H, W, 3), 2.0, np.float32)
    aov[5:9, 7:12] = 0.0
    rgb[5:9, 7:12] = (0.125, 0.5, 0.75)
    aov[20, 30] = 0.0  # a lone miss pixel: only its centre tap counts
    rgb[20, 30] = (9.0, 8.0, 7.0)
    out = it.denoise_var(rgb, var, aov, iterations=3, demodulate=True)
    assert np.array_equal(out[5:9, 7:12], rgb[5:9, 7:12])
    assert np.array_equal(out[20, 30], rgb[20, 30])


def test_gpu_denoise_var_is_deterministic_and_device_equals_host():
    import torch

    it, rgb, var, aov = inputs(1)
    a, av = it.denoise_var(rgb, var, aov, return_variance=True)
    b, bv = it.denoise_var(rgb, var, aov, return_variance=True)
    assert np.array_equal(a, b) and np.array_equal(av, bv)
    assert it.stats()["launches"] == 2 + bdpt_amd.denoise_var_settings().iterations
    dev = torch.device("cuda", 0)
    trgb, tvar, taov = (torch.from_numpy(x).to(dev) for x in (rgb, var, aov))
    tout, tov = torch.zeros_like(trgb), torch.zeros((H, W), device=dev)
    torch.cuda.synchronize()
    it.denoise_var_device(trgb.data_ptr(), tvar.data_ptr(), taov.data_ptr(), tout.data_ptr(), tov.data_ptr())
    it.synchronize()
    assert np.array_equal(tout.cpu().numpy(), a) and np.array_equal(tov.cpu().numpy(), av)
    # the plain filter shares the scratch and keeps its result around a call of this one
    plain = it.denoise(rgb, aov)
    it.denoise_var(rgb, var, aov)
    assert np.array_equal(it.denoise(rgb, aov), plain)


# ---------------------------------------------------------------- quality
def test_gpu_denoise_var_lowers_the_error_of_an_8spp_frame():
    """HardLight 64 x 64, 8 spp in 8 batches: the mean squared error against a 256-spp frame of the batches'
    sum, of the variance-guided filter with its defaults (asserted to be lower: a condition) and of the plain
    filter with its defaults on the same frame (printed: a measurement)."""
    ref = integrator(64, 64, 256).render_frame().astype(np.float64)
    it = integrator(64, 64, 8)
    it.render_batches(8)
    noisy, _ = it.batch_moments()
    it.render_aov()
    den_var = it.denoise_var()
    den = it.denoise()
    e_noisy, e_var, e_plain = (np.mean((x - ref) ** 2) for x in (noisy, den_var, den))
    print(f"MSE against 256 spp: 8-spp sum of 8 batches {e_noisy:.6g}, denoise_var {e_var:.6g}, denoise {e_plain:.6g}")
    assert e_var < e_noisy


# ---------------------------------------------------------------- refusals
def test_gpu_denoise_var_refusals():
    it, rgb, var, aov = inputs(1)
    for field, kw in (("iterations", dict(iterations=9)), ("sigma_color", dict(sigma_color=0.0)),
                      ("sigma_normal", dict(sigma_normal=-1.0)), ("sigma_depth", dict(sigma_depth=0.0))):
        with pytest.raises(bdpt_amd.BdptError, match="bdpt_denoise_var: " + field) as e:
            it.denoise_var(rgb, var, aov, **kw)
        assert e.value.code == bdpt_amd.ERR_INVALID
    L = bdpt_amd.lib()
    out, ov = np.zeros_like(rgb), np.zeros((H, W), np.float32)

    def refused(what, d, c, v, a, o, o2):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        assert L.bdpt_denoise_var_host(it._h, W, H, p(c), p(v), p(a), p(o), p(o2), ctypes.byref(d)) == bdpt_amd.ERR_INVALID
        assert what.encode() in L.bdpt_last_error(), (what, L.bdpt_last_error())

    ok = bdpt_amd.denoise_var_settings().c(1.0)
    refused("norm", bdpt_amd.denoise_var_settings().c(0.0), rgb, var, aov, out, ov)
    bad = bdpt_amd.denoise_var_settings().c(1.0)
    bad.demodulate = 2
    refused("demodulate", bad, rgb, var, aov, out, ov)
    refused("var must not be NULL", ok, rgb, None, aov, out, ov)
    refused("out overlaps color", ok, rgb, var, aov, rgb, ov)
    refused("out overlaps var", ok, rgb, var, aov, var, ov)
    refused("out overlaps aov", ok, rgb, var, aov, aov.reshape(-1)[8:], ov)
    refused("out_var overlaps color", ok, rgb, var, aov, out, rgb.reshape(-1)[4:])
    refused("out_var overlaps var", ok, rgb, var, aov, out, var)
    refused("out_var overlaps aov", ok, rgb, var, aov, out, aov)
    refused("out_var overlaps out", ok, rgb, var, aov, out, out.reshape(-1)[W * H:])
    with pytest.raises(bdpt_amd.BdptError, match="var"):
        it.denoise_var(rgb, var[:1], aov)


def half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_gpu_cli_batches_write_the_sum_its_variance_and_the_filtered_frame(tmp_path):
    cw, ch, spp = 32, 24, 8
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", cw, ch, spp))
    r = subprocess.run([cli, str(toml), "--batches", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--batches" in r.stderr and sorted(os.listdir(tmp_path)) == ["scene.toml"]
    r = subprocess.run([cli, str(toml), "--batches", "4", "--denoise-var"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["scene.exr", "scene.toml", "scene_denoised.exr", "scene_variance.exr"]
    main, var, den = (decode_exr((tmp_path / f"scene{s}.exr").read_bytes()).astype(np.float32)
                      for s in ("", "_variance", "_denoised"))
    it = integrator(cw, ch, spp)
    it.render_batches(4)
    s, v = it.batch_moments()
    it.render_aov()
    api = it.denoise_var()
    # two renders differ by the order of their atomic additions (as every frame does): the sum and the
    # filtered frame by a half-precision ulp, the variance (a difference of nearly equal planes) by more
    assert np.allclose(main, half(s), rtol=2 ** -9, atol=1e-6)
    assert np.allclose(den, half(api), rtol=2 ** -9, atol=1e-6)
    assert np.allclose(var, half(v), rtol=1e-2, atol=1e-6)
    assert var.shape == (ch, cw, 3) and var.min() >= 0 and var.max() > 0
    assert np.abs(den - main).max() > 0  # it is not the unfiltered frame
