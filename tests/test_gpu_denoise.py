"""The edge-avoiding a-trous filter (bdpt_denoise) on the GPU against a numpy restatement of
the formulas in include/bdpt_amd.h, in float64 (the reference) and in float32 (what
single precision alone costs: the yardstick of the tolerance)."""
import ctypes

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


def atrous(color, aov, iterations, sigma_color, sigma_normal, sigma_depth, demodulate, norm, dt=np.float64):
    """bdpt_denoise as the header states it, every operation in `dt`."""
    f = dt
    c = color.astype(dt) * f(norm)
    a = aov.astype(dt) * f(norm)
    if iterations == 0:
        return c
    H, W = c.shape[:2]
    cov = a[..., 7]
    hit = cov > 0
    safe = np.where(hit, cov, f(1))
    alb = np.where(hit[..., None], a[..., 0:3] / safe[..., None], f(1))
    N = np.where(hit[..., None], a[..., 3:6] / safe[..., None], f(0))
    z = np.where(hit, a[..., 6] / safe, f(0))
    m = np.maximum(alb, f(1e-3))
    img = c / m if demodulate else c
    kern = np.array([1, 4, 6, 4, 1], dt) / f(16)
    zs = f(sigma_depth) * np.maximum(z, f(1e-6))
    for i in range(iterations):
        s = 1 << i
        sc = f(sigma_color) * f(2.0 ** -i)
        num = np.zeros_like(img)
        den = np.zeros((H, W), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                py = slice(max(0, -oy), min(H, H - oy))
                px = slice(max(0, -ox), min(W, W - ox))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                h = kern[dy + 2] * kern[dx + 2]
                if dx == 0 and dy == 0:
                    w = np.ones((H, W), dt)
                else:
                    dc = img[py, px] - img[qy, qx]
                    dn = N[py, px] - N[qy, qx]
                    dz = z[py, px] - z[qy, qx]
                    wc = np.exp(-np.minimum(((dc[..., 0] ** 2 + dc[..., 1] ** 2) + dc[..., 2] ** 2) / (sc * sc), f(80)))
                    wn = np.exp(-np.minimum(((dn[..., 0] ** 2 + dn[..., 1] ** 2) + dn[..., 2] ** 2)
                                            / (f(sigma_normal) * f(sigma_normal)), f(80)))
                    wz = np.exp(-np.minimum((dz * dz) / (zs[py, px] * zs[py, px]), f(80)))
                    w = np.where(hit[py, px] == hit[qy, qx], (wc * wn) * wz, f(0))
                hw = h * w
                num[py, px] += hw[..., None] * img[qy, qx]
                den[py, px] += hw
        img = num / den[..., None]
    return img * m if demodulate else img


def rel_l2(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return np.linalg.norm(a - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-8)


def integrator(W, H, spp):
    cam = bdpt_amd.Camera(**variants.SCENES["hardlight"]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=variants.SCENES["hardlight"]["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    it.init()
    return it


_inputs = {}


def inputs(norm):
    """The 4-spp HardLight 40 x 28 frame with its feature buffers (norm 1), or half of its
    samples through a window (norm 2); rendered once."""
    if norm not in _inputs:
        it = integrator(40, 28, 4)
        window = None if norm == 1 else bdpt_amd.SampleWindow(0, 1, 2)
        it.render_frame(window=window)
        it.render_aov(window=window)
        _inputs[norm] = (it, it.rgb.copy(), it.aov.copy())
    return _inputs[norm]


# Worst per-pixel relative L2 of the float32 restatement against the float64 one on the
# inputs above (dumped from the GPU, measured on the host), keyed (iterations, demodulate,
# norm). The test allows 4 x that: the device's exp and division differ from numpy's by a
# few ulp. The largest of them and the GPU's own figures are in the commit message.
F32_VS_F64 = {
    (1, 0, 1): 6.166e-07, (1, 1, 1): 6.104e-07, (3, 0, 1): 7.047e-07, (3, 1, 1): 7.323e-07,
    (5, 0, 1): 7.541e-07, (5, 1, 1): 8.656e-07, (1, 0, 2): 9.910e-07, (1, 1, 2): 8.607e-07,
    (3, 0, 2): 1.067e-06, (3, 1, 2): 1.014e-06, (5, 0, 2): 1.578e-06, (5, 1, 2): 1.630e-06,
}
SIGMAS = dict(sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.1)  # the formula test's own (not the defaults' business)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_gpu_denoise_matches_the_formula(iterations, demodulate, norm):
    it, rgb, aov = inputs(norm)
    out = it.denoise(rgb, aov, samples_done=4 // norm, iterations=iterations, demodulate=bool(demodulate), **SIGMAS)
    ref = atrous(rgb, aov, iterations, demodulate=demodulate, norm=norm, **SIGMAS)
    err = rel_l2(out, ref).max()
    f32 = rel_l2(atrous(rgb, aov, iterations, demodulate=demodulate, norm=norm, dt=np.float32, **SIGMAS), ref).max()
    print(f"iterations {iterations} demodulate {demodulate} norm {norm}: GPU {err:.3e}, float32 numpy here {f32:.3e}")
    assert np.isfinite(out).all()
    assert err <= 4 * F32_VS_F64[(iterations, demodulate, norm)]


def test_gpu_denoise_zero_iterations_is_the_scaled_input():
    it, rgb, aov = inputs(2)
    out = it.denoise(rgb, aov, samples_done=2, iterations=0)
    assert np.array_equal(out, rgb * np.float32(2))
    assert np.array_equal(it.denoise(rgb, aov, iterations=0, demodulate=False), rgb)


def flat_guides(H, W, cov=1.0):
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 2.0, 1.0
    return aov * np.float32(cov)


def test_gpu_denoise_keeps_a_constant_image():
    it, _, _ = inputs(1)
    rgb = np.empty((28, 40, 3), np.float32)
    rgb[:] = (0.25, 1.5, 3.0)
    for demodulate in (False, True):
        out = it.denoise(rgb, flat_guides(28, 40), iterations=5, demodulate=demodulate)
        assert np.abs(out / rgb - 1).max() <= 1e-6


def test_gpu_denoise_without_edge_stopping_is_the_b3_blur():
    """All sigmas 1e30: every weight is exp(-0) = 1, and one iteration is the 5 x 5 B3-spline
    blur renormalised at the borders."""
    it, rgb, aov = inputs(1)
    out = it.denoise(rgb, flat_guides(28, 40), iterations=1, demodulate=False, sigma_color=1e30, sigma_normal=1e30,
                     sigma_depth=1e30)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    img = rgb.astype(np.float64)
    num, den = np.zeros_like(img), np.zeros((28, 40))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            py, px = slice(max(0, -dy), min(28, 28 - dy)), slice(max(0, -dx), min(40, 40 - dx))
            qy, qx = slice(py.start + dy, py.stop + dy), slice(px.start + dx, px.stop + dx)
            num[py, px] += k[dy + 2] * k[dx + 2] * img[qy, qx]
            den[py, px] += k[dy + 2] * k[dx + 2]
    assert rel_l2(out, num / den[..., None]).max() <= 1e-6  # 25 float32 products and sums


def test_gpu_denoise_miss_pixels_do_not_mix_with_hits():
    """A block of miss pixels (coverage 0) of one colour inside hit pixels of another: its
    same-class neighbours are all equal, so it keeps its value exactly."""
    it, _, _ = inputs(1)
    aov = flat_guides(28, 40)
    rgb = np.full((28, 40, 3), 2.0, np.float32)
    aov[5:9, 7:12] = 0.0
    rgb[5:9, 7:12] = (0.125, 0.5, 0.75)
    aov[20, 30] = 0.0  # a lone miss pixel: only its centre tap counts
    rgb[20, 30] = (9.0, 8.0, 7.0)
    out = it.denoise(rgb, aov, iterations=3, demodulate=True)
    assert np.array_equal(out[5:9, 7:12], rgb[5:9, 7:12])
    assert np.array_equal(out[20, 30], rgb[20, 30])


def test_gpu_denoise_is_deterministic_and_device_equals_host():
    import torch

    it, rgb, aov = inputs(1)
    a = it.denoise(rgb, aov)
    assert np.array_equal(a, it.denoise(rgb, aov))
    dev = torch.device("cuda", 0)
    trgb, taov = torch.from_numpy(rgb).to(dev), torch.from_numpy(aov).to(dev)
    tout = torch.zeros_like(trgb)
    torch.cuda.synchronize()
    it.denoise_device(trgb.data_ptr(), taov.data_ptr(), tout.data_ptr())
    it.synchronize()
    assert np.array_equal(tout.cpu().numpy(), a)


def test_gpu_denoise_lowers_the_error_of_a_4spp_frame():
    """HardLight 64 x 64: the mean squared error against a 256-spp frame, before and after
    the filter with the default settings. A condition, not a tuned number."""
    ref = integrator(64, 64, 256).render_frame().astype(np.float64)
    it = integrator(64, 64, 4)
    noisy = it.render_frame().copy()
    it.render_aov()
    den = it.denoise()
    e_noisy = np.mean((noisy - ref) ** 2)
    e_den = np.mean((den - ref) ** 2)
    print(f"MSE against 256 spp: 4-spp frame {e_noisy:.6g}, denoised {e_den:.6g}")
    assert e_den < e_noisy


def test_gpu_denoise_refusals():
    it, rgb, aov = inputs(1)
    for field, kw in (("iterations", dict(iterations=9)), ("sigma_color", dict(sigma_color=0.0))):
        with pytest.raises(bdpt_amd.BdptError, match=field) as e:
            it.denoise(rgb, aov, **kw)
        assert e.value.code == bdpt_amd.ERR_INVALID
    d = bdpt_amd.DenoiseSettings().c(0.0)
    out = np.zeros_like(rgb)
    L = bdpt_amd.lib()
    assert L.bdpt_denoise_host(it._h, 40, 28, rgb.ctypes.data, aov.ctypes.data, out.ctypes.data,
                               ctypes.byref(d)) == bdpt_amd.ERR_INVALID
    assert b"norm" in L.bdpt_last_error()
    d = bdpt_amd.DenoiseSettings().c(1.0)
    assert L.bdpt_denoise_host(it._h, 40, 28, rgb.ctypes.data, aov.ctypes.data, rgb.ctypes.data,
                               ctypes.byref(d)) == bdpt_amd.ERR_INVALID
    assert b"out overlaps color" in L.bdpt_last_error()
