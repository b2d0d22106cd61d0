"""The planes filter (bdpt_denoise_planes) on the GPU: OWN mode against bdpt_denoise
per plane, bit for bit; SHARED mode against the restatement of the header's formulas in float64
(bdpt_amd.denoise_planes_numpy), with the float32 restatement's own error as the yardstick of every
tolerance (computed here on the same inputs, never a constant); that the shared weights keep the
planes summing and relighting, which weights of their own do not; chunk and block edges; determinism;
refusals; the command line."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import gpu_available
from plane_cases import EDGES_CASE, golden_integrator
from test_config_exr import decode_exr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SIGMAS = dict(sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.1)  # tests/test_gpu_denoise.py's
MARGIN = 4  # that test's margin for the device's expf and division over the float32 restatement
CHUNK = 4   # planes per launch (include/bdpt_amd.h): 2 * CHUNK + 1 planes end on a chunk of one


def rel_l2(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return np.linalg.norm(a - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-8)


def worst(a, ref):
    """Per plane, the worst per-pixel relative L2."""
    return np.array([rel_l2(x, y).max() for x, y in zip(a.reshape((-1,) + a.shape[-3:]), ref.reshape((-1,) + ref.shape[-3:]))])


def integrator(W, H, spp):
    cam = bdpt_amd.Camera(**variants.SCENES["hardlight"]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=variants.SCENES["hardlight"]["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    it.init()
    return it


_inputs = {}


def layers(norm):
    """The 4-spp HardLight 40 x 28 frame as 5 path-length layers with its feature buffers (norm 1), or
    half of its samples through a window (norm 2); rendered once, never written."""
    if ("layers", norm) not in _inputs:
        it = integrator(40, 28, 4)
        window = None if norm == 1 else bdpt_amd.SampleWindow(0, 1, 2)
        planes = it.render_layers(5, window=window)
        it.render_aov(window=window)
        _inputs[("layers", norm)] = (it, planes, it.aov.copy())
    return _inputs[("layers", norm)]


def groups():
    """The five-emitter 32 x 32 4-spp frame as light groups: iterations 4 and 5 step 16 and 32 pixels."""
    if "groups" not in _inputs:
        it = golden_integrator(EDGES_CASE)
        planes = it.render_light_groups()
        assert planes.shape == (5, 32, 32, 3)
        it.render_aov()
        _inputs["groups"] = (it, planes, it.aov.copy())
    return _inputs["groups"]


def float_sum(planes):
    """The planes' sequential float32 sum, ascending, starting from plane 0's value."""
    acc = planes[0].copy()
    for k in range(1, planes.shape[0]):
        acc = acc + planes[k]
    return acc


def other_guide(planes):
    """A guide that is not the planes' sum: the frame with its brightest plane doubled."""
    return float_sum(planes) + planes[int(np.argmax(planes.sum(axis=(1, 2, 3))))]


def restated(planes, aov, mode, guide, norm, dt, **kw):
    return bdpt_amd.denoise_planes_numpy(planes, aov, mode, guide, bdpt_amd.DenoiseSettings(**kw), norm, dt)


def check_shared_against_the_formula(it, planes, aov, norm, guide=None, **kw):
    """SHARED mode against the float64 restatement: every plane's worst pixel within MARGIN x the float32
    restatement's on the same plane, the filtered guide likewise. -> (planes, guide) of the GPU."""
    out, og = it.denoise_planes(planes, aov, "shared", guide, samples_done=it.config.spp // norm, return_guide=True, **kw)
    ref, rg = restated(planes, aov, "shared", guide, norm, np.float64, **kw)
    f32, fg = restated(planes, aov, "shared", guide, norm, np.float32, **kw)
    err, yard = worst(out, ref), worst(f32, ref)
    eg, yg = rel_l2(og, rg).max(), rel_l2(fg, rg).max()
    print(f"{kw} norm {norm}: GPU per plane {np.array2string(err, precision=3)}, float32 numpy "
          f"{np.array2string(yard, precision=3)}; guide GPU {eg:.3e}, float32 numpy {yg:.3e}")
    assert np.isfinite(out).all() and out.shape == planes.shape
    assert (err <= MARGIN * yard).all()
    assert eg <= MARGIN * yg
    return out, og


# ---- 1. OWN mode is the single-plane filter
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_gpu_own_mode_has_the_bits_of_denoise_per_plane(iterations, demodulate, norm):
    it, planes, aov = layers(norm)
    kw = dict(samples_done=4 // norm, iterations=iterations, demodulate=bool(demodulate), **SIGMAS)
    out = it.denoise_planes(planes, aov, "own", **kw)
    assert out.shape == planes.shape
    for j in range(planes.shape[0]):
        assert np.array_equal(out[j].view(np.uint32), it.denoise(planes[j], aov, **kw).view(np.uint32)), j


# ---- 2. SHARED mode: the guide is the single-plane filter of G
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 5])
def test_gpu_shared_mode_filters_the_guide_as_denoise_does(iterations, demodulate):
    it, planes, aov = layers(2)
    kw = dict(samples_done=2, iterations=iterations, demodulate=bool(demodulate), **SIGMAS)
    G = it.compose_layers(planes, range(5))
    assert np.array_equal(G.view(np.uint32), float_sum(planes).view(np.uint32))
    _, og = it.denoise_planes(planes, aov, "shared", return_guide=True, **kw)
    assert np.array_equal(og.view(np.uint32), it.denoise(G, aov, **kw).view(np.uint32))
    mine = other_guide(planes)
    _, og = it.denoise_planes(planes, aov, "shared", guide=mine, return_guide=True, **kw)
    assert np.array_equal(og.view(np.uint32), it.denoise(mine, aov, **kw).view(np.uint32))
    assert not np.array_equal(og, it.denoise(G, aov, **kw))


# ---- 3. SHARED mode: the planes against the formula
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_gpu_shared_mode_matches_the_formula_on_layers(iterations, demodulate, norm):
    it, planes, aov = layers(norm)
    check_shared_against_the_formula(it, planes, aov, norm, iterations=iterations, demodulate=bool(demodulate), **SIGMAS)


@pytest.mark.parametrize("demodulate", [0, 1])
def test_gpu_shared_mode_matches_the_formula_on_light_groups(demodulate):
    it, planes, aov = groups()
    check_shared_against_the_formula(it, planes, aov, 1, iterations=5, demodulate=bool(demodulate), **SIGMAS)
    check_shared_against_the_formula(it, planes, aov, 1, guide=other_guide(planes), iterations=5,
                                     demodulate=bool(demodulate), **SIGMAS)


# ---- 4. the planes still add up
@pytest.mark.parametrize("which", ["layers", "groups"])
def test_gpu_shared_planes_sum_to_the_filtered_guide_and_own_planes_do_not(which):
    """sum_j out[j] (added in float64) against out_guide, within MARGIN x what the float32 restatement's
    own planes miss its own guide by; OWN mode misses the same guide by more than 100 x that bound."""
    it, planes, aov = layers(1) if which == "layers" else groups()
    kw = dict(iterations=5, demodulate=True, **SIGMAS)
    out, og = it.denoise_planes(planes, aov, "shared", return_guide=True, **kw)
    f32, fg = restated(planes, aov, "shared", None, 1, np.float32, **kw)
    got = rel_l2(out.astype(np.float64).sum(axis=0), og)
    yard = rel_l2(f32.astype(np.float64).sum(axis=0), fg).max()
    print(f"{which}: sum of the shared planes against the guide: GPU {got.max():.3e}, float32 numpy {yard:.3e}")
    assert got.max() <= MARGIN * yard
    own = it.denoise_planes(planes, aov, "own", **kw)
    gap = rel_l2(own.astype(np.float64).sum(axis=0), og)
    r64, rg = restated(planes, aov, "own", None, 1, np.float64, **kw)[0], restated(planes, aov, "shared", None, 1, np.float64, **kw)[1]
    print(f"{which}: sum of the own planes against the guide: GPU {gap.max():.3e}, float64 numpy "
          f"{rel_l2(r64.sum(axis=0), rg).max():.3e}")
    assert gap.max() > 100 * MARGIN * yard


def test_gpu_relight_of_the_shared_planes_is_the_filter_of_the_relit_planes():
    """relight(out_planes, gains) against the float64 restatement of the relit planes under the same fixed
    guide, within MARGIN x what the float32 restatement, relit in float32, misses it by."""
    it, planes, aov = groups()
    kw = dict(iterations=5, demodulate=True, **SIGMAS)
    G = float_sum(planes)
    gains = np.float32([[2.0, 0.5, 0.25], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 4.0, 2.0], [8.0, 0.125, 1.0]])
    relit = gains[:, None, None, :] * planes  # (powers of two: exact in float32)
    out = it.denoise_planes(planes, aov, "shared", guide=G, **kw)
    ref = restated(relit, aov, "shared", G, 1, np.float64, **kw)[0].sum(axis=0)
    f32 = restated(planes, aov, "shared", G, 1, np.float32, **kw)[0]
    acc = gains[0][None, None, :] * f32[0]
    for g in range(1, 5):
        acc = acc + gains[g][None, None, :] * f32[g]
    assert acc.dtype == np.float32
    got, yard = rel_l2(it.relight(out, gains), ref).max(), rel_l2(acc, ref).max()
    print(f"relight of the shared planes against the filter of the relit planes: GPU {got:.3e}, float32 numpy {yard:.3e}")
    assert got <= MARGIN * yard


# ---- 5. chunk and block edges
def flat_guides(H, W):
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 2.0, 1.0
    return aov


_edges = {}


def edge_case(n):
    if n not in _edges:
        if "it" not in _edges:
            _edges["it"] = integrator(33, 9, 4)
        rng = np.random.default_rng(100 + n)
        planes = rng.uniform(0.0, 2.0, (n, 9, 33, 3)).astype(np.float32)
        if n > 2:
            planes[n - 2] = 0.0
        aov = flat_guides(9, 33)
        aov[:, 17] = 0.0  # a column of miss pixels
        _edges[n] = (_edges["it"], planes, aov)
    return _edges[n]


@pytest.mark.parametrize("n_planes", [1, 7, 2 * CHUNK + 1])
def test_gpu_chunk_and_block_edges(n_planes):
    it, planes, aov = edge_case(n_planes)
    kw = dict(iterations=4, demodulate=True, **SIGMAS)
    own = it.denoise_planes(planes, aov, "own", **kw)
    for j in range(n_planes):
        assert np.array_equal(own[j].view(np.uint32), it.denoise(planes[j], aov, **kw).view(np.uint32)), j
    shared, _ = check_shared_against_the_formula(it, planes, aov, 1, **kw)
    if n_planes > 2:
        for out in (own, shared):
            assert not out[n_planes - 2].view(np.uint32).any()  # all-zero bits
            assert out[n_planes - 1].any()


def test_gpu_own_mode_past_the_chunk_threshold():
    """Frames of more than 512 x 512 pixels take OWN mode plane by plane: the same bits."""
    W, H = 520, 505  # 262 600 pixels, no multiple of the 32 x 8 block
    it = integrator(W, H, 4)
    rng = np.random.default_rng(7)
    planes = rng.uniform(0.0, 2.0, (2, H, W, 3)).astype(np.float32)
    aov = flat_guides(H, W)
    aov[:, 300] = 0.0
    kw = dict(iterations=2, demodulate=True, **SIGMAS)
    own = it.denoise_planes(planes, aov, "own", **kw)
    assert it.stats()["launches"] == 2 * 3
    for j in range(2):
        assert np.array_equal(own[j].view(np.uint32), it.denoise(planes[j], aov, **kw).view(np.uint32)), j


def test_gpu_leading_axes_are_kept():
    it, planes, aov = edge_case(7)
    six = planes[:6].reshape(2, 3, 9, 33, 3)
    for mode in ("own", "shared"):
        out = it.denoise_planes(six, aov, mode, iterations=2)
        assert out.shape == six.shape
        assert np.array_equal(out.reshape(6, 9, 33, 3), it.denoise_planes(planes[:6], aov, mode, iterations=2))


# ---- 6. determinism, the device form, no iterations
def test_gpu_planes_filter_is_deterministic_and_device_equals_host():
    import torch

    it, planes, aov = groups()
    n = planes.shape[0]
    dev = torch.device("cuda", 0)
    tp, ta = torch.from_numpy(planes).to(dev), torch.from_numpy(aov).to(dev)
    for mode in ("own", "shared"):
        want_guide = mode == "shared"
        a = it.denoise_planes(planes, aov, mode, return_guide=want_guide)
        st = it.stats()
        assert st["kernel_ms"] > 0 and 0 < st["launches"] < 6 * n  # fewer than n single-plane calls
        b = it.denoise_planes(planes, aov, mode, return_guide=want_guide)
        a, b = (a, b) if want_guide else ((a,), (b,))
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        tout, tg = torch.zeros_like(tp), torch.zeros((32, 32, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        it.denoise_planes_device(tp.data_ptr(), n, ta.data_ptr(), tout.data_ptr(), mode,
                                 out_guide_ptr=tg.data_ptr() if want_guide else 0)
        it.synchronize()
        assert np.array_equal(tout.cpu().numpy().view(np.uint32), a[0].view(np.uint32))
        if want_guide:
            assert np.array_equal(tg.cpu().numpy().view(np.uint32), a[1].view(np.uint32))


def test_gpu_zero_iterations_scale_the_planes_and_the_guide():
    it, planes, aov = layers(2)
    two = np.float32(2)
    assert np.array_equal(it.denoise_planes(planes, aov, "own", samples_done=2, iterations=0), planes * two)
    out, og = it.denoise_planes(planes, aov, "shared", samples_done=2, iterations=0, return_guide=True)
    assert np.array_equal(out, planes * two) and np.array_equal(og, float_sum(planes) * two)
    mine = other_guide(planes)
    out, og = it.denoise_planes(planes, aov, "shared", guide=mine, iterations=0, return_guide=True)
    assert np.array_equal(out, planes) and np.array_equal(og, mine)
    many = np.concatenate([planes] * 14)  # 70 planes: past the 64 a layer mask names
    out, og = it.denoise_planes(many, aov, "shared", iterations=0, return_guide=True)
    assert np.array_equal(out, many) and np.array_equal(og, float_sum(many))


# ---- 7. refusals
def test_gpu_planes_filter_refusals():
    it, planes, aov = layers(1)
    it.denoise_planes(planes, aov, "own", iterations=1)
    before = it.stats()["launches"]

    def refused(*words, **kw):
        args = dict(planes=planes, aov=aov, mode="shared")
        args.update(kw)
        with pytest.raises(bdpt_amd.BdptError) as e:
            it.denoise_planes(**args)
        assert e.value.code == bdpt_amd.ERR_INVALID, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    refused("iterations", iterations=9)
    refused("iterations", iterations=-1)
    refused("sigma_color", sigma_color=0.0)
    refused("sigma_normal", sigma_normal=-1.0)
    refused("sigma_depth", sigma_depth=float("nan"))
    refused("n_planes", planes=planes[:0])
    refused("mode", mode=2)
    refused("mode", mode=-1)
    refused("guide_color", "OWN", mode="own", guide=planes[0])
    refused("out_guide", "OWN", mode="own", return_guide=True)

    L = bdpt_amd.lib()
    px = 40 * 28
    d = bdpt_amd.DenoiseSettings().c(1.0)
    host = L.bdpt_denoise_planes_host
    out = np.zeros_like(planes)
    og = np.zeros((28, 40, 3), np.float32)
    guide = planes[0].copy()
    SHARED, OWN = bdpt_amd.DENOISE_PLANES_SHARED, bdpt_amd.DENOISE_PLANES_OWN

    def raw(word, n=5, p=planes, a=aov, g=None, mode=SHARED, params=d, o=out, o2=None, shift=0):
        rc = host(it._h, 40, 28, n, p.ctypes.data, a.ctypes.data, None if g is None else g.ctypes.data, mode,
                  ctypes.byref(params), o.ctypes.data + shift, None if o2 is None else o2)
        assert rc == bdpt_amd.ERR_INVALID and word in L.bdpt_last_error(), (word, L.bdpt_last_error())

    raw(b"norm", params=bdpt_amd.DenoiseSettings().c(0.0))
    raw(b"demodulate", params=bdpt_amd._DenoiseParams(5, 2.0, 0.3, 0.02, 2, 1.0))
    raw(b"n_planes", n=0)
    raw(b"2^30", n=(1 << 30) // px + 1)  # (refused before any buffer is read)
    raw(b"out_planes overlaps planes", o=planes)
    raw(b"out_planes overlaps planes", o=planes, shift=4 * (5 * px * 3 - 1))  # the last float
    raw(b"out_planes overlaps aov", o=aov, n=1)
    raw(b"out_planes overlaps guide_color", o=guide, g=guide, n=1)
    raw(b"out_guide overlaps planes", o2=planes.ctypes.data + 4 * px * 3)
    raw(b"out_guide overlaps aov", o2=aov.ctypes.data)
    raw(b"out_guide overlaps guide_color", g=guide, o2=guide.ctypes.data)
    raw(b"out_guide overlaps out_planes", o2=out.ctypes.data + 4 * 4 * px * 3)
    raw(b"guide_color", mode=OWN, g=guide)
    raw(b"out_guide", mode=OWN, o2=og.ctypes.data)
    dev = L.bdpt_denoise_planes  # the device form checks the same, before anything is launched
    assert dev(it._h, 40, 28, 5, planes.ctypes.data, aov.ctypes.data, None, SHARED, ctypes.byref(d), planes.ctypes.data,
               None, None) == bdpt_amd.ERR_INVALID
    assert b"out_planes overlaps planes" in L.bdpt_last_error()
    assert it.stats()["launches"] == before, "a refused call launched"


# ---- 8. the command line
def half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def test_gpu_cli_writes_the_denoised_planes(tmp_path):
    it, planes, aov = groups()
    W, H, spp = it.config.width, it.config.height, it.config.spp
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    (tmp_path / "scene.toml").write_text(variants.toml_text("emit_edges", W, H, spp, it.config.rr_depth))
    r = subprocess.run([cli, str(tmp_path / "scene.toml"), "--light-groups", "--denoise-planes"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = [f"scene.E{e:02d}" for e in range(5)]
    assert sorted(os.listdir(tmp_path)) == sorted(["scene.toml", "scene.exr", "scene_denoised.exr"] +
                                                  [n + ".exr" for n in names] + [n + "_denoised.exr" for n in names])
    api, api_guide = it.denoise_planes(planes, aov, "shared", return_guide=True)
    # the filter is deterministic, but two renders of the planes differ by the order of their atomic
    # additions (as every frame does): one half-precision ulp, as tests/test_gpu_aov_cli.py allows
    for e, n in enumerate(names):
        den = decode_exr((tmp_path / (n + "_denoised.exr")).read_bytes()).astype(np.float32)
        assert np.allclose(den, half(api[e]), rtol=2 ** -9, atol=1e-6), e
        raw = decode_exr((tmp_path / (n + ".exr")).read_bytes()).astype(np.float32)
        assert np.allclose(raw, half(planes[e]), rtol=2 ** -9, atol=1e-6), e
        assert np.abs(den - raw).max() > 0  # it is not the unfiltered plane
    den = decode_exr((tmp_path / "scene_denoised.exr").read_bytes()).astype(np.float32)
    assert np.allclose(den, half(api_guide), rtol=2 ** -9, atol=1e-6)
