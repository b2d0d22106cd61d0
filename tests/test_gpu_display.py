"""bdpt_display and bdpt_meter on the GPU: their bytes and words against display_numpy and meter_numpy (the
float32 restatements of the header's formulas) on synthetic frames - the edge image that holds every threshold
and its neighbours, tiny and odd shapes, shapes past one sweep of the capped grids on the scalar and on the
vector path, misaligned views, flat and empty frames - then the chain on the device, a rendered HardLight frame,
the command line's files, the refusals' messages and the stats."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import bdpt_amd
import display_cases as dc
import sweep_cases as sw
import variants
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
f32 = np.float32
HL = variants.SCENES["hardlight"]
DEV = "cuda:0"

_it = None


def integrator():
    """One context for every synthetic case: the display entries take the frame size per call."""
    global _it
    if _it is None:
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**HL["camera"]), width=40, height=28, spp=4, rr_depth=HL["rr_depth"])
        _it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    return _it


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words_of(t):
    return t.cpu().numpy().view(np.uint32)


def shown(img, s, **kw):
    return integrator().display(up(img), settings=s, **kw).cpu().numpy()


# ---------------------------------------------------------------- display
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("encode", dc.ENCODES)
@pytest.mark.parametrize("tone", dc.TONES)
def test_gpu_display_has_the_bytes_of_the_formula_on_the_edge_image(tone, encode, channels):
    img = dc.edge_image(encode)
    s = bdpt_amd.DisplaySettings(exposure=1.0, white=1.5, tone=tone, encode=encode, channels=channels)
    got = shown(img, s)
    want = bdpt_amd.display_numpy(img, dc.thresholds(encode), s)
    assert got.shape == want.shape == (dc.EDGE_H, dc.EDGE_W, channels) and np.array_equal(got, want)
    if tone == "clamp":  # every edge value reaches the search as it is (tests/test_display_cpu.py)
        assert np.array_equal(np.unique(got[..., :3]), np.arange(256))


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
@pytest.mark.parametrize("channels", [3, 4])
def test_gpu_display_tiny_frames(H, W, channels):
    img = dc.frame(20 + H, H, W)
    for tone in dc.TONES:
        s = bdpt_amd.DisplaySettings(exposure=0.7, white=1.2, tone=tone, channels=channels)
        assert np.array_equal(shown(img, s, norm=1.5), bdpt_amd.display_numpy(img, dc.thresholds("srgb"), s, norm=1.5))


def misaligned(img, channels):
    """The frame as a view one float into its buffer and an output view one byte into its: no 16-byte loads, no
    dword stores."""
    flat = torch.zeros(img.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = up(img).reshape(-1)
    H, W = img.shape[:2]
    out = torch.zeros(H * W * channels + 1, dtype=torch.uint8, device=DEV)
    return flat[1:].view(H, W, 3), out[1:].view(H, W, channels)


@pytest.mark.parametrize("channels", [3, 4])
def test_gpu_display_scalar_path_gives_the_same_bytes(channels):
    img = dc.edge_image("srgb")
    s = bdpt_amd.DisplaySettings(exposure=1.3, white=2.0, tone="reinhard", channels=channels)
    src, dst = misaligned(img, channels)
    assert src.data_ptr() % 16 == 4 and dst.data_ptr() % 4 == 1
    got = integrator().display(src, settings=s, out=dst).cpu().numpy()
    assert np.array_equal(got, shown(img, s)) and np.array_equal(got, bdpt_amd.display_numpy(img, dc.thresholds("srgb"), s))


def test_gpu_display_past_one_sweep_on_the_scalar_path():
    """1025^2 pixels, an odd count beyond the 4096 x 256 lanes of one sweep, through the misaligned views."""
    H, W = sw.PIXEL1
    img = dc.frame(31, H, W)
    s = bdpt_amd.DisplaySettings(exposure=0.8, white=1.5, tone="filmic", encode="gamma22")
    src, dst = misaligned(img, 3)
    got = integrator().display(src, settings=s, out=dst).cpu().numpy()
    assert np.array_equal(got, bdpt_amd.display_numpy(img, dc.thresholds("gamma22"), s))


def test_gpu_display_past_one_sweep_on_the_vector_path():
    """2052 x 2048 pixels: 1 050 624 units of 4 pixels, beyond one sweep of units."""
    H, W = sw.PIXEL4
    img = dc.frame(32, H, W)
    s = bdpt_amd.DisplaySettings(exposure=0.8, white=1.5, tone="reinhard")
    t = up(img)
    assert t.data_ptr() % 16 == 0
    got = integrator().display(t, settings=s).cpu().numpy()
    assert np.array_equal(got, bdpt_amd.display_numpy(img, dc.thresholds("srgb"), s))


def test_gpu_display_vector_path_with_pixels_left_over():
    """1025^2 aligned: 262 656 units and one pixel left over."""
    H, W = sw.PIXEL1
    img = dc.frame(33, H, W)
    s = bdpt_amd.DisplaySettings(exposure=1.1, tone="clamp", encode="linear")
    assert np.array_equal(shown(img, s), bdpt_amd.display_numpy(img, dc.thresholds("linear"), s))


# ---------------------------------------------------------------- meter
def metered(color, aov=None, prev=None, settings=None, norm=1.0):
    it = integrator()
    w = words_of(it.meter(up(color), None if aov is None else up(aov), None if prev is None else up(prev.view(np.int32)),
                          settings, norm))
    return w, it.meter_histogram()


@pytest.mark.parametrize("H,W", [(dc.EDGE_H, dc.EDGE_W), sw.UNIT1, sw.PIXEL4])
def test_gpu_meter_has_the_words_and_the_histogram_of_the_formula(H, W):
    """One block (851 pixels), 86 blocks, and 1024 blocks of more than one sweep each; with and without the
    feature buffers, with an earlier call's words, and twice."""
    color, aov = dc.frame(50 + H, H, W), dc.guides(51 + H, H, W)
    s = bdpt_amd.MeterSettings(key=0.2, key_permille=400, white_permille=950, rate=0.3)
    first = None
    for a in (None, aov):
        w, hist = metered(color, a, None, s, norm=1.25)
        assert np.array_equal(hist, bdpt_amd.meter_histogram_numpy(color, a, 1.25))
        assert np.array_equal(w, bdpt_amd.meter_numpy(color, a, s, None, 1.25)) and w[2] > H * W // 4
        first = w
    again, _ = metered(color, aov, None, s, norm=1.25)
    assert np.array_equal(again, first)
    prev = np.array([3.0, 9.0], f32).view(np.uint32).tolist() + [77, 0]
    prev = np.array(prev, np.uint32)
    w, _ = metered(color, aov, prev, s, norm=1.25)
    assert np.array_equal(w, bdpt_amd.meter_numpy(color, aov, s, prev, 1.25)) and w[0] != first[0]


def test_gpu_meter_all_zero_frame_returns_the_fallbacks():
    s = bdpt_amd.MeterSettings(fallback_exposure=2.5, fallback_white=7.0)
    w, hist = metered(np.zeros((dc.EDGE_H, dc.EDGE_W, 3), f32), None, None, s)
    assert not hist.any() and np.array_equal(w, bdpt_amd.meter_numpy(np.zeros((2, 2, 3), f32), None, s))
    assert w[:2].view(f32).tolist() == [2.5, 7.0]


def test_gpu_meter_constant_frame_puts_every_lane_in_one_bin():
    H, W = sw.PIXEL4
    color = dc.constant_frame(H, W)
    w, hist = metered(color)
    assert np.array_equal(hist, bdpt_amd.meter_histogram_numpy(color)) and hist.max() == H * W
    assert np.array_equal(w, bdpt_amd.meter_numpy(color))
    # half of each wave in another bin: the waves are no longer uniform
    color[:, 1::2] = f32(0.5)
    w, hist = metered(color)
    assert np.array_equal(hist, bdpt_amd.meter_histogram_numpy(color)) and np.count_nonzero(hist) == 2
    assert np.array_equal(w, bdpt_amd.meter_numpy(color))


# ---------------------------------------------------------------- chain
def test_gpu_display_auto_chains_meter_and_display_on_the_device():
    H, W = dc.EDGE_H, dc.EDGE_W
    color, aov = dc.frame(60, H, W), dc.guides(61, H, W)
    it = integrator()
    for tone in dc.TONES:
        s = bdpt_amd.DisplaySettings(tone=tone, channels=4)
        m = bdpt_amd.MeterSettings(key=0.3)
        got = it.display(up(color), exposure="auto", aov=up(aov), settings=s, meter_settings=m).cpu().numpy()
        words = bdpt_amd.meter_numpy(color, aov, m)
        assert np.array_equal(got, bdpt_amd.display_numpy(color, dc.thresholds("srgb"), s, meter=words))
    assert len(np.unique(got)) > 100
    # and on a stream of torch's own: the two launches are ordered with the upload and the read-back by the stream
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        again = it.display(up(color), exposure="auto", aov=up(aov), settings=s, meter_settings=m).cpu().numpy()
    assert np.array_equal(again, got)


# ---------------------------------------------------------------- rendered
def hardlight(spp=4):
    it = integrator()
    it.config.camera, it.config.spp = bdpt_amd.Camera(**HL["camera"]), spp
    it.init()
    return it


def test_gpu_display_of_a_rendered_frame():
    it = hardlight()
    rgb = it.render_frame().reshape(28, 40, 3).copy()
    aov = it.render_aov().reshape(28, 40, 8).copy()
    s, m = bdpt_amd.DisplaySettings(), bdpt_amd.MeterSettings()
    got = it.display(up(rgb), exposure="auto", aov=up(aov), settings=s, meter_settings=m).cpu().numpy()
    words = bdpt_amd.meter_numpy(rgb, aov, m)
    assert np.array_equal(got, bdpt_amd.display_numpy(rgb, dc.thresholds("srgb"), s, meter=words))
    # an exposed frame: the median code away from both ends, and the lamp at the top of the range
    assert 40 < np.median(got) < 215 and got.max() == 255 and words[2] > 28 * 40 // 2


def run_cli(d, *args):
    toml = d / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 40, 28, 4))
    r = subprocess.run([CLI, str(toml)] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_command_line_display_png_shows_the_frame_of_its_exr(tmp_path):
    """The PNG decodes to display(exposure="auto") of the frame the command rendered. The EXR holds that frame
    as half floats, so the frame itself is rendered again here with the command's parameters and tied to the
    command's EXR by its bytes; the EXR is the same file with and without --display."""
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir(), b.mkdir()
    run_cli(a, "--display=png", "--tone", "filmic")
    run_cli(b)
    assert sorted(os.listdir(a)) == ["scene.exr", "scene.png", "scene.toml"]
    exr = (a / "scene.exr").read_bytes()
    assert exr == (b / "scene.exr").read_bytes()
    it = hardlight()
    rgb = it.render_frame().reshape(28, 40, 3).copy()
    assert bdpt_amd.encode_exr(rgb, 40, 28) == exr
    want = it.display(up(rgb), exposure="auto", settings=bdpt_amd.DisplaySettings(tone="filmic")).cpu().numpy()
    assert np.array_equal(dc.decode_png((a / "scene.png").read_bytes()), want)
    # and a fixed exposure as a PPM, with the filter's frame
    c = tmp_path / "ppm"
    c.mkdir()
    run_cli(c, "--display=ppm", "--exposure", "1", "--denoise", "--encode", "gamma22")
    aov = it.render_aov()
    den = it.denoise(rgb, aov)
    s = bdpt_amd.DisplaySettings(exposure=2.0, encode="gamma22")
    want = it.display(up(den), settings=s).cpu().numpy()
    assert (c / "scene.ppm").read_bytes() == b"P6\n40 28\n255\n" + want.tobytes()


def test_command_line_temporal_display_equals_render_sequence(tmp_path):
    eye, at = HL["camera"]["eye"], HL["camera"]["at"]
    cams = [bdpt_amd.Camera(eye=(eye[0] + 0.02 * k, eye[1], eye[2]), at=(at[0] + 0.02 * k, at[1], at[2]),
                            up=HL["camera"]["up"], fov=HL["camera"]["fov"]) for k in range(3)]
    text = "".join(" ".join(repr(float(v)) for v in (*c.eye, *c.at, *c.up, c.fov)) + "\n" for c in cams)
    (tmp_path / "cams.txt").write_text(text)
    run_cli(tmp_path, "--cameras", str(tmp_path / "cams.txt"), "--temporal", "--display", "--exposure", "auto:0.25:0.5")
    it = hardlight()
    frames = list(it.render_sequence(cams, display=bdpt_amd.DisplaySettings(), meter=bdpt_amd.MeterSettings(key=0.25, rate=0.5)))
    assert len(frames) == 3
    for f, (acc, img) in enumerate(frames):
        assert (tmp_path / f"scene.f{f:02d}.exr").read_bytes() == bdpt_amd.encode_exr(acc, 40, 28)
        assert np.array_equal(dc.decode_png((tmp_path / f"scene.f{f:02d}.png").read_bytes()), img), f


# ---------------------------------------------------------------- refusals and stats
def test_gpu_display_and_meter_refusals_name_the_field():
    it = integrator()
    color = up(dc.frame(70, 4, 6, specials=False))
    out = torch.zeros(4 * 6 * 4, dtype=torch.uint8, device=DEV)
    words = torch.zeros(4, dtype=torch.int32, device=DEV)
    D, M = bdpt_amd.DisplaySettings, bdpt_amd.MeterSettings
    for s, word in ((D(exposure=0.0), "exposure"), (D(white=-1.0), "white"), (D(tone=3), "tone"), (D(encode=5), "encode"),
                    (D(channels=2), "channels"), (D(exposure=float("nan")), "exposure")):
        with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: .*" + word) as e:
            it.display_device(color.data_ptr(), out.data_ptr(), 0, 6, 4, settings=s)
        assert e.value.code == bdpt_amd.ERR_INVALID
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: .*norm"):
        it.display_device(color.data_ptr(), out.data_ptr(), 0, 6, 4, norm=0.0)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: color"):
        it.display_device(0, out.data_ptr(), 0, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: out must"):
        it.display_device(color.data_ptr(), 0, 0, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: out overlaps color"):
        it.display_device(color.data_ptr(), color.data_ptr() + 8, 0, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: out overlaps meter"):
        it.display_device(color.data_ptr(), out.data_ptr(), out.data_ptr() + 4, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_display: .*2\\^28"):
        it.display_device(color.data_ptr(), out.data_ptr(), 0, 1 << 14, 1 << 14)
    for s, word in ((M(key=0.0), "key"), (M(key_permille=0), "key_permille"), (M(white_permille=1001), "white_permille"),
                    (M(rate=0.0), "rate"), (M(rate=1.5), "rate"), (M(fallback_exposure=0.0), "fallback_exposure"),
                    (M(fallback_white=-2.0), "fallback_white")):
        with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: .*" + word) as e:
            it.meter_device(color.data_ptr(), 0, 0, words.data_ptr(), 6, 4, settings=s)
        assert e.value.code == bdpt_amd.ERR_INVALID
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: .*norm"):
        it.meter_device(color.data_ptr(), 0, 0, words.data_ptr(), 6, 4, norm=-1.0)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: color"):
        it.meter_device(0, 0, 0, words.data_ptr(), 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: out_words must"):
        it.meter_device(color.data_ptr(), 0, 0, 0, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: out_words overlaps color"):
        it.meter_device(color.data_ptr(), 0, 0, color.data_ptr() + 16, 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: out_words overlaps prev"):
        it.meter_device(color.data_ptr(), 0, words.data_ptr(), words.data_ptr(), 6, 4)
    with pytest.raises(bdpt_amd.BdptError, match="bdpt_meter: .*2\\^28"):
        it.meter_device(color.data_ptr(), 0, 0, words.data_ptr(), 1 << 14, 1 << 14)
    torch.cuda.synchronize()


def test_gpu_display_and_meter_set_the_stats():
    it = integrator()
    color = up(dc.frame(71, 64, 64, specials=False))
    it.meter(color)
    it.synchronize()
    st = it.stats()
    assert st["launches"] == 2 and st["kernel_ms"] > 0 and st["samples"] == 0
    it.display(color)
    it.synchronize()
    st = it.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0


def test_host_forms_equal_the_device_forms():
    """bdpt_meter_host and bdpt_display_host (what the command line calls) on host arrays."""
    it = integrator()
    H, W = dc.EDGE_H, dc.EDGE_W
    color, aov = dc.frame(80, H, W), dc.guides(81, H, W)
    m = bdpt_amd.MeterSettings().c(1.0)
    words = np.zeros(4, np.uint32)
    bdpt_amd._check(bdpt_amd.lib().bdpt_meter_host(it._h, W, H, color.ctypes.data, aov.ctypes.data, None, ctypes.byref(m),
                                                   words.ctypes.data))
    assert np.array_equal(words, bdpt_amd.meter_numpy(color, aov))
    d = bdpt_amd.DisplaySettings(channels=4).c(1.0)
    out = np.zeros((H, W, 4), np.uint8)
    bdpt_amd._check(bdpt_amd.lib().bdpt_display_host(it._h, W, H, color.ctypes.data, words.ctypes.data, ctypes.byref(d),
                                                     out.ctypes.data))
    assert np.array_equal(out, bdpt_amd.display_numpy(color, dc.thresholds("srgb"), bdpt_amd.DisplaySettings(channels=4), meter=words))
