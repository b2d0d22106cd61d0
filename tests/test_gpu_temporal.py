"""bdpt_reproject on the GPU: its bits against reproject_numpy (the float32 restatement of the header's
formula) on synthetic buffers - odd shapes, tiny frames, a shape past one sweep of the capped grid - and on
a rendered HardLight pair of cameras, where the accumulated frame must also beat the 4-spp frame against
256 spp; the refusals' messages, the stats, and the command line's camera sequence."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bdpt_amd
import sweep_cases as sw
import temporal_cases as tc
import variants
from conftest import gpu_available
from test_config_exr import decode_exr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
f32 = np.float32
HL = variants.SCENES["hardlight"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


_integrators = {}


def integrator(W, H, spp=4, cam=None):
    """One context per frame size; the camera and spp are set per use."""
    if (W, H) not in _integrators:
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**HL["camera"]), width=W, height=H, spp=spp, rr_depth=HL["rr_depth"])
        _integrators[(W, H)] = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("hardlight")), cfg)
    it = _integrators[(W, H)]
    it.config.camera = cam or bdpt_amd.Camera(**HL["camera"])
    it.config.spp = spp
    it.init()
    return it


def synthetic(W, H, seed, extremes=True):
    """Colour and feature buffers of the synthetic scene at cameras A and B, with sprinkle's zeros, 1e-20 and
    1e6 over all of them (so some pixels turn into misses and some depths into 1e6)."""
    aovA, _, _, cA = tc.buffers(tc.CAM_A, W, H)
    aovB, _, _, cB = tc.buffers(tc.CAM_B, W, H)
    cols = tc.colours(seed, W, H, 2)
    if extremes:
        for k, a in enumerate((aovA, aovB, cols[0], cols[1])):
            sw.sprinkle(a.reshape(-1)[k:])  # (a view: other floats in each)
    return (aovA, cA), (aovB, cB), cols


def two_steps(it, W, H, seed, settings, cams=(tc.CAM_A, tc.CAM_B), n_c=4.0):
    """History made at cams[0] with no history, carried to cams[1]: the GPU's (out, hist) and the restatement's,
    both on the GPU's own first history and the device's own ray directions."""
    (aovA, _), (aovB, _), cols = synthetic(W, H, seed)
    if cams[0] is cams[1]:
        aovB = aovA
    cA, cB = (bdpt_amd.camera_constants(c, W, H) for c in cams)
    it.config.camera, it.config.spp = cams[0], int(n_c)
    dirsA = it.primary_directions()
    g0 = it.reproject(cams[0], None, cols[0], aovA, settings=settings)
    n0 = bdpt_amd.reproject_numpy(cols[0], aovA, None, dirsA, cA, cA, settings, cur_samples=n_c)
    it.config.camera = cams[1]
    dirsB = it.primary_directions()
    g1 = it.reproject(cams[0], g0[1], cols[1], aovB, settings=settings)
    n1 = bdpt_amd.reproject_numpy(cols[1], aovB, g0[1], dirsB, cB, cA, settings, cur_samples=n_c)
    return (g0, n0), (g1, n1)


@pytest.mark.parametrize("clamp", [0.0, 1.5])
@pytest.mark.parametrize("demodulate", [False, True])
def test_gpu_reproject_has_the_bits_of_the_formula(demodulate, clamp):
    """37 x 23 (no multiple of the block or of 4), a pan plus a dolly, extremes sprinkled in. The acceptance is the
    test's own, wide enough that at this size, with a third of the floats extreme, over 100 pixels find history
    (counted with the restatement on the host) and far more than 10 covered ones do not."""
    W, H = 37, 23
    s = bdpt_amd.ReprojectSettings(demodulate=demodulate, clamp_sigma=clamp, sigma_depth=0.2, sigma_normal=0.5, min_weight=0.1)
    (g0, n0), (g1, n1) = two_steps(integrator(W, H), W, H, 11, s)
    assert same_bits(g0, n0)  # hist_in NULL
    assert same_bits(g1, n1)
    n = g1[1][..., 3]
    assert (n > 4).sum() > 100 and ((n == 4) & (g1[1][..., 7] > 0)).sum() > 10  # both branches ran


def test_gpu_reproject_identical_cameras_land_on_their_own_pixel():
    W, H = 37, 23
    s = bdpt_amd.ReprojectSettings(demodulate=False, clamp_sigma=0.0)
    (g0, n0), (g1, n1) = two_steps(integrator(W, H), W, H, 12, s, cams=(tc.CAM_A, tc.CAM_A))
    assert same_bits(g0, n0) and same_bits(g1, n1)
    # where the sprinkled extremes left a plain hit, the count doubles
    plain = (g0[1][..., 7] >= 1) & (g0[1][..., 7] < 100) & (np.abs(g0[1][..., 4:7]).max(-1) <= 1)
    assert plain.sum() > 200 and np.array_equal(g1[1][plain][:, 3], np.full(plain.sum(), 8.0, f32))


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3)])
def test_gpu_reproject_tiny_frames_project_outside_on_every_side(W, H):
    """A 1 x 1 and a 5 x 3 frame under a turn of the camera to the left, right, up and down (about a pixel of the
    5 x 3 frame): history projects outside the image on every side, and taps straddle its border."""
    s = bdpt_amd.ReprojectSettings(demodulate=True, clamp_sigma=1.5, sigma_depth=0.5)
    it = integrator(W, H)
    moves = [(0.0, 0.0)] + [(dx, dy) for dx, dy in ((-1.2, 0), (1.2, 0), (0, 0.9), (0, -0.9), (0.15, 0.1))]
    kept = []
    for dx, dy in moves:
        at = (tc.CAM_A.at[0] + dx, tc.CAM_A.at[1] + dy, tc.CAM_A.at[2])
        camB = bdpt_amd.Camera(eye=tc.CAM_A.eye, at=at, up=tc.CAM_A.up, fov=tc.CAM_A.fov)
        aovA, _, _, cA = tc.buffers(tc.CAM_A, W, H)
        aovB, _, _, cB = tc.buffers(camB, W, H)
        cols = tc.colours(13, W, H, 2)
        it.config.camera = tc.CAM_A
        g0 = it.reproject(tc.CAM_A, None, cols[0], aovA, settings=s)
        it.config.camera = camB
        dirs = it.primary_directions()
        g1 = it.reproject(tc.CAM_A, g0[1], cols[1], aovB, settings=s)
        n1 = bdpt_amd.reproject_numpy(cols[1], aovB, g0[1], dirs, cB, cA, s, cur_samples=4.0)
        assert same_bits(g1, n1), (dx, dy)
        kept.append(int((g1[1][..., 3] > 4).sum()))
    assert kept[0] > 0 and max(kept) <= kept[0], kept
    if (W, H) == (5, 3):  # a turn by about a pixel: a column or a row of history is lost
        assert max(kept[1:5]) < kept[0], kept


def test_gpu_reproject_past_one_grid_sweep():
    """1025 x 1025: more pixels than the 4096 x 256 lanes of one sweep, an odd count."""
    H, W = sw.PIXEL1
    assert H * W > sw.SWEEP
    s = bdpt_amd.ReprojectSettings(demodulate=True, clamp_sigma=1.5)
    (g0, n0), (g1, n1) = two_steps(integrator(W, H), W, H, 14, s)
    assert same_bits(g0, n0)
    assert same_bits(g1, n1)
    assert (g1[1][-1, :, 3] > 4).any()  # the last row, which only a later sweep reaches, found history


def hardlight_camera(shift):
    """The HardLight camera with eye and at moved sideways by `shift` of the eye-at distance."""
    cam = HL["camera"]
    eye, at = np.asarray(cam["eye"], np.float64), np.asarray(cam["at"], np.float64)
    fwd = at - eye
    side = np.cross(fwd, np.asarray(cam["up"], np.float64))
    move = side / np.linalg.norm(side) * np.linalg.norm(fwd) * shift
    return bdpt_amd.Camera(eye=tuple(eye + move), at=tuple(at + move), up=tuple(cam["up"]), fov=cam["fov"])


@pytest.fixture(scope="module")
def rendered():
    """HardLight 40 x 28 at 4 spp: camera A, then camera B = A moved sideways by 2 % of the eye-at distance, each
    frame with its feature buffers and its own seeds; and B's 256-spp frame."""
    W, H = 40, 28
    camA, camB = hardlight_camera(0.0), hardlight_camera(0.02)
    it = integrator(W, H, 4, camA)
    rgbA, aovA = it.render_frame().copy(), it.render_aov().copy()
    it = integrator(W, H, 4, camB)
    it.config.seed_base = bdpt_amd.REFERENCE_SEED + W * H * 4
    rgbB, aovB = it.render_frame().copy(), it.render_aov().copy()
    dirsB = it.primary_directions()
    it.config.seed_base = bdpt_amd.REFERENCE_SEED
    ref = integrator(W, H, 256, camB).render_frame().astype(np.float64)
    return dict(W=W, H=H, camA=camA, camB=camB, rgbA=rgbA, aovA=aovA, rgbB=rgbB, aovB=aovB, dirsB=dirsB, ref=ref)


@pytest.mark.parametrize("clamp", [None, 0.0])
def test_gpu_reproject_rendered_pair(rendered, clamp):
    """(a) the bits of the restatement on the rendered inputs; (b) at least half of the covered pixels get
    history under the default sigmas; (c) over the pixels with history the accumulated frame is closer to the
    256-spp frame than the 4-spp frame is, with the default clamp and without one; (d) two runs, same bits.
    Measured on an MI355X (938 of 1038 covered pixels with history; mean squared error over them): 4-spp frame
    0.002074, accumulated 0.000735 with the defaults, 0.000737 with clamp_sigma 0."""
    r = rendered
    W, H = r["W"], r["H"]
    s = bdpt_amd.ReprojectSettings() if clamp is None else bdpt_amd.ReprojectSettings(clamp_sigma=clamp)
    it = integrator(W, H, 4, r["camA"])
    _, histA = it.reproject(r["camA"], None, r["rgbA"], r["aovA"], settings=s)
    it = integrator(W, H, 4, r["camB"])
    got = it.reproject(r["camA"], histA, r["rgbB"], r["aovB"], settings=s)
    cA, cB = (bdpt_amd.camera_constants(c, W, H) for c in (r["camA"], r["camB"]))
    want = bdpt_amd.reproject_numpy(r["rgbB"], r["aovB"], histA, r["dirsB"], cB, cA, s, cur_samples=4.0)
    assert same_bits(got, want)
    covered = r["aovB"][..., 7] > 0
    has = got[1][..., 3] > 4
    print(f"covered {covered.sum()}, with history {has.sum()}")
    assert has.sum() * 2 >= covered.sum()
    e_acc = np.mean((got[0][has] - r["ref"][has]) ** 2)
    e_cur = np.mean((r["rgbB"][has] - r["ref"][has]) ** 2)
    print(f"MSE against 256 spp over the pixels with history: 4-spp frame {e_cur:.6g}, accumulated {e_acc:.6g} "
          f"(clamp_sigma {s.clamp_sigma})")
    assert e_acc < e_cur
    again = it.reproject(r["camA"], histA, r["rgbB"], r["aovB"], settings=s)
    assert same_bits(got, again)


def test_gpu_reproject_device_entry_equals_host_and_counts_one_launch():
    import torch

    W, H = 37, 23
    (aovA, _), (aovB, _), cols = synthetic(W, H, 15)
    it = integrator(W, H, 4, tc.CAM_A)
    s = bdpt_amd.ReprojectSettings()
    _, histA = it.reproject(tc.CAM_A, None, cols[0], aovA, settings=s)
    it.config.camera = tc.CAM_B
    want = it.reproject(tc.CAM_A, histA, cols[1], aovB, settings=s)
    st = it.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0
    dev = "cuda:0"
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(c=cols[1], a=aovB, h=histA).items()}
    out, ho = torch.zeros(H, W, 3, device=dev), torch.zeros(H, W, 8, device=dev)
    torch.cuda.synchronize()  # (torch's stream and the context's are not ordered against each other)
    it.reproject_device(tc.CAM_A, t["c"].data_ptr(), t["a"].data_ptr(), t["h"].data_ptr(), out.data_ptr(), ho.data_ptr(),
                        settings=s)
    it.synchronize()
    assert it.stats()["launches"] == 1
    assert same_bits((out.cpu().numpy(), ho.cpu().numpy()), want)
    # buffers 4 bytes off a 16-byte boundary take the dword path: the same bits
    pad = torch.zeros(1 + H * W * 8, device=dev)
    pad[1:] = t["a"].reshape(-1)
    torch.cuda.synchronize()
    it.reproject_device(tc.CAM_A, t["c"].data_ptr(), pad.data_ptr() + 4, t["h"].data_ptr(), out.data_ptr(), ho.data_ptr(),
                        settings=s)
    it.synchronize()
    assert same_bits((out.cpu().numpy(), ho.cpu().numpy()), want)


def test_gpu_reproject_refusals_name_their_field():
    W, H = 8, 4
    it = integrator(W, H, 4, tc.CAM_A)
    rgb, aov, hist = np.zeros((H, W, 3), f32), np.zeros((H, W, 8), f32), np.zeros((H, W, 8), f32)
    for field, kw in (("max_history", dict(max_history=0.0)), ("sigma_normal", dict(sigma_normal=-1.0)),
                      ("sigma_depth", dict(sigma_depth=float("nan"))), ("min_weight", dict(min_weight=1.5)),
                      ("min_weight", dict(min_weight=0.0)), ("clamp_sigma", dict(clamp_sigma=-0.5))):
        with pytest.raises(bdpt_amd.BdptError, match=field) as e:
            it.reproject(tc.CAM_A, hist, rgb, aov, **kw)
        assert e.value.code == bdpt_amd.ERR_INVALID
    L = bdpt_amd.lib()
    p = it.params()
    out, ho = np.zeros_like(rgb), np.zeros_like(hist)

    def call(r, c=rgb, a=aov, h=hist, o=out, s=ho, params=p):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.bdpt_reproject_host(it._h, ctypes.byref(params), ptr(c), ptr(a), ptr(h), ptr(o), ptr(s), ctypes.byref(r))

    ok = bdpt_amd.ReprojectSettings().c(tc.CAM_A, 4.0)
    assert call(ok) == 0
    for field, r in (("norm", bdpt_amd.ReprojectSettings().c(tc.CAM_A, 4.0, 0.0)),
                     ("cur_samples", bdpt_amd.ReprojectSettings().c(tc.CAM_A, 0.0)),
                     ("demodulate", bdpt_amd._ReprojectParams(tc.CAM_A.c(), 1.0, 4.0, 8.0, 0.3, 0.02, 0.25, 1.5, 2))):
        assert call(r) == bdpt_amd.ERR_INVALID and field.encode() in L.bdpt_last_error(), field
    for word, kw in (("color", dict(c=None)), ("aov", dict(a=None)), ("out_color", dict(o=None)), ("hist_out", dict(s=None)),
                     ("hist_out overlaps hist_in", dict(s=hist)), ("out_color overlaps color", dict(o=rgb)),
                     ("hist_out overlaps aov", dict(s=aov))):
        assert call(ok, **kw) == bdpt_amd.ERR_INVALID and word.encode() in L.bdpt_last_error(), word
    big = it.params()
    big.width, big.height = 1 << 14, 1 << 14
    assert call(ok, params=big) == bdpt_amd.ERR_INVALID and b"2^28" in L.bdpt_last_error()
    both = np.zeros(H * W * 8 + 3, f32)  # the two outputs overlapping each other
    assert L.bdpt_reproject_host(it._h, ctypes.byref(p), rgb.ctypes.data, aov.ctypes.data, None, both.ctypes.data,
                                 both.ctypes.data + 4, ctypes.byref(ok)) == bdpt_amd.ERR_INVALID
    assert b"hist_out overlaps out_color" in L.bdpt_last_error()


def test_gpu_cli_camera_sequence_equals_render_sequence(tmp_path):
    """32 x 32 at 1 spp, three cameras, --temporal --denoise: the six files; frame 0 is the plain render of
    camera 0; frame 2 and its filtered frame are what render_sequence gives."""
    W = H = 32
    cams = [hardlight_camera(s) for s in (0.0, 0.01, 0.02)]
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", W, H, 1))
    lines = ["# eye at up fov", ""] + [" ".join(repr(float(np.float32(v))) for v in (*c.eye, *c.at, *c.up, c.fov)) for c in cams]
    (tmp_path / "cams.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([CLI, str(toml), "--cameras", str(tmp_path / "cams.txt"), "--temporal", "--denoise"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = [f"scene.f{f:02d}{s}.exr" for f in range(3) for s in ("", "_denoised")]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["scene.toml", "cams.txt"])
    read = lambda n: decode_exr((tmp_path / n).read_bytes())  # noqa: E731
    half = lambda a: decode_exr(bdpt_amd.encode_exr(np.ascontiguousarray(a, f32), W, H))  # noqa: E731
    it = integrator(W, H, 1, cams[0])
    assert np.array_equal(read("scene.f00.exr"), half(it.render_frame()))
    it = integrator(W, H, 1, cams[0])
    frames = list(it.render_sequence(cams, 1, denoise=True))
    assert np.array_equal(read("scene.f02.exr"), half(frames[2][0]))
    assert np.array_equal(read("scene.f02_denoised.exr"), half(frames[2][1]))
    assert not np.array_equal(frames[2][0], frames[0][0])
