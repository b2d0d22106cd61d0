"""One context through everything it serves, its refusals, and a refused context.

A context owns the device buffers of every entry (frame renders of the three
integrators, feature buffers, the filter, the per-function and single-sample calls) and
grows them on demand. The tests here run one context through all of them with growing
sizes, on its own stream and on a caller's, and hold every result to what the suite
already pins: the frame goldens at the tolerance of tests/test_gpu_parity.py, the
per-function goldens bit for bit as tests/test_gpu_kat.py does. They also pin which
message each frame entry gives for which bad argument (and which of two), and that a
context the library refuses to create leaves it working.
"""
import ctypes
import os
import shutil
from dataclasses import replace

import numpy as np
import pytest
import torch

import bdpt_amd
import variants
from conftest import load_golden
from test_gpu_kat import kat, same_bits
from test_gpu_parity import TOL, rel_l2

pytestmark = pytest.mark.gpu

# the smallest BDPT golden of the scene within 64x64 at 16 spp
GOLDEN = {"caustic": "G2_caustic_64x64_spp16", "hardlight": "G3_hardlight_64x64_spp16"}
SAMPLER = {"caustic": "kat_sampler_bdpt_caustic", "hardlight": "kat_sampler_bdpt_hardlight_rr12"}
L = bdpt_amd.lib


def context(name, W=16, H=16, spp=2, rr=3):
    cam = bdpt_amd.Camera(**variants.SCENES[name]["camera"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)),
                                 bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=rr))
    it.init()
    return it


def configure(it, W, H, spp, rr):
    it.config = replace(it.config, width=W, height=H, spp=spp, rr_depth=rr)
    it.init()  # zeroed rgb / aov of the new size


class Host:
    """The host entries: every call returns with its result."""

    def frame(self, it, path=None, direct=None):
        p = it.params()
        it.rgb[:] = 0
        if path is not None:
            pp = path.c()
            bdpt_amd._check(L().bdpt_render_path_host(it._h, ctypes.byref(p), ctypes.byref(pp), it.rgb.ctypes.data))
        elif direct is not None:
            dp = direct.c()
            bdpt_amd._check(L().bdpt_render_direct_host(it._h, ctypes.byref(p), ctypes.byref(dp), it.rgb.ctypes.data))
        else:
            it.render_frame()
        out = it.rgb.copy()
        return lambda: out

    def aov(self, it):
        it.aov[:] = 0
        out = it.render_aov().copy()
        return lambda: out

    def denoise(self, it, rgb, aov):
        out = it.denoise(rgb, aov)
        return lambda: out


class OnStream:
    """The device entries on a caller's stream: a call returns at once, its result is
    collected after whatever the test runs on the context in between."""

    def __init__(self):
        self.s = torch.cuda.Stream()

    def _buffer(self, *shape, src=None):
        t = torch.zeros(shape, dtype=torch.float32, device="cuda") if src is None else \
            torch.from_numpy(np.ascontiguousarray(src, np.float32)).cuda()
        torch.cuda.synchronize()  # the buffer is ready before the other stream uses it
        return t

    def _collect(self, t):
        def collect():
            self.s.synchronize()
            return t.cpu().numpy()
        return collect

    def frame(self, it, path=None, direct=None):
        c, p = it.config, it.params()
        fb = self._buffer(c.height, c.width, 3)
        ptr, st = ctypes.c_void_p(fb.data_ptr()), ctypes.c_void_p(self.s.cuda_stream)
        if path is not None:
            pp = path.c()
            bdpt_amd._check(L().bdpt_render_path(it._h, ctypes.byref(p), ctypes.byref(pp), ptr, st))
        elif direct is not None:
            dp = direct.c()
            bdpt_amd._check(L().bdpt_render_direct(it._h, ctypes.byref(p), ctypes.byref(dp), ptr, st))
        else:
            it.render_device(fb.data_ptr(), self.s.cuda_stream)
        return self._collect(fb)

    def aov(self, it):
        c = it.config
        buf = self._buffer(c.height, c.width, 8)
        it.render_aov_device(buf.data_ptr(), self.s.cuda_stream)
        return self._collect(buf)

    def denoise(self, it, rgb, aov):
        c = it.config
        drgb, daov, out = self._buffer(src=rgb), self._buffer(src=aov), self._buffer(c.height, c.width, 3)
        it.denoise_device(drgb.data_ptr(), daov.data_ptr(), out.data_ptr(), self.s.cuda_stream)
        collect = self._collect(out)
        return lambda: (collect(), drgb, daov)[0]  # the inputs live until the result is read


def check_unpinned(it, fb, what):
    """A frame without a golden: finite, and every sample of the frame was rendered."""
    c = it.config
    assert np.all(np.isfinite(fb)), what
    assert it.stats()["samples"] == c.width * c.height * c.spp, what


def check_golden(it, fb, name, manifest):
    assert it.stats()["samples"] == manifest["framebuffers"][name]["samples"]
    worst = rel_l2(fb.reshape(-1), load_golden(name)).max()
    assert np.all(np.isfinite(fb))
    assert worst <= TOL, f"{name}: max per-pixel rel L2 {worst:.3g}"


def check_bsdf_eval(it, scene):
    g = kat(f"kat_bsdf_{scene}")
    live = g["null"] == 0
    f = it.bsdf_eval(g["mat"][live], g["wo"][live], g["wi"][live])
    assert same_bits(f, g["eval"][live]), np.abs(f - g["eval"][live]).max()


def check_intersect(it, scene):
    g = kat(f"kat_intersect_{scene}")
    h, ref = it.intersect(g["rays"]), g["out"]
    assert np.array_equal(h["hit"], ref[:, 0].astype(np.int32))
    k = ref[:, 0] == 1
    assert same_bits(h["t"][k], ref[k, 1]) and same_bits(h["u"][k], ref[k, 2]) and same_bits(h["v"][k], ref[k, 3])
    assert np.array_equal(h["prim_id"][k], ref[k, 5].view(np.int32))
    assert same_bits(h["p"][k], ref[k, 7:10]) and same_bits(h["ns"][k], ref[k, 10:13])


def check_render_ray_sampler(it, scene, i=0):
    """Integrator::render(ray, sampler) at the frame size of the sampler golden."""
    g = kat(SAMPLER[scene])
    configure(it, int(g["width"]), int(g["height"]), int(g["spp"]), int(g["rr"]))
    r = g["rays"][i]
    s = bdpt_amd.Sampler.from_state(g["state_in"][i])
    Li = it.render(bdpt_amd.Ray(tuple(r[:3]), tuple(r[3:6]), float(r[6]), float(r[7])), s)
    assert same_bits(Li, g["Li"][i]), (Li, g["Li"][i])
    assert np.array_equal(s.state, g["state_out"][i])


def run_sequence(scene, via, manifest):
    """Growing demands on one context; `via` issues the frames (Host or OnStream), the
    per-function calls between them are the context's own host entries either way."""
    name = GOLDEN[scene]
    m = manifest["framebuffers"][name]
    W, H, spp, rr = m["width"], m["height"], m["spp"], m["rr_depth"]
    it = context(scene, 16, 16, 2, 3)

    small = via.frame(it)  # 1: a small frame
    check_unpinned(it, small(), "16x16 BDPT")
    small_aov = via.aov(it)()

    configure(it, W, H, spp, rr)  # 2: the golden frame (larger frame buffer, more light vertices)
    golden = via.frame(it)
    check_bsdf_eval(it, scene)  # (runs after the frame in flight on the caller's stream)
    check_golden(it, golden(), name, manifest)

    configure(it, W, H, spp, 29)  # 3: past the lazy MT19937 window: generator rings, the deep build
    deep = via.frame(it)
    assert it.stats()["kernel"] == "bdpt_frame_kernel_deep"
    check_unpinned(it, deep(), "rr_depth 29")

    configure(it, W, H, spp, rr)
    for depth in (2, 6):  # 4: the path tracer's level stacks, then deeper ones
        fb = via.frame(it, path=bdpt_amd.PathSettings(max_depth=depth))
        check_unpinned(it, fb(), f"path max_depth {depth}")
        assert it.stats()["counters"]["shadow_rays"] == 0  # no sample outgrew the level stack
    check_intersect(it, scene)

    fb = via.frame(it, direct=bdpt_amd.DirectSettings(sampling_strategy="mis"))  # 5
    check_render_ray_sampler(it, scene)
    configure(it, W, H, spp, rr)
    check_unpinned(it, fb(), "direct")  # (the single-sample call leaves the frame's stats)

    aov = via.aov(it)  # 6
    assert it.stats()["samples"] == W * H * spp
    aov = aov()
    assert np.all(np.isfinite(aov)) and np.any(aov[..., 7] > 0)

    configure(it, 16, 16, 2, 3)  # 7: the filter, then on a larger frame
    out = via.denoise(it, small(), small_aov)()
    assert out.shape == (16, 16, 3) and np.all(np.isfinite(out))
    configure(it, W, H, spp, rr)
    out = via.denoise(it, golden(), aov)()
    assert out.shape == (H, W, 3) and np.all(np.isfinite(out)) and np.any(out > 0)
    assert it.stats()["launches"] == bdpt_amd.DenoiseSettings().iterations + 1

    check_golden(it, Host().frame(it)(), name, manifest)  # and a host entry after all of it
    it.close()


@pytest.mark.parametrize("scene", list(GOLDEN))
def test_gpu_one_context_serves_growing_demands(scene, golden_manifest):
    run_sequence(scene, Host(), golden_manifest)


@pytest.mark.parametrize("scene", list(GOLDEN))
def test_gpu_one_context_serves_growing_demands_on_a_callers_stream(scene, golden_manifest):
    run_sequence(scene, OnStream(), golden_manifest)


# ---- refusals: code and message of every frame entry, copied from csrc/bdpt_capi.cpp ----
INVALID, UNSUPPORTED = bdpt_amd.ERR_INVALID, bdpt_amd.ERR_UNSUPPORTED
SIZE = "width/height/spp must be > 0"
HOST_SIZE = "width/height must be > 0"  # the path / direct host entries size their staging buffer first
SHARD = "bad row shard"
PAST = "sample window: count reaches past spp (first + (count - 1) * stride must be < spp = 4)"
RR_DEPTH = "rr_depth must be in [1, 1024]"
FLAG = "unknown flag (bit 2, the round-1 wavefront schedule, was removed)"
NEGATIVE = "negative sample counts"
STRATEGY = "Error: wrong strategy"
AOV_FLAG = "bdpt_render_aov: flags must be 0 (no counting pass or full traversal)"
WINDOW_PAST = (2, 1, 3)  # of spp 4: 2 + 2 * 1 = 4

# (entry, frame fields, integrator fields, window, code, message[, the host entry's message])
REFUSALS = [
    # what every entry checks
    *[(e, dict(width=0), {}, None, INVALID, SIZE, HOST_SIZE if e in ("path", "direct") else SIZE)
      for e in ("bdpt", "path", "direct", "aov")],
    *[(e, dict(spp=0), {}, None, INVALID, SIZE) for e in ("bdpt", "path", "direct", "aov")],
    *[(e, dict(row_stride=0), {}, None, INVALID, SHARD) for e in ("bdpt", "path", "direct", "aov")],
    *[(e, dict(row_offset=-1), {}, None, INVALID, SHARD) for e in ("bdpt", "path", "direct", "aov")],
    *[(e, {}, {}, WINDOW_PAST, INVALID, PAST) for e in ("bdpt", "path", "direct", "aov")],
    # what an entry owns
    ("bdpt", dict(rr_depth=0), {}, None, UNSUPPORTED, RR_DEPTH),
    ("bdpt", dict(flags=4), {}, None, UNSUPPORTED, FLAG),
    ("path", {}, dict(emitter_samples=-1), None, INVALID, NEGATIVE),
    ("path", {}, dict(bsdf_samples=-1), None, INVALID, NEGATIVE),
    ("direct", {}, dict(bsdf_samples=-1), None, INVALID, NEGATIVE),
    ("direct", {}, dict(sampling_strategy=0), None, INVALID, STRATEGY),
    ("direct", {}, dict(sampling_strategy=6), None, INVALID, STRATEGY),
    ("aov", dict(flags=1), {}, None, UNSUPPORTED, AOV_FLAG),
    # two at once: which one is reported
    ("bdpt", dict(spp=0, rr_depth=0), {}, None, INVALID, SIZE),
    ("bdpt", dict(rr_depth=0, flags=4), {}, None, UNSUPPORTED, RR_DEPTH),
    ("bdpt", dict(rr_depth=0, row_stride=0), {}, None, UNSUPPORTED, RR_DEPTH),
    ("bdpt", dict(flags=4, strategy=3), {}, None, UNSUPPORTED, FLAG),
    ("bdpt", dict(strategy=3, row_stride=0), {}, None, INVALID, "unknown strategy"),
    ("bdpt", dict(row_stride=0), {}, WINDOW_PAST, INVALID, SHARD),
    ("bdpt", dict(russian_roulette=2), {}, WINDOW_PAST, INVALID, "unknown russian_roulette mode"),
    ("path", dict(height=0, row_stride=0), {}, None, INVALID, SIZE, HOST_SIZE),
    ("path", dict(row_stride=0), dict(emitter_samples=-1), None, INVALID, SHARD),
    ("path", {}, dict(bsdf_samples=-1), WINDOW_PAST, INVALID, NEGATIVE),
    ("path", {}, dict(max_depth=600), WINDOW_PAST, INVALID, PAST),
    ("path", {}, dict(max_depth=600), None, UNSUPPORTED, "maxDepth > 510 is not supported"),
    ("direct", dict(row_offset=-1), dict(sampling_strategy=0), None, INVALID, SHARD),
    ("direct", {}, dict(sampling_strategy=0, emitter_samples=-1), None, INVALID, STRATEGY),
    ("direct", {}, dict(emitter_samples=-1), WINDOW_PAST, INVALID, NEGATIVE),
    ("aov", dict(spp=0, flags=1), {}, None, INVALID, SIZE),
    ("aov", dict(flags=1, row_stride=0), {}, None, UNSUPPORTED, AOV_FLAG),
    ("aov", dict(row_stride=0), {}, WINDOW_PAST, INVALID, SHARD),
]


@pytest.fixture(scope="module")
def refusing():
    it = context("caustic", 16, 16, 4, 3)
    yield it
    it.close()


@pytest.mark.parametrize("case", REFUSALS, ids=[f"{i}-{c[0]}" for i, c in enumerate(REFUSALS)])
def test_gpu_frame_entries_refuse_with_the_same_code_and_message(case, refusing):
    entry, frame, integ, window, code, msg = case[:6]
    host_msg = case[6] if len(case) > 6 else msg
    it = refusing
    p = it.params()
    for k, v in frame.items():
        setattr(p, k, v)
    w = bdpt_amd.SampleWindow(*window).c() if window else None
    pp = bdpt_amd.PathSettings().c() if entry == "path" else None
    dp = bdpt_amd.DirectSettings(sampling_strategy="mis").c() if entry == "direct" else None
    for k, v in integ.items():
        setattr(pp if entry == "path" else dp, k, v)
    ref = lambda x: x and ctypes.byref(x)  # noqa: E731
    n = 16 * 16 * 8
    host = np.full(n, 7.0, np.float32)
    dev = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dptr = ctypes.c_void_p(dev.data_ptr())
    if entry == "aov":
        calls = [(host_msg, lambda: L().bdpt_render_aov_host(it._h, ctypes.byref(p), ref(w), host.ctypes.data)),
                 (msg, lambda: L().bdpt_render_aov(it._h, ctypes.byref(p), ref(w), dptr, None))]
    else:  # the window entries: with a null window exactly the unwindowed ones
        calls = [(host_msg, lambda: L().bdpt_render_window_host(it._h, ctypes.byref(p), ref(w), ref(pp), ref(dp),
                                                                host.ctypes.data)),
                 (msg, lambda: L().bdpt_render_window(it._h, ctypes.byref(p), ref(w), ref(pp), ref(dp), dptr, None))]
        if not window:
            calls += {"bdpt": [(host_msg, lambda: L().bdpt_render_host(it._h, ctypes.byref(p), host.ctypes.data)),
                               (msg, lambda: L().bdpt_render(it._h, ctypes.byref(p), dptr, None))],
                      "path": [(host_msg, lambda: L().bdpt_render_path_host(it._h, ctypes.byref(p), ref(pp),
                                                                            host.ctypes.data)),
                               (msg, lambda: L().bdpt_render_path(it._h, ctypes.byref(p), ref(pp), dptr, None))],
                      "direct": [(host_msg, lambda: L().bdpt_render_direct_host(it._h, ctypes.byref(p), ref(dp),
                                                                                host.ctypes.data)),
                                 (msg, lambda: L().bdpt_render_direct(it._h, ctypes.byref(p), ref(dp), dptr, None))],
                      }[entry]
    for expect, call in calls:
        assert call() == code
        assert L().bdpt_last_error().decode() == expect
    it.synchronize()
    assert np.all(host == 7.0) and bool(torch.all(dev == 7.0))


# ---- a context the library refuses to create ----
def many_emitters_obj(dst_dir, n=600):
    """cbox_low plus n one-triangle shapes of its emissive material under the ceiling."""
    src = variants.obj_path("cbox_low")
    with open(src) as f:
        base = f.read()
    nv = sum(1 for line in base.splitlines() if line.startswith("v "))
    nn = sum(1 for line in base.splitlines() if line.startswith("vn "))
    lines = ["vn 0.0000 -1.0000 0.0000"]
    for i in range(n):
        x, z = -0.9 + 0.06 * (i % 30), -0.9 + 0.06 * (i // 30)
        a, vn = nv + 3 * i + 1, nn + 1
        lines += [f"o emitter{i}", f"v {x:.6f} 1.5 {z:.6f}", f"v {x + 0.04:.6f} 1.5 {z:.6f}",
                  f"v {x:.6f} 1.5 {z + 0.04:.6f}", "usemtl light", f"f {a}//{vn} {a + 1}//{vn} {a + 2}//{vn}"]
    os.makedirs(dst_dir, exist_ok=True)
    dst = os.path.join(dst_dir, "many_emitters.obj")
    with open(dst, "w") as f:
        f.write(base.rstrip("\n") + "\n" + "\n".join(lines) + "\n")
    shutil.copyfile(os.path.join(os.path.dirname(src), "cbox_low.mtl"), os.path.join(dst_dir, "cbox_low.mtl"))
    return dst


def test_gpu_refused_context_leaves_a_working_library(tmp_path, golden_manifest):
    """600 emitters: 600 EmitterRecords of 48 B are 28 800 B, past the 24 KiB (24 576 B) the
    LDS tables may take, so bdpt_ctx_create refuses after it has uploaded the scene arrays."""
    sc = bdpt_amd.Scene(many_emitters_obj(str(tmp_path)))
    assert sc.info()["emitters"] >= 600 and sc.info()["emitters"] * 48 > 24 * 1024
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES["cbox_low"]["camera"]), width=16, height=16)
    for _ in range(8):
        with pytest.raises(bdpt_amd.BdptError, match="emitter records exceed the 24 KiB LDS budget") as e:
            bdpt_amd.BDPTIntegrator(sc, cfg)
        assert e.value.code == UNSUPPORTED
    name = GOLDEN["caustic"]
    m = golden_manifest["framebuffers"][name]
    it = context("caustic", m["width"], m["height"], m["spp"], m["rr_depth"])
    check_golden(it, it.render_frame(), name, golden_manifest)
    it.close()
