"""Light groups (bdpt_render_light_groups): one BDPT frame split by the emitter
at the light end of each contribution's path, and recombined with per-group RGB gains
(bdpt_light_groups_relight).

The planes must add up to the reference's frame (the goldens, at the project's bound: per-pixel
relative L2 <= 1e-4, tests/test_gpu_parity.py's metric), each plane must be right in absolute
terms (the planes of emit_edges recombined with per-emitter gains must be the reference's frame
of the scene with those emitters' Ke scaled, tests/golden/make_light_groups_golden.py), group
maps must merge planes, row shards and sample windows must commute with the split, the ring-full
fallback must file its connections like the tasks, the relight kernel must be the sequential
float32 loop bit for bit, and what the build does not serve must be refused before any launch.

Frames are at most 64 x 64 x 16 spp. A grouped render is made once per (case, map) and shared."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO, gpu_available, load_golden
from test_config_exr import decode_exr
from plane_cases import (CBOX_CASE, EDGES_CASE, FRAMES, LT_CASE, PT_CASE, STRATEGY, golden_integrator, plane_sum, refused,
                         scene, unsupported_setups, worst_per_plane)
from test_gpu_parity import TOL, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CAUSTIC_CASE = "G2_caustic_64x64_spp16"
SUM_CASES = [EDGES_CASE, CBOX_CASE, CAUSTIC_CASE, LT_CASE, PT_CASE]
KERNEL = "bdpt_frame_kernel_groups"
RELIT = np.load(os.path.join(REPO, "tests", "golden", "light_groups_emit_edges_relit.npz"))

_groups = {}


def emitter_count(name):
    return len(scene(variants.obj_path(FRAMES[name]["scene"])).emitters())


def groups_of(name, group_map=None, n_groups=None, **kw):
    """The grouped render of a golden's frame, made once (read-only: callers do not write to it)."""
    key = (name, None if group_map is None else tuple(group_map), n_groups, tuple(sorted(kw.items())))
    if key not in _groups:
        it = golden_integrator(name, **kw)
        out = it.render_light_groups(group_map, n_groups)
        st = it.stats()
        n = n_groups if n_groups is not None else (emitter_count(name) if group_map is None else max(group_map) + 1)
        assert st["kernel"] == KERNEL, st["kernel"]
        assert st["schedule_errors"] == 0 and st["samples"] == FRAMES[name]["samples"]
        assert out.shape == (n, FRAMES[name]["height"], FRAMES[name]["width"], 3) and out.dtype == np.float32
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _groups[key] = out
    return _groups[key]


def relight_model(planes, gains):
    """bdpt_light_groups_relight as include/bdpt_amd.h defines it: float32, the product and the
    sum rounded one after the other, ascending groups."""
    planes, gains = np.asarray(planes, np.float32), np.asarray(gains, np.float32)
    acc = gains[0][None, None, :] * planes[0]
    for g in range(1, planes.shape[0]):
        t = gains[g][None, None, :] * planes[g]
        acc = acc + t
    assert acc.dtype == np.float32
    return acc


# ---------------------------------------------------------------- 1. the planes add up
@pytest.mark.parametrize("name", SUM_CASES)
def test_gpu_planes_sum_to_the_reference_frame(name):
    n = emitter_count(name)
    planes = groups_of(name)
    assert planes.shape[0] == n
    if name == CBOX_CASE:
        assert n == 1
    ref = load_golden(name)
    total = planes[0] if n == 1 else plane_sum(planes)  # one emitter: the plane itself is the frame
    worst = rel_l2(np.asarray(total), ref).max()
    print(f"{name}: {n} emitters, max per-pixel rel L2 of the plane sum {worst:.3g}; plane means "
          f"{[float(f'{x:.3g}') for x in planes.reshape(n, -1).mean(axis=1)]}")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


# ------------------------------------------------ 2. each plane in absolute terms
def edges_gains():
    """Per emitter index (Scene.emitters() order) the golden's RGB gain, found through the
    emitter's material: its index names a `newmtl` of the MTL in file order."""
    obj = variants.obj_path("emit_edges")
    with open(os.path.splitext(obj)[0] + ".mtl") as f:
        names = re.findall(r"^\s*newmtl\s+(\S+)", f.read(), re.M)
    by_material = {str(m): RELIT["gains"][i] for i, m in enumerate(RELIT["materials"])}
    em = scene(obj).emitters()
    assert len(em) == 5 and len({e["material"] for e in em}) == 5
    return np.float32([by_material[names[e["material"]]] for e in em])


@pytest.mark.parametrize("strategy", ["bdpt", "lt", "pt"])
def test_gpu_relit_planes_are_the_reference_frame_of_the_rescaled_scene(strategy):
    """The reference rendered emit_edges with every emitter's Ke multiplied by its own RGB gain;
    the planes of the unscaled scene, each multiplied by its emitter's gain, must be that frame.
    A contribution filed under a wrong emitter at any of the four sites gets a wrong gain (the
    gains differ per emitter and channel). BDPT reaches all sites; light tracing alone pins
    connectToCamera and the camera ray's own hit, path tracing connectToLight and the eye hits."""
    W, H, spp, rr = (int(x) for x in RELIT["shape"])
    assert (W, H, spp, rr) == tuple(FRAMES[EDGES_CASE][k] for k in ("width", "height", "spp", "rr_depth"))
    planes = groups_of(EDGES_CASE, strategy=STRATEGY[strategy])
    gains = edges_gains()
    it = golden_integrator(EDGES_CASE)
    relit = it.relight(planes, gains)
    ref = RELIT[strategy]
    worst = rel_l2(relit, ref).max()
    # the plain frame against the same golden: how far a wrong filing is from passing
    plain = rel_l2(plane_sum(planes), ref).max()
    print(f"{strategy}: relit planes vs the rescaled scene's reference frame {worst:.3g} (the unscaled sum: {plain:.3g})")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"
    assert plain > 0.1  # the golden is not the unscaled frame
    for g in range(5):
        assert planes[g].any(), f"plane {g} is empty"
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(planes[a], planes[b]), (a, b)


# ------------------------------------------------------------------------- 3. maps
def test_gpu_group_maps_merge_planes():
    ident = groups_of(EDGES_CASE)
    two = groups_of(EDGES_CASE, [0, 0, 1, 1, 1], 2)
    assert two.shape[0] == 2
    w0 = rel_l2(two[0], plane_sum(ident[:2])).max()
    w1 = rel_l2(two[1], plane_sum(ident[2:])).max()
    print(f"map [0, 0, 1, 1, 1]: plane 0 vs identity planes 0 + 1 {w0:.3g}, plane 1 vs 2 + 3 + 4 {w1:.3g}")
    assert w0 <= TOL and w1 <= TOL
    eight = groups_of(EDGES_CASE, [0, 1, 2, 3, 4], 8)
    assert eight.shape[0] == 8
    assert not eight[5:].any(), "a plane no emitter maps to holds energy"
    assert worst_per_plane(eight[:5], ident) <= TOL


# ------------------------------------------------------- 4. decompositions commute
def test_gpu_row_shards_sum_to_the_full_planes():
    full = groups_of(EDGES_CASE)
    parts = [golden_integrator(EDGES_CASE).render_light_groups(row_offset=o, row_stride=2) for o in (0, 1)]
    worst = worst_per_plane(parts[0] + parts[1], full)
    print(f"two interleaved row shards: worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= TOL


def test_gpu_sample_windows_sum_to_the_full_planes():
    """The even and the odd samples of 16 spp on one 64-pixel row of the five-emitter scene."""
    row = dict(row_offset=20, row_stride=64)
    kw = dict(width=64, height=64, spp=16)
    full = golden_integrator(EDGES_CASE, **kw).render_light_groups(**row)
    a = golden_integrator(EDGES_CASE, **kw).render_light_groups(window=bdpt_amd.SampleWindow(0, 2, 8), **row)
    b = golden_integrator(EDGES_CASE, **kw).render_light_groups(window=bdpt_amd.SampleWindow(1, 2, 8), **row)
    assert all(full[g, 20].any() for g in range(5))  # (camera splats of the row's samples land on other rows too)
    worst = worst_per_plane(a + b, full)
    print(f"sample windows 0:2:8 + 1:2:8 of 16: worst per-plane per-pixel rel L2 {worst:.3g}")
    assert worst <= TOL
    assert rel_l2(plane_sum(full), golden_integrator(EDGES_CASE, **kw).render_frame(**row)).max() <= TOL


# ------------------------------------------------- 5. the ring-full path is grouped
RING_SCRIPT = """
import json, sys
import numpy as np
import torch
import bdpt_amd, variants
name, W, H, spp, rr, out = json.loads(sys.argv[1])
cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[name]["camera"]), width=W, height=H, spp=spp, rr_depth=rr)
it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
it.init()
planes = it.render_light_groups()
st = it.stats()
np.save(out, planes)
# a grouped render cannot count (flags are refused): the default build, whose schedule and ring this
# build shares, counts the same frame on the same context
it.render_frame(flags=bdpt_amd.FLAG_COUNT)
sched = it.stats()["sched"]
print("RING " + json.dumps({"kernel": st["kernel"], "schedule_errors": int(st["schedule_errors"]),
                           "samples": int(st["samples"]), "pushed": int(sched["step_tasks"]),
                           "refused": int(sched["shade_steps"])}))
"""


def test_gpu_ring_full_fallback_is_grouped(tmp_path):
    """BDPT_TASK_CAP=64 in a fresh process (the context reads it when it is created): pushes are
    refused and the owner traces those shadow rays itself; each such connection must still land
    in its emitter's plane (pend_px). stats()["sched"] of the counting pass at that capacity
    shows the refusals (tests/test_gpu_task_ring.py's fields)."""
    m = FRAMES[CAUSTIC_CASE]
    out = str(tmp_path / "planes.npy")
    env = dict(os.environ, BDPT_TASK_CAP="64")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "bidirectional-path-tracing_amd"),
                                         os.path.join(REPO, "scenes")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    case = [m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"], out]
    p = subprocess.run([sys.executable, "-c", RING_SCRIPT, json.dumps(case)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads([line for line in p.stdout.splitlines() if line.startswith("RING ")][-1][5:])
    planes = np.load(out)
    print(f"{CAUSTIC_CASE} at BDPT_TASK_CAP=64: {got}")
    assert got["kernel"] == KERNEL and got["schedule_errors"] == 0 and got["samples"] == m["samples"]
    assert got["refused"] > 0, "no push was refused: the ring-full fallback did not run"
    assert np.isfinite(planes).all()
    worst = rel_l2(plane_sum(planes), load_golden(CAUSTIC_CASE)).max()
    per_plane = worst_per_plane(planes, groups_of(CAUSTIC_CASE))
    print(f"plane sum vs golden {worst:.3g}, per plane vs the default ring {per_plane:.3g}")
    assert worst <= TOL and per_plane <= TOL


# ------------------------------------------------------------------- 6. relight bits
def test_gpu_relight_is_the_sequential_float32_loop():
    planes = groups_of(EDGES_CASE)
    assert planes.shape == (5, 32, 32, 3)
    it = golden_integrator(EDGES_CASE)
    rng = np.random.default_rng(20261020)
    gains = rng.uniform(-2.0, 3.0, (5, 3)).astype(np.float32)
    gains[1] = 0.0  # a zero gain multiplies (its plane still enters the sum)
    gains[3, 0] = -0.75
    assert (gains < 0).any() and (gains == 0).any()
    want = relight_model(planes, gains)
    got = it.relight(planes, gains)
    again = it.relight(planes, gains)
    assert got.shape == (32, 32, 3) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    ones = it.relight(planes, np.ones((5, 3), np.float32))
    seq = planes[0].copy()
    for g in range(1, 5):
        seq = seq + planes[g]  # float32 + float32, ascending
    assert np.array_equal(ones.view(np.uint32), seq.view(np.uint32))
    grey = it.relight(planes, np.float32([1, 2, 0.5, 4, 3]))
    assert np.array_equal(grey.view(np.uint32),
                          relight_model(planes, np.repeat(np.float32([1, 2, 0.5, 4, 3])[:, None], 3, 1)).view(np.uint32))
    # a frame whose float count is no multiple of 12 and a single plane (the dword-load kernel)
    odd = np.ascontiguousarray(planes[:3, :5, :7])
    assert np.array_equal(it.relight(odd, gains[:3]).view(np.uint32), relight_model(odd, gains[:3]).view(np.uint32))
    one = it.relight(planes[:1], gains[3:4])
    assert np.array_equal(one.view(np.uint32), (gains[3][None, None, :] * planes[0]).view(np.uint32))


def test_gpu_relight_errors():
    import torch

    it = golden_integrator(EDGES_CASE)
    planes = groups_of(EDGES_CASE)
    I = bdpt_amd.ERR_INVALID
    for bad in (np.float32([[1, 1, np.nan]] * 5), np.float32([[1, np.inf, 1]] * 5)):
        with pytest.raises(bdpt_amd.BdptError) as e:
            it.relight(planes, bad)
        assert e.value.code == I and "finite" in str(e.value), str(e.value)
    d = torch.zeros(5 * 32 * 32 * 3, dtype=torch.float32, device="cuda")
    o = torch.zeros(32 * 32 * 3, dtype=torch.float32, device="cuda")
    g = np.ones((5, 3), np.float32)
    launches = it.stats()["launches"]
    for n, w, h, gains, out, word in ((65, 32, 32, np.ones((65, 3), np.float32), o.data_ptr(), "n_groups"),
                                      (5, 0, 32, g, o.data_ptr(), "width"), (2, 32768, 16384, g[:2], o.data_ptr(), "2^30"),
                                      (5, 32, 32, g, d.data_ptr() + 4 * 32 * 32 * 3 * 4, "overlap"),
                                      (5, 32, 32, g, d.data_ptr(), "overlap")):
        with pytest.raises(bdpt_amd.BdptError) as e:
            it.relight_device(d.data_ptr(), n, w, h, gains, out)
        assert e.value.code == I and word in str(e.value), str(e.value)
    assert it.stats()["launches"] == launches


# ------------------------------------------------- 7. refusals and non-interference
def test_gpu_light_groups_unsupported_and_invalid(monkeypatch):
    U, I = bdpt_amd.ERR_UNSUPPORTED, bdpt_amd.ERR_INVALID
    name = EDGES_CASE
    for bad, kw, word in unsupported_setups(name, monkeypatch):
        refused(lambda: bad.render_light_groups(**kw), U, "light groups", word, launched=bad)
    it = golden_integrator(name)
    refused(lambda: it.render_light_groups([0] * 5, 0), I, "n_groups", launched=it)
    refused(lambda: it.render_light_groups([0] * 5, 65), I, "n_groups", launched=it)
    refused(lambda: it.render_light_groups(None, 4), I, "n_groups", "emitter count", launched=it)
    refused(lambda: it.render_light_groups(None, 6), I, "n_groups", "emitter count", launched=it)
    refused(lambda: it.render_light_groups([0, 1, 2, 3, 5], 5), I, "group_of_emitter[4]", launched=it)
    refused(lambda: it.render_light_groups([0, -1, 2, 3, 4], 5), I, "group_of_emitter[1]", launched=it)
    # n_groups * W * H >= 2^30, in the params only: refused before anything is allocated
    big = golden_integrator(name)
    big.render_frame()
    before = big.stats()["launches"]
    big.config.width, big.config.height = 32768, 16384
    for m, n in (([0, 0, 1, 1, 1], 2), ([0] * 5, 1)):
        if n == 1:
            big.config.width, big.config.height = 32768, 32768
        with pytest.raises(bdpt_amd.BdptError) as e:
            big.render_light_groups(m, n)
        assert e.value.code == I and "2^30" in str(e.value), str(e.value)
    assert big.stats()["launches"] == before


def test_gpu_plain_frames_around_a_grouped_render_are_unchanged():
    it = golden_integrator(CAUSTIC_CASE)  # caustic: glossy materials, so the default build by name
    before = it.render_frame().copy()
    k0 = it.stats()["kernel"]
    planes = it.render_light_groups()
    assert it.stats()["kernel"] == KERNEL
    it.rgb[:] = 0
    after = it.render_frame().copy()
    k1 = it.stats()["kernel"]
    assert k0 == k1 == "bdpt_frame_kernel", (k0, k1)
    assert rel_l2(after, before).max() <= TOL
    assert rel_l2(plane_sum(planes), before).max() <= TOL


def test_gpu_group_map_may_be_freed_after_the_call():
    """The asynchronous entry copies the caller's map before it returns: a map overwritten right
    after the call (before the device has run) does not change where contributions go."""
    import torch

    it = golden_integrator(EDGES_CASE)
    fb = torch.zeros((2, 32, 32, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    m = np.int32([0, 0, 1, 1, 1])
    it.render_light_groups_device(fb.data_ptr(), m, 2)
    m[:] = 0
    it.synchronize()
    assert worst_per_plane(fb.cpu().numpy(), groups_of(EDGES_CASE, [0, 0, 1, 1, 1], 2)) <= TOL


# ------------------------------------------------------------------- 8. the command line
def test_gpu_cli_writes_one_exr_per_emitter(tmp_path):
    """--light-groups on emit_edges: five extra EXRs that sum to the main one within half-float
    rounding. Every file is rounded to half once (relative error <= 2^-11 for a normal half) and
    the planes are non-negative, so the sum of the five rounded planes is within 2^-11 of the
    exact sum, the main file within 2^-11 more, and two renders differ by the order of their
    float32 atomic additions (<= 1e-4, about 0.2 of 2^-11): within 3 * 2^-11, the layers test's
    bound. Subnormal halves round absolutely, by at most 2^-25 in each of the six files: the
    floor 2^-22."""
    W = H = 32
    spp = 4
    cli = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("emit_edges", W, H, spp))
    r = subprocess.run([cli, str(toml), "--light-groups"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == [f"scene.E{e:02d}.exr" for e in range(5)] + ["scene.exr", "scene.toml"]
    main = decode_exr((tmp_path / "scene.exr").read_bytes()).astype(np.float64)
    parts = [decode_exr((tmp_path / f"scene.E{e:02d}.exr").read_bytes()).astype(np.float64) for e in range(5)]
    assert all(p.shape == main.shape and p.any() for p in parts)
    total = sum(parts)
    tol = 3 * 2.0 ** -11 * np.maximum(total, main) + 2.0 ** -22
    assert (np.abs(total - main) <= tol).all(), float((np.abs(total - main) / np.maximum(main, 1e-6)).max())
    path = tmp_path / "path.toml"
    path.write_text(variants.path_toml_text("emit_edges", W, H, spp))
    r = subprocess.run([cli, str(path), "--light-groups"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--light-groups" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted([f"scene.E{e:02d}.exr" for e in range(5)] + ["path.toml", "scene.exr", "scene.toml"])
