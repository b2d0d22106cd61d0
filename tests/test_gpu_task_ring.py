"""The per-wave shadow-ray task rings (bdpt_path.hpp task_push).

A task record holds its shadow ray's end points (40 bytes for a connection or
next-event task, 28 for a camera splat, whose start is the camera); the lane
that claims it forms the ray again. These tests make the ring wrap and refuse
pushes (BDPT_TASK_CAP=64, the smallest capacity, read when the integrator's
context is created), run both record shapes at the default capacity, and
render with Russian roulette, whose kernels have no ring (the context then
allocates none). The checks are the suite's: goldens at test_gpu_parity's
tolerance and metric, and the counting pass against the oracle's counters as
in test_gpu_counters.

bdpt_stats.sched of a task-ring build holds (tasks pushed, pushes refused,
claim rounds, claims); bdpt_amd.py still names the first two "step_tasks" and
"shade_steps".
"""
import numpy as np
import pytest

import bdpt_amd
import oracle as O
import variants
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_parity.py

_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = bdpt_amd.Scene(variants.obj_path(name))
    return _scenes[name]


def rel_l2(fb, ref):  # per pixel, as tests/test_gpu_parity.py
    a = fb.reshape(-1, 3).astype(np.float64)
    r = ref.reshape(-1, 3).astype(np.float64)
    return np.linalg.norm(a - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-8)


def counting_pass(name, W, H, spp, rr, off=0, stride=1, russian_roulette=0):
    cam = bdpt_amd.Camera(**variants.SCENES[name]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp, rr_depth=rr, russian_roulette=russian_roulette)
    it = bdpt_amd.BDPTIntegrator(scene(name), cfg)
    it.init()
    it.render_frame(row_offset=off, row_stride=stride, flags=bdpt_amd.FLAG_COUNT)
    return it.stats()


def assert_oracle_counters(st, name, W, H, spp, rr, off=0, stride=1, russian_roulette=0):
    """tests/test_gpu_counters.py's equality: what steers a path, then the queries."""
    rows = list(range(off, H, stride))
    p = O.make_params(variants.SCENES[name]["camera"], W, H, spp, rr)
    p.russian_roulette = russian_roulette
    O.counters(True)
    _, n_ref = O.Scene(variants.obj_path(name)).render(p, rows=rows)
    o = O.counters(True)
    g = st["counters"]
    assert st["samples"] == n_ref == len(rows) * W * spp
    assert o["eye_retraces"] > 0
    pairs = {k: (g[k], o[k]) for k in ("rng_draws", "light_verts", "light_vert_reads", "shadow_rays", "splats")}
    pairs["closest_rays"] = (g["closest_rays"], o["closest_rays"] - o["eye_retraces"])
    bad = {k: v for k, v in pairs.items() if v[0] != v[1]}
    assert not bad, f"{st['kernel']}: counters differ from the oracle's (gpu, oracle): {bad}"
    return g


@pytest.mark.parametrize("name", ["G2_caustic_64x64_spp16", "G5_caustic_80x48_spp1"])
def test_gpu_small_ring_wraps_and_refuses_frame_matches_golden(name, golden_manifest, monkeypatch):
    monkeypatch.setenv("BDPT_TASK_CAP", "64")
    m = golden_manifest["framebuffers"][name]
    cam = bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=m["width"], height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(scene(m["scene"]), cfg)
    it.init()
    fb = it.render_frame(row_offset=0, row_stride=m["row_stride"]).reshape(-1)
    assert it.stats()["samples"] == m["samples"]
    assert np.all(np.isfinite(fb))
    worst = rel_l2(fb, load_golden(name)).max()
    print(f"{name} at BDPT_TASK_CAP=64: max per-pixel rel L2 {worst:.3g}")
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


def test_gpu_small_ring_wraps_and_refuses_exact_paths(monkeypatch):
    """64 slots per wave: far more tasks pass through a ring than it holds (it
    wraps), and pushes are refused (the owner then traces that shadow ray itself);
    the walked paths and queries stay the oracle's."""
    monkeypatch.setenv("BDPT_TASK_CAP", "64")
    case = ("caustic", 64, 64, 16, 8)
    st = counting_pass(*case)
    pushed, refused, rounds, claims = (st["sched"][k] for k in ("step_tasks", "shade_steps", "steps_ge32", "steps_ge64"))
    print(f"BDPT_TASK_CAP=64 {case}: pushed {pushed} refused {refused} claim rounds {rounds} claims {claims} "
          f"({st['samples']} samples)")
    assert st["kernel"] == "bdpt_frame_kernel"
    assert pushed > 0 and claims == pushed
    assert refused > 0, "no push was refused: the ring-full fallback did not run"
    assert pushed > 64 * 4096, "fewer tasks than slots in the grid's rings: no ring can have wrapped"
    assert_oracle_counters(st, *case)


@pytest.mark.parametrize("case", [("hardlight", 64, 64, 16, 8), ("cbox_low", 64, 64, 4, 8)])
def test_gpu_default_ring_mixed_task_kinds_exact_paths(case):
    """Both record shapes in one frame: camera splats (28 bytes) and connection /
    next-event tasks (40 bytes)."""
    st = counting_pass(*case)
    assert st["sched"]["step_tasks"] > 0 and st["sched"]["steps_ge64"] == st["sched"]["step_tasks"]
    g = assert_oracle_counters(st, *case)
    assert g["splats"] > 0 and g["shadow_rays"] > g["splats"]


def test_gpu_russian_roulette_context_renders_without_a_ring():
    """The Russian-roulette kernels push no tasks; their context allocates no ring
    and still walks the oracle's paths."""
    case = ("caustic", 64, 64, 4, 8)
    st = counting_pass(*case, russian_roulette=1)
    assert st["kernel"].startswith("bdpt_frame_kernel_rr")
    assert_oracle_counters(st, *case, russian_roulette=1)
