"""The reference-leaf check of a closest-hit walk made once, on the walk's winner
(bdpt_kernels.hip BDPT_LEAF_DEFER, bdpt_path.hpp closest_apply): the same
results as the check in the leaf step.

* The per-function entry of the protocol (bdpt_intersect_deferred: the deferred walk, the
  check against the box in the winner's shade record, the checked second walk) on the
  committed kat_intersect_* and kat_adversarial_* rays, closest hits: t, u, v and ids bit
  for bit against the reference's recorded results, with the debugging knob
  BDPT_LEAF_RECHECK off and on. On, every hit found by the culled walk took the second
  walk (rays that walk the reference's own tree — a direction with a zero component, an
  origin beyond 100 scene diagonals — defer nothing).
* Frames: Caustic 64^2 x 16 (G2), as a counting pass, against the golden at the suite's
  1e-4 per-pixel bound and the oracle's counters (as tests/test_gpu_counters.py compares
  them), knob on and off. On, the second walks equal the closest-hit rays that hit
  something (the hits the frame applied, counted where a result is applied). Off, the count is reported and, when it
  is 0, tri_tests and interior_visits equal those of the build with the check in the leaf
  step (lib/libbdpt_amd_defer0.so, in a process of its own).
* One small frame through each other build that takes the switch and a small golden reaches:
  the textured build (leaf id in the record, box from lbox) and _split. (_hbm is the default
  build's code with the BSDF table read from HBM; _deep, _layers and _groups keep the check in
  the leaf step.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bdpt_amd
import oracle as O
import variants
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4
GOLD = os.path.join(REPO, "tests", "golden")
FRAME = ("caustic", 64, 64, 16, 8)  # G2_caustic_64x64_spp16
_integ = {}


def integrator(scene, W=64, H=64, spp=16, rr=None, fresh=False):
    """fresh: an integrator of its own (a frame adds into its integrator's framebuffer)."""
    key = (scene, W, H, spp, rr)
    if fresh or key not in _integ:
        cam = bdpt_amd.Camera(**variants.SCENES[scene]["camera"])
        cfg = bdpt_amd.Config(camera=cam, width=W, height=H, spp=spp,
                              rr_depth=rr if rr is not None else variants.SCENES[scene]["rr_depth"])
        it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(scene)), cfg)
        it.init()
        if fresh:
            return it
        _integ[key] = it
    return _integ[key]


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b)


def rel_l2(fb, ref):
    a = fb.reshape(-1, 3).astype(np.float64)
    r = ref.reshape(-1, 3).astype(np.float64)
    return np.linalg.norm(a - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-8)


def knob(monkeypatch, on):
    monkeypatch.setenv("BDPT_DEBUG_KNOBS", "1")
    monkeypatch.setenv("BDPT_LEAF_RECHECK", "1" if on else "0")


def culled_walk(rays):
    """Rays the culled 4-wide walk serves (ray_inv's `fast`): finite reciprocal directions."""
    with np.errstate(divide="ignore"):
        inv = 1.0 / rays[:, 3:6].astype(np.float32)
    return np.isfinite(inv).all(1) & np.isfinite(rays[:, 0:3]).all(1)


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("scene", ["caustic", "hardlight", "cbox_low"])
def test_gpu_deferred_intersect_matches_reference(scene, force, monkeypatch):
    knob(monkeypatch, force)
    g = np.load(os.path.join(GOLD, f"kat_intersect_{scene}.npz"))
    h, again = integrator(scene).intersect_deferred(g["rays"])
    ref = g["out"]
    assert np.array_equal(h["hit"], ref[:, 0].astype(np.int32))
    k = ref[:, 0] == 1
    r, hh = ref[k], h[k]
    assert same_bits(hh["t"], r[:, 1]) and same_bits(hh["u"], r[:, 2]) and same_bits(hh["v"], r[:, 3])
    assert np.array_equal(hh["shape_id"], r[:, 4].view(np.int32))
    assert np.array_equal(hh["prim_id"], r[:, 5].view(np.int32))
    assert np.array_equal(hh["mat_id"], r[:, 6].view(np.int32))
    assert same_bits(hh["p"], r[:, 7:10]) and same_bits(hh["ns"], r[:, 10:13])
    assert same_bits(hh["ng"], r[:, 13:16]) and same_bits(hh["wo"], r[:, 16:19])
    walked = culled_walk(g["rays"])
    print(f"{scene} force={force}: {int(k.sum())} hits of {len(k)} rays, {int(walked.sum())} on the culled walk, "
          f"{int(again.sum())} walked again")
    assert (k & walked).sum() > 0.5 * k.sum()
    if force:
        assert np.all(again[k & walked] == 1)
    assert np.all(again[~walked] == 0)


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("scene", ["caustic", "hardlight", "synth1m"])
def test_gpu_deferred_intersect_adversarial_rays_match_reference(scene, force, monkeypatch):
    """tests/test_gpu_kat.py's adversarial batches (without the near cull, with the plane normal's
    rule, with the frames' own rule), closest hits."""
    knob(monkeypatch, force)
    g = np.load(os.path.join(GOLD, f"kat_adversarial_{scene}.npz"))
    it = integrator(scene)
    rays, kind, onrm, otri, osn = g["rays"], g["kind"], g["onrm"], g["otri"], g["osn"]
    far = kind == 4
    every = np.ones_like(far)
    cases = ((~far, None, None), (far, None, None), (every, None, None), (~far, onrm[~far], None),
             (every, onrm, None), (~far, osn[~far], otri[~far]), (every, osn, otri))
    for n, (sel, nrm, tris) in enumerate(cases):
        h, again = it.intersect_deferred(rays[sel], origin_normals=nrm, origin_tris=tris)
        hit = g["hit"][sel].astype(np.int32)
        bad = np.flatnonzero(h["hit"] != hit)
        assert bad.size == 0, f"{bad.size} acceptance mismatches, kinds {np.bincount(kind[sel][bad])}"
        k = hit == 1
        assert same_bits(h["t"][k], g["t"][sel][k]) and same_bits(h["u"][k], g["u"][sel][k])
        assert same_bits(h["v"][k], g["v"][sel][k])
        assert np.array_equal(h["shape_id"][k], g["shape"][sel][k]) and np.array_equal(h["prim_id"][k],
                                                                                          g["prim"][sel][k])
        walked = culled_walk(rays[sel]) & ~far[sel]  # (of the far origins, those past 100 diagonals walk the reference's tree)
        print(f"{scene} case {n} force={force}: {int(k.sum())} hits, {int(again.sum())} walked again")
        if force:
            assert np.all(again[k & walked] == 1)


COUNT_SCRIPT = """
import json, sys
import torch
import bdpt_amd, variants
name, W, H, spp, rr = json.loads(sys.argv[1])
cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[name]["camera"]), width=W, height=H, spp=spp, rr_depth=rr)
it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
it.init()
it.render_frame(flags=bdpt_amd.FLAG_COUNT)
st = it.stats()
print("COUNTS " + json.dumps({"lib": bdpt_amd.LIB_PATH, "kernel": st["kernel"], "samples": st["samples"],
                             "leaf_rewalks": st["leaf_rewalks"], "leaf_hits": st["leaf_hits"],
                             "counters": {k: int(v) for k, v in st["counters"].items()}}))
"""
_oracle = {}


def oracle_counters():
    if "o" not in _oracle:
        name, W, H, spp, rr = FRAME
        O.counters(True)
        _, n = O.Scene(variants.obj_path(name)).render(O.make_params(variants.SCENES[name]["camera"], W, H, spp, rr))
        _oracle["o"] = (O.counters(True), n)
    return _oracle["o"]


def counted_frame():
    """FRAME as a counting pass: (stats, framebuffer); the golden and the oracle's counters asserted."""
    name, W, H, spp, rr = FRAME
    it = integrator(name, W, H, spp, rr, fresh=True)
    fb = it.render_frame(flags=bdpt_amd.FLAG_COUNT).reshape(-1)
    st = it.stats()
    worst = rel_l2(fb, load_golden("G2_caustic_64x64_spp16")).max()
    print(f"{st['kernel']}: max per-pixel rel L2 {worst:.3g}, leaf_rewalks {st['leaf_rewalks']}")
    assert np.all(np.isfinite(fb)) and worst <= TOL, worst
    assert st["schedule_errors"] == 0
    o, n_ref = oracle_counters()
    g = st["counters"]
    assert st["samples"] == n_ref == W * H * spp
    pairs = {k: (g[k], o[k]) for k in ("rng_draws", "light_verts", "light_vert_reads", "shadow_rays", "splats")}
    pairs["closest_rays"] = (g["closest_rays"], o["closest_rays"] - o["eye_retraces"])
    bad = {k: v for k, v in pairs.items() if v[0] != v[1]}
    assert not bad, f"{st['kernel']}: counters differ from the oracle's (gpu, oracle): {bad}"
    return st


def test_gpu_frame_with_every_hit_walked_again(monkeypatch):
    knob(monkeypatch, True)
    st = counted_frame()
    # every closest hit the frame applied (counted where a result is applied, after the second walk)
    # was walked twice; the rest of the closest-hit rays left the box through its open side
    print(f"leaf_rewalks {st['leaf_rewalks']} leaf_hits {st['leaf_hits']} closest_rays {st['counters']['closest_rays']}")
    assert 0 < st["leaf_hits"] <= st["counters"]["closest_rays"]
    assert st["leaf_rewalks"] == st["leaf_hits"]


def test_gpu_frame_counters_equal_leaf_step_check_build(monkeypatch):
    knob(monkeypatch, False)
    st = counted_frame()
    g = st["counters"]
    assert st["leaf_rewalks"] >= 0
    lib0 = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "libbdpt_amd_defer0.so")
    assert os.path.exists(lib0), f"{lib0} is missing: build() makes it"
    env = dict(os.environ, BDPT_AMD_LIB=lib0)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "bidirectional-path-tracing_amd"),
                                         os.path.join(REPO, "scenes")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", COUNT_SCRIPT, json.dumps(FRAME)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    zero = json.loads([line for line in p.stdout.splitlines() if line.startswith("COUNTS ")][-1][7:])
    assert zero["lib"] == lib0 and zero["kernel"] == st["kernel"] and zero["samples"] == st["samples"]
    assert zero["leaf_rewalks"] == 0
    print(f"{st['kernel']}: leaf_rewalks {st['leaf_rewalks']}, tri_tests {g['tri_tests']} interior_visits "
          f"{g['interior_visits']} (check in the leaf step: {zero['counters']['tri_tests']} "
          f"{zero['counters']['interior_visits']})")
    for k in ("closest_rays", "shadow_rays"):
        assert int(g[k]) == zero["counters"][k], (k, int(g[k]), zero["counters"][k])
    if st["leaf_rewalks"] == 0:
        for k in ("tri_tests", "interior_visits"):
            assert int(g[k]) == zero["counters"][k], (k, int(g[k]), zero["counters"][k])


@pytest.mark.parametrize("force", [False, True])
def test_gpu_textured_frame(force, monkeypatch):
    knob(monkeypatch, force)
    with open(os.path.join(GOLD, "tex_manifest.json")) as f:
        man = json.load(f)
    m = man["frames"]["tex_T1_texbox_bdpt"]
    cam = bdpt_amd.Camera(**{k: tuple(v) if isinstance(v, list) else v for k, v in man["camera"].items()})
    cfg = bdpt_amd.Config(camera=cam, width=m["width"], height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(os.path.join(REPO, "scenes", "tex", m["obj"])), cfg)
    it.init()
    fb = it.render_frame()
    st = it.stats()
    assert st["kernel"].startswith("bdpt_frame_kernel_tex"), st["kernel"]
    worst = rel_l2(fb, load_golden("tex_T1_texbox_bdpt")).max()
    assert st["schedule_errors"] == 0 and worst <= TOL, worst


@pytest.mark.parametrize("force", [False, True])
def test_gpu_split_build_frame(force, monkeypatch, golden_manifest):
    knob(monkeypatch, force)
    m = golden_manifest["framebuffers"]["G3_hardlight_64x64_spp16"]
    it = integrator(m["scene"], m["width"], m["height"], m["spp"], m["rr_depth"], fresh=True)
    fb = it.render_frame().reshape(-1)
    st = it.stats()
    assert st["kernel"].startswith("bdpt_frame_kernel_split"), st["kernel"]
    worst = rel_l2(fb, load_golden("G3_hardlight_64x64_spp16")).max()
    assert st["schedule_errors"] == 0 and worst <= TOL, worst
