"""The walk's leaf triangles fetched in pairs (dev_traverse.hpp wleaf_tests,
BDPT_WLEAF_GROUP = 2): the same decisions in the same order as one triangle at a
time.

* The per-function intersect entry point (the one tests/test_gpu_kat.py drives) on
  cbox_low, with rays aimed at every triangle of every traversal leaf
  (tests/golden/make_leaf_group_golden.py): leaves of 1, 2, 3 and 4 triangles, the
  leaf that ends the triangle array (an odd count: its last pair's second load is
  clamped to the last triangle), closest hits and occlusion queries whose hit is the
  first or the second triangle of a pair. Every hit field bit for bit against the
  reference's answer. That the ray set holds these cases is asserted from the host
  tree (Scene.export_traversal) and a float64 triangle test, without the GPU.
  (The C oracle exports no ray query; as in test_gpu_kat.py the expected values are
  the reference binary's, recorded in tests/golden/kat_leaf_group_cbox_low.npz.)
* The counting pass at Caustic 64^2 x 16: tri_tests and interior_visits equal those
  of the group-size-1 build (lib/libbdpt_amd_wleaf1.so, run in a process of its own:
  a process loads one build), and the counters tests/test_gpu_counters.py pins equal
  the oracle's.
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

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_BIT, EMPTY = 0x80000000, 0xFFFFFFFF
SCENE = "cbox_low"
TRI_MIN_T = 1e-3  # accel.h:43: hits at t <= 1e-3 are not accepted
_cache = {}


def fixture():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(GOLD, f"kat_leaf_group_{SCENE}.npz")))
    return _cache["g"]


def host_tree():
    """(wtri, per-triangle leaf start, leaf count, position in leaf, wtri position of reference index)."""
    if "tree" not in _cache:
        wn, wt, _, root = bdpt_amd.Scene(variants.obj_path(SCENE)).export_traversal()
        n = wt.shape[0]
        start, count = np.full(n, -1), np.zeros(n, np.int64)

        def walk(link):
            if link & LEAF_BIT:
                s, c = (link & 0x7FFFFFFF) >> 3, link & 7
                assert 1 <= c <= 4 and s + c <= n
                start[s:s + c], count[s:s + c] = s, c
                return
            for child in wn[link][6].view(np.uint32):
                if child != EMPTY:
                    walk(int(child))

        walk(root)
        assert np.all(start >= 0)
        pos_of_ref = np.empty(n, np.int64)
        pos_of_ref[wt[:, 0, 3].view(np.uint32).astype(np.int64)] = np.arange(n)
        _cache["tree"] = (wt, start, count, np.arange(n) - start, pos_of_ref)
    return _cache["tree"]


def hits_f64(rays, wt):
    """t[ray, triangle] of the two-sided ray-triangle test in float64 (inf: no hit inside [min_t, max_t]
    or at t <= 1e-3), with the barycentrics kept 1e-6 inside the edges so that no hit counted here is a
    rounding case of the float32 test."""
    o, d = rays[:, None, 0:3].astype(np.float64), rays[:, None, 3:6].astype(np.float64)
    v0, e1, e2 = (wt[None, :, j, :3].astype(np.float64) for j in range(3))
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1)
        v = (d * q).sum(-1) * inv
        t = (e2 * q).sum(-1) * inv
        eps = 1e-6
        ok = (np.abs(det) > 1e-12) & (u > eps) & (v > eps) & (u + v < 1 - eps) & (t > TRI_MIN_T)
        ok &= (t >= rays[:, None, 6]) & (t <= rays[:, None, 7])
    return np.where(ok, t, np.inf)


def coverage():
    """The aimed rays whose case the host can vouch for: kind 0 rays whose closest float64 hit is the
    targeted triangle, clear of any other by 1e-3; kind 1 segments that cross the targeted triangle and
    no other triangle of the scene. Returns per case the leaf (start, count) and the position in it."""
    if "cov" in _cache:
        return _cache["cov"]
    g = fixture()
    wt, start, count, k_in_leaf, pos_of_ref = host_tree()
    out = {}
    for kind in (0, 1):
        sel = np.flatnonzero(g["kind"] == kind)
        t = hits_f64(g["rays"][sel], wt)
        pos = pos_of_ref[g["target"][sel]]
        rows = np.arange(len(sel))
        t_target = t[rows, pos]
        others = t.copy()
        others[rows, pos] = np.inf
        if kind == 0:
            good = np.isfinite(t_target) & (others.min(1) > t_target + 1e-3)
            good &= g["out"][sel, 0] == 1  # the reference accepts a hit
        else:
            good = np.isfinite(t_target) & np.isinf(others.min(1))
            good &= g["out"][sel, 20] == 1  # the reference reports the segment occluded
        p = pos[good]
        out[kind] = dict(start=start[p], count=count[p], k=k_in_leaf[p], n=len(sel))
    _cache["cov"] = out
    return out


def test_ray_set_meets_every_leaf_shape_and_both_pair_positions():
    """Host only: without these cases in the fixture the GPU comparison below would pass vacuously."""
    wt = host_tree()[0]
    n = wt.shape[0]
    cov = coverage()
    for kind in (0, 1):
        c = cov[kind]
        assert len(c["k"]) >= 0.9 * c["n"], (kind, len(c["k"]), c["n"])
        assert set(np.unique(c["count"])) == {1, 2, 3, 4}, np.unique(c["count"])
        # every position of every leaf size: the first and the second triangle of a pair, an odd
        # count's lone last triangle (whose pair partner is the clamped load)
        for cnt in (1, 2, 3, 4):
            assert set(np.unique(c["k"][c["count"] == cnt])) == set(range(cnt)), (kind, cnt)
        ends = c["start"] + c["count"] == n  # the leaf that ends the triangle array
        assert ends.any()
        last_count = int(c["count"][ends][0])
        assert set(c["k"][ends]) == set(range(last_count))
    # occlusion queries that end at the first / at the second triangle of a pair
    k1 = cov[1]["k"]
    assert (k1 % 2 == 0).sum() > 100 and (k1 % 2 == 1).sum() > 100
    # an odd leaf ends the array in this tree: the clamped load is the array's last record
    assert int(cov[0]["count"][cov[0]["start"] + cov[0]["count"] == n][0]) % 2 == 1


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_intersect_on_every_leaf_matches_reference():
    test_ray_set_meets_every_leaf_shape_and_both_pair_positions()
    g = fixture()
    cam = bdpt_amd.Camera(**variants.SCENES[SCENE]["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=64, height=64, spp=1, rr_depth=variants.SCENES[SCENE]["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(SCENE)), cfg)
    it.init()
    ref = g["out"]
    h = it.intersect(g["rays"])
    bad = np.flatnonzero(h["hit"] != ref[:, 0].astype(np.int32))
    assert bad.size == 0, f"{bad.size} acceptance mismatches, kinds {np.bincount(g['kind'][bad])}"
    k = ref[:, 0] == 1
    r, hh = ref[k], h[k]
    assert same_bits(hh["t"], r[:, 1]) and same_bits(hh["u"], r[:, 2]) and same_bits(hh["v"], r[:, 3])
    assert np.array_equal(hh["shape_id"], r[:, 4].view(np.int32))
    assert np.array_equal(hh["prim_id"], r[:, 5].view(np.int32))
    assert np.array_equal(hh["mat_id"], r[:, 6].view(np.int32))
    assert same_bits(hh["p"], r[:, 7:10]) and same_bits(hh["ns"], r[:, 10:13])
    assert same_bits(hh["ng"], r[:, 13:16]) and same_bits(hh["wo"], r[:, 16:19])
    occ = it.intersect(g["rays"], occlusion=True)
    bad = np.flatnonzero(occ["hit"] != ref[:, 20].astype(np.int32))
    assert bad.size == 0, f"{bad.size} occlusion mismatches, kinds {np.bincount(g['kind'][bad])}"


CASE = ("caustic", 64, 64, 16, 8)  # tests/test_gpu_task_ring.py's shape
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
                             "counters": {k: int(v) for k, v in st["counters"].items()}}))
"""


@pytest.mark.gpu
def test_gpu_counting_pass_equals_group_1_build_and_oracle():
    name, W, H, spp, rr = CASE
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[name]["camera"]), width=W, height=H, spp=spp,
                          rr_depth=rr)
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
    it.init()
    it.render_frame(flags=bdpt_amd.FLAG_COUNT)
    st = it.stats()
    g = st["counters"]

    lib1 = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "libbdpt_amd_wleaf1.so")
    assert os.path.exists(lib1), f"{lib1} is missing: build() makes it"
    env = dict(os.environ, BDPT_AMD_LIB=lib1)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "bidirectional-path-tracing_amd"),
                                         os.path.join(REPO, "scenes")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, "-c", COUNT_SCRIPT, json.dumps(CASE)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    one = json.loads([line for line in p.stdout.splitlines() if line.startswith("COUNTS ")][-1][7:])
    assert one["lib"] == lib1 and one["kernel"] == st["kernel"] and one["samples"] == st["samples"]
    print(f"{st['kernel']}: tri_tests {g['tri_tests']} interior_visits {g['interior_visits']} "
          f"(group 1: {one['counters']['tri_tests']} {one['counters']['interior_visits']})")
    for k in ("tri_tests", "interior_visits", "closest_rays", "shadow_rays", "slab_fallbacks"):
        assert int(g[k]) == one["counters"][k], (k, int(g[k]), one["counters"][k])

    # tests/test_gpu_counters.py's equality with the oracle
    p_ = O.make_params(variants.SCENES[name]["camera"], W, H, spp, rr)
    O.counters(True)
    _, n_ref = O.Scene(variants.obj_path(name)).render(p_)
    o = O.counters(True)
    assert st["samples"] == n_ref == W * H * spp
    assert o["eye_retraces"] > 0
    pairs = {k: (g[k], o[k]) for k in ("rng_draws", "light_verts", "light_vert_reads", "shadow_rays", "splats")}
    pairs["closest_rays"] = (g["closest_rays"], o["closest_rays"] - o["eye_retraces"])
    bad = {k: v for k, v in pairs.items() if v[0] != v[1]}
    assert not bad, f"{st['kernel']}: counters differ from the oracle's (gpu, oracle): {bad}"
