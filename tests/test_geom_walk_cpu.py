"""The float32 restatement of the reference's BVH query (tests/ref_walk.py) and the generated
geometry fixtures (scenes/variants.py GEOM_SCENES, tests/golden/kat_geom_<scene>.npz), on the host.

* The walker equals the unmodified reference bit for bit (hit, t, u, v, shape, prim, occluded) on
  the committed kat_intersect_* and kat_adversarial_* goldens and on every kat_geom_* golden: that
  licenses it as the judge of rays drawn at test time (tests/test_gpu_kat_geometry.py).
* On every generated scene the product's exported reference tree equals the oracle's, bit for bit,
  and both traversal trees meet test_traversal_tree_cpu.py's preconditions.
* The fixtures are not vacuous, judged by the reference's recorded results alone.
"""
import os

import numpy as np
import pytest

import bdpt_amd
import geom_rays
import oracle as O
import ref_walk
import variants
from test_traversal_tree_cpu import check_tree

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}

# (scene, kind) pairs that cannot hit by construction (at most the rounding noise of a coplanar,
# grazing query, which the reference accepts now and then, gives one a hit):
#  - tiny1 holds one triangle: a ray leaving it, or a segment between two of its points, meets nothing else;
#  - tiny2 has nothing between its two surfaces (a floor half under the emitter).
CANNOT_HIT = {("tiny1", "shadow"), ("tiny1", "surface"), ("tiny2", "shadow")}
CANNOT_MISS = set()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exported(name, tmp_root):
    """(Scene, (tf, ti, nf, nu), obj path) of a catalogue or generated scene, loaded once."""
    if name not in _cache:
        path = (variants.geom_obj(name, str(tmp_root.mktemp("geom_" + name))) if name in variants.GEOM_SCENES
                else variants.obj_path(name))
        s = bdpt_amd.Scene(path)
        _cache[name] = (s, s.export(), path)
    return _cache[name]


def assert_walk_equals(w, ti, hit, t, u, v, shape, prim, occluded, what):
    bad = np.flatnonzero(w["hit"] != (hit == 1))
    assert bad.size == 0, f"{what}: {bad.size} acceptance mismatches, first ray {bad[:5]}"
    k = hit == 1
    for name, a, b in (("t", w["t"], t), ("u", w["u"], u), ("v", w["v"], v)):
        bad = np.flatnonzero(bits(a[k]) != bits(b[k]))
        assert bad.size == 0, f"{what}: {name} differs on {bad.size} hits"
    assert np.array_equal(ti[w["tri"][k], 0], shape[k]), f"{what}: shape"
    assert np.array_equal(ti[w["tri"][k], 1], prim[k]), f"{what}: prim"
    bad = np.flatnonzero(w["occluded"] != (occluded == 1))
    assert bad.size == 0, f"{what}: {bad.size} occlusion mismatches, first ray {bad[:5]}"


@pytest.mark.parametrize("scene", ["caustic", "hardlight", "cbox_low"])
def test_walker_equals_reference_on_intersect_goldens(scene, tmp_path_factory):
    g = np.load(os.path.join(GOLD, f"kat_intersect_{scene}.npz"))
    _, (tf, ti, nf, nu), _ = exported(scene, tmp_path_factory)
    ref = g["out"]
    w = ref_walk.walk(tf, nf, nu, g["rays"])
    assert_walk_equals(w, ti, ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3], ref[:, 4].view(np.int32),
                       ref[:, 5].view(np.int32), ref[:, 20], scene)
    k = ref[:, 0] == 1
    assert np.array_equal(ti[w["tri"][k], 2], ref[k, 6].view(np.int32))


@pytest.mark.parametrize("scene", ["caustic", "hardlight"])
def test_walker_equals_reference_on_adversarial_goldens(scene, tmp_path_factory):
    g = np.load(os.path.join(GOLD, f"kat_adversarial_{scene}.npz"))
    _, (tf, ti, nf, nu), _ = exported(scene, tmp_path_factory)
    w = ref_walk.walk(tf, nf, nu, g["rays"])
    assert_walk_equals(w, ti, g["hit"], g["t"], g["u"], g["v"], g["shape"], g["prim"], g["occluded"], scene)


@pytest.mark.parametrize("scene", list(variants.GEOM_SCENES))
def test_walker_equals_reference_on_generated_goldens(scene, tmp_path_factory):
    g = np.load(os.path.join(GOLD, f"kat_geom_{scene}.npz"))
    _, (tf, ti, nf, nu), path = exported(scene, tmp_path_factory)
    assert variants.file_sha256(path) == str(g["obj_sha256"]), "the generated OBJ text differs from the recorded one"
    ref = g["out"]
    w = ref_walk.walk(tf, nf, nu, g["rays"])
    assert_walk_equals(w, ti, ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3], ref[:, 4].view(np.int32),
                       ref[:, 5].view(np.int32), ref[:, 20], scene)
    k = ref[:, 0] == 1
    assert np.array_equal(ti[w["tri"][k], 2], ref[k, 6].view(np.int32))


def test_walker_decides_in_float32():
    """No float64 on the decision path: float64 inputs are narrowed first, every intermediate of the
    triangle test is float32 (asserted inside tri_hit), and a box test's NaN (0 / 0 on a flat axis)
    passes as in C."""
    rays = np.array([[0.5, 0.0, 0.5, 1.0, 0.0, 0.0, 1e-8, 3e38]], np.float64)
    lo, hi = np.array([0, 0, 0], np.float32), np.array([1, 0, 1], np.float32)
    r = rays.astype(np.float32)
    assert ref_walk.box_hit(lo, hi, r[:, 0:3], r[:, 3:6])[0]
    ok, t, u, v = ref_walk.tri_hit(np.float32([0, -1, 0]), np.float32([0, 1, 1]), np.float32([0, 1, -1]) + 0,
                                   r[:, 0:3] * 0 + np.float32([-1, 0, 0]), r[:, 3:6])
    assert t.dtype == u.dtype == v.dtype == np.float32 and ok[0] and t[0] == 1


@pytest.mark.parametrize("scene", list(variants.GEOM_SCENES))
def test_generated_scene_trees(scene, tmp_path_factory, monkeypatch):
    s, ex, path = exported(scene, tmp_path_factory)
    for a, b in zip(ex, O.Scene(path).dump()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    info = s.info()
    assert info["emitters"] == 1 and info["triangles"] <= 600
    check_tree(s, tri_tree=True)
    monkeypatch.setenv("BDPT_TRAV_TREE", "refleaf")
    r = bdpt_amd.Scene(path)
    check_tree(r, tri_tree=False)
    # inside the reference's fixed stacks: 64 traversal entries (bvh.h:269), 128 build entries (bvh.h:149)
    assert info["bvh_max_depth"] + 2 <= 64
    if scene in ("tiny1", "tiny2", "tiny4"):
        assert info["bvh_nodes"] == 1  # the root is the only leaf: no box is ever tested
    if scene == "tiny5":
        assert info["bvh_nodes"] == 3 and info["bvh_leaves"] == 2  # the first split
    if scene == "flat":
        _, _, nf, nu = ex
        assert np.any((nf[:, 1] == 0) & (nf[:, 4] == 0) & (nu[:, 2] != 0))  # zero-thick interior boxes
    if scene == "chain":
        assert info["bvh_max_depth"] >= 40
        assert info["wide_depth"] > 7 and r.info()["wide_depth"] > 7  # past the LDS stack (kLdsStack = 7)
        assert info["wide_max_stack"] > 7 and r.info()["wide_max_stack"] > 7


@pytest.mark.parametrize("family", list(variants.GEOM_FAMILIES))
def test_generated_goldens_are_not_vacuous(family, tmp_path_factory):
    """Read from the goldens: the judge is the reference, not the code under test. Only the count of
    triangles at the winner's t comes from the walker (the reference reports one winner)."""
    hits, rays_n = 0, 0
    shared_hits, shared_ties = 0, 0
    for scene in variants.GEOM_FAMILIES[family]:
        g = np.load(os.path.join(GOLD, f"kat_geom_{scene}.npz"))
        hit, kind = g["out"][:, 0] == 1, g["kind"]
        assert 1900 <= hit.size <= 2100
        assert 0.2 <= hit.mean() <= 0.8, (scene, hit.mean())
        hits, rays_n = hits + int(hit.sum()), rays_n + hit.size
        for k in np.unique(kind):
            name = geom_rays.KINDS[k]
            m = kind == k
            assert (scene, name) in CANNOT_HIT or hit[m].any(), (scene, name, "no hit")
            assert (scene, name) in CANNOT_MISS or not hit[m].all(), (scene, name, "no miss")
        tie_kinds = np.ones_like(hit) if family == "dupes" else kind == geom_rays.K_SHARED_EXACT
        if tie_kinds.any():
            _, (tf, _, nf, nu), _ = exported(scene, tmp_path_factory)
            w = ref_walk.walk(tf, nf, nu, g["rays"])
            sel = tie_kinds & hit
            shared_hits += int(sel.sum())
            shared_ties += int((w["ties"][sel] >= 2).sum())
    assert 0.2 <= hits / rays_n <= 0.8
    if family in ("tiny", "flat", "dupes"):
        assert shared_hits >= 100 and shared_ties >= 0.9 * shared_hits, (shared_hits, shared_ties)


def test_slivers_straddle_the_stated_corner_limit(tmp_path_factory):
    """dev_traverse.hpp names ~0.35 degrees as the corner below which the near cull's argument fails."""
    _, (tf, _, _, _), _ = exported("slivers", tmp_path_factory)
    v = tf[:, :9].reshape(-1, 3, 3).astype(np.float64)
    small = np.full(v.shape[0], 180.0)
    for c in range(3):
        a, b = v[:, (c + 1) % 3] - v[:, c], v[:, (c + 2) % 3] - v[:, c]
        sin = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        cos = np.sum(a * b, 1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        small = np.minimum(small, np.degrees(np.arctan2(sin, cos)))
    assert (small > 0.35).sum() >= 10 and (small < 0.05).sum() >= 30 and small.min() < 0.002 and small.max() > 0.5


def test_slivers_golden_reaches_the_near_culls_stated_limit(tmp_path_factory):
    """The regime dev_traverse.hpp's comment on kGrazeCos names: a ray leaving a sliver at |cos| >= 0.02 to
    its plane (the near cull is on) whose origin triangle the reference itself reports as the hit, because
    the triangle test's t there is rounding noise above 1e-3. Read from the golden."""
    g = np.load(os.path.join(GOLD, "kat_geom_slivers.npz"))
    _, (_, ti, _, _), _ = exported("slivers", tmp_path_factory)
    ref, otri = g["out"], g["otri"]
    left = otri >= 0
    cos = np.abs(np.sum(g["rays"][:, 3:6].astype(np.float64) * g["onrm"], axis=1))
    own = left & (ref[:, 0] == 1)
    own[left] &= ((ref[left, 4].view(np.int32) == ti[otri[left], 0]) & (ref[left, 5].view(np.int32) == ti[otri[left], 1]))
    assert (own & (cos >= 0.02)).sum() >= 10, int((own & (cos >= 0.02)).sum())


@pytest.mark.parametrize("tree", ["", "refleaf"])
def test_chain_golden_rays_spill_the_lds_stack(tree, tmp_path_factory, monkeypatch):
    """That the chain trees CAN hold more than kLdsStack = 7 entries is a bound; this counts, on a host model of
    the device's 4-wide walk in its push order (ref_walk.wide_walk_stack), how many of the golden's rays DO, and
    for how many the reference's winner sits in a leaf reached through an entry popped from a spilled slot
    (so a wrong spill read changes the result the per-ray tests compare)."""
    g = np.load(os.path.join(GOLD, "kat_geom_chain.npz"))
    _, (tf, ti, _, _), path = exported("chain", tmp_path_factory)
    if tree:
        monkeypatch.setenv("BDPT_TRAV_TREE", tree)
    wn, wt, _, root = bdpt_amd.Scene(path).export_traversal()
    ref, kind, rays = g["out"], g["kind"], g["rays"]
    hit = ref[:, 0] == 1
    index_of = {(int(s), int(p)): k for k, (s, p) in enumerate(ti[:, :2])}
    shape, prim = ref[:, 4].view(np.int32), ref[:, 5].view(np.int32)
    winners = np.array([index_of[(int(shape[i]), int(prim[i]))] if hit[i] else -1 for i in range(hit.size)])
    most, after_spill = ref_walk.wide_walk_stack(wn, wt, root, tf, rays, winners)
    walked = (kind != geom_rays.K_FAR) & np.all(rays[:, 3:6] != 0, axis=1)  # the others walk the reference's tree
    share = (most[walked] > ref_walk.LDS_STACK).mean()
    n_after = int(after_spill[walked & hit].sum())
    print(f"chain {tree or 'default'}: {share:.1%} of {int(walked.sum())} walked rays hold more than 7 entries "
          f"(most {most.max()}); {n_after} of {int((walked & hit).sum())} winners reached through a spilled entry")
    assert share >= 0.05 and most.max() >= 16 and n_after >= 25
