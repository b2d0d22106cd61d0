"""Makes tests/golden/kat_leaf_group_cbox_low.npz for tests/test_gpu_leaf_group.py.

Rays aimed at every triangle of every traversal leaf of cbox_low (leaves of 1, 2,
3 and 4 triangles; the last leaf, of 3, ends the triangle array), so that the walk
tests each leaf with its hit at every position of a pair:

  kind 0  from 0.02 in front of the triangle's centroid along its normal, towards
          it, [Epsilon, FLT_MAX]: the closest hit is that triangle
  kind 1  the same start, the segment [Epsilon, 0.04]: it crosses that triangle and
          no other, so an occlusion query ends at that triangle's position in its leaf
  kind 2  make_kat_goldens.scene_rays (camera rays, rays inside the box, segments)

`out` is the reference's answer for each ray (oracle/_ref/ref_bdpt, kat mode
`intersect`, as kat_intersect_<scene>.npz: AcceleratorBVH::intersect's fields and
the occlusion query); `target` the reference leaf-order index of the triangle a
ray of kind 0 / 1 is aimed at (-1 for kind 2).

    python tests/golden/make_leaf_group_golden.py     (after build(): needs oracle/_ref/ref_bdpt)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_kat_goldens as K  # noqa: E402

sys.path.insert(0, os.path.join(K.REPO, "bidirectional-path-tracing_amd"))
import bdpt_amd  # noqa: E402  (host-only scene ingest)

SCENE, OFFSET, N_RANDOM = "cbox_low", 0.02, 1200
FLT_MAX = 3.402823466e38


def main():
    s = bdpt_amd.Scene(K.variants.obj_path(SCENE))
    _, wt, _, _ = s.export_traversal()
    v0 = wt[:, 0, :3].astype(np.float64)
    e1, e2 = wt[:, 1, :3].astype(np.float64), wt[:, 2, :3].astype(np.float64)
    ref_idx = wt[:, 0, 3].view(np.uint32).astype(np.int32)
    c = v0 + (e1 + e2) / 3.0
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    o = c + OFFSET * n
    m = len(c)
    one = np.ones((m, 1))
    aimed = np.concatenate([o, -n, 1e-8 * one, FLT_MAX * one], 1)
    seg = np.concatenate([o, -n, 1e-8 * one, 2 * OFFSET * one], 1)
    rnd = K.scene_rays(np.random.default_rng(77), SCENE, N_RANDOM)
    rays = np.concatenate([aimed, seg, rnd]).astype(np.float32)
    kind = np.concatenate([np.zeros(m), np.ones(m), np.full(len(rnd), 2)]).astype(np.int8)
    target = np.concatenate([ref_idx, ref_idx, np.full(len(rnd), -1)]).astype(np.int32)
    out = K.kat(K.toml(SCENE), 64, 64, "intersect", rays, 21)
    path = os.path.join(HERE, f"kat_leaf_group_{SCENE}.npz")
    np.savez_compressed(path, rays=rays, out=out, kind=kind, target=target)
    print(path, len(rays), "rays, hits", int(out[:, 0].sum()), "occluded", int(out[:, 20].sum()),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
