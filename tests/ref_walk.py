"""The reference's BVH query restated in float32 numpy, vectorised over rays: a judge for
traversal tests that needs neither the reference nor a GPU.

It works on the arrays Scene.export() returns (the reference's dump layout): tf[n, 18]
leaf-order triangles (v0 v1 v2, then corner normals), nf[m, 6] node boxes (min, max),
nu[m, 3] = (start, count, right_offset), nodes in preorder, right_offset 0 for a leaf.

What the reference does (bvh.h:259-352, accel.h:27-52, :125-172, core.h:379-400):

* BBox::intersect never writes its tnear, so every child is pushed with mint 0: the left
  child is always popped first and no box is culled by distance (`near > best` can only
  fire for the root, whose mint is min_t). The root's own box is never tested. Nodes are
  therefore met in index (pre)order, triangles in leaf order.
* A triangle is accepted when rayTriangleIntersect passes and t > 1e-3. The closest-hit
  query starts at best = max_t and replaces it on t < best, so among equal t the lowest
  leaf-order index stays. AcceleratorBVH::intersect then reports a hit when
  min_t <= best <= max_t.
* The occlusion query returns at the first accepted triangle with min_t <= t <= max_t;
  when there is none it ends like the closest-hit query: true when anything replaced best.

Every value a decision depends on is float32: numpy float32 arrays divide, multiply and
add in IEEE single precision, one rounding per operation, and comparisons with NaN are
false as in C. The threshold `t > 1e-3` compares a float with a double constant; 1e-3 lies
strictly between float32(1e-3) and the float below it, so it is `t >= float32(1e-3)`.
"""
import numpy as np

f32 = np.float32
EPSILON = f32(1e-8)  # platform.h:57
TRI_MIN_T = f32(1e-3)  # the smallest float32 above the double 1e-3 (see above)


def _cross(ax, ay, az, bx, by, bz):  # glm::cross
    return ay * bz - by * az, az * bx - bz * ax, ax * by - bx * ay


def _dot(ax, ay, az, bx, by, bz):  # glm::dot: (x x' + y y') + z z'
    return (ax * bx + ay * by) + az * bz


def box_hit(lo, hi, o, d):
    """BBox::intersect (bvh.h:33-69) of one box against rays o, d [k, 3]: bool [k]."""
    with np.errstate(all="ignore"):
        tmin, tmax = (lo[0] - o[:, 0]) / d[:, 0], (hi[0] - o[:, 0]) / d[:, 0]
        s = tmin > tmax
        tmin, tmax = np.where(s, tmax, tmin), np.where(s, tmin, tmax)
        tymin, tymax = (lo[1] - o[:, 1]) / d[:, 1], (hi[1] - o[:, 1]) / d[:, 1]
        s = tymin > tymax
        tymin, tymax = np.where(s, tymax, tymin), np.where(s, tymin, tymax)
        ok = ~((tmin > tymax) | (tymin > tmax))
        tmin = np.where(tymin > tmin, tymin, tmin)
        tmax = np.where(tymax < tmax, tymax, tmax)
        tzmin, tzmax = (lo[2] - o[:, 2]) / d[:, 2], (hi[2] - o[:, 2]) / d[:, 2]
        s = tzmin > tzmax
        tzmin, tzmax = np.where(s, tzmax, tzmin), np.where(s, tzmin, tzmax)
        ok &= ~((tmin > tzmax) | (tzmin > tmax))
    return ok


def tri_hit(v0, v1, v2, o, d):
    """rayTriangleIntersect (core.h:379-400) and accel.h:43's t > 1e-3 of one triangle against
    rays o, d [k, 3]: (accepted bool [k], t, u, v float32 [k])."""
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        px, py, pz = _cross(d[:, 0], d[:, 1], d[:, 2], e2[0], e2[1], e2[2])
        det = _dot(e1[0], e1[1], e1[2], px, py, pz)
        ok = ~(np.abs(det) < EPSILON)
        inv = f32(1) / det
        tx, ty, tz = o[:, 0] - v0[0], o[:, 1] - v0[1], o[:, 2] - v0[2]
        u = _dot(tx, ty, tz, px, py, pz) * inv
        ok &= ~((u < 0) | (u > 1))
        qx, qy, qz = _cross(tx, ty, tz, e1[0], e1[1], e1[2])
        v = _dot(d[:, 0], d[:, 1], d[:, 2], qx, qy, qz) * inv
        ok &= ~((v < 0) | (u + v > 1))
        t = _dot(e2[0], e2[1], e2[2], qx, qy, qz) * inv
        ok &= t >= TRI_MIN_T
    for a in (t, u, v):
        assert a.dtype == f32
    return ok, t, u, v


def walk(tf, nf, nu, rays):
    """Both queries of the reference for rays [n, 8] (o, d, min_t, max_t). Returns a dict of
    hit (AcceleratorBVH::intersect's result), t, u, v and tri (the winner's leaf-order index,
    -1: none) of the closest accepted triangle, occluded (the occlusion query's result) and
    ties (how many reachable accepted triangles share the winner's t)."""
    tf, nf, rays = (np.ascontiguousarray(a, f32) for a in (tf, nf, rays))
    n = rays.shape[0]
    o, d, mn, mx = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    best = mx.copy()
    bu, bv = np.zeros(n, f32), np.zeros(n, f32)
    tri = np.full(n, -1, np.int64)
    ties = np.zeros(n, np.int64)
    any_in_range = np.zeros(n, bool)
    reach = {0: np.flatnonzero(~(mn > best))}  # the root's mint is min_t
    zero = f32(0)
    for ni in range(nu.shape[0]):
        act = reach.pop(ni, None)
        if act is None or act.size == 0:
            continue
        if ni:
            act = act[~(zero > best[act])]  # children are pushed with mint 0
        start, count, right = (int(x) for x in nu[ni])
        if right == 0:
            oa, da = o[act], d[act]
            for p in range(start, start + count):
                ok, t, u, v = tri_hit(tf[p, 0:3], tf[p, 3:6], tf[p, 6:9], oa, da)
                any_in_range[act] |= ok & (t <= mx[act]) & (t >= mn[act])
                same = ok & (t == best[act]) & (tri[act] >= 0)
                ties[act[same]] += 1
                win = ok & (t < best[act])
                w = act[win]
                best[w], bu[w], bv[w], tri[w], ties[w] = t[win], u[win], v[win], p, 1
        else:
            oa, da = o[act], d[act]
            for c in (ni + 1, ni + right):
                reach[c] = act[box_hit(nf[c, 0:3], nf[c, 3:6], oa, da)]
    found = tri >= 0
    hit = found & (best <= mx) & (best >= mn)
    return dict(hit=hit, t=best, u=bu, v=bv, tri=tri, occluded=any_in_range | found, ties=np.where(found, ties, 0))


LEAF_BIT, EMPTY_LINK, LDS_STACK = 0x80000000, 0xFFFFFFFF, 7  # wide_bvh.hpp links; dev_traverse.hpp kLdsStack


def wide_walk_stack(wn, wt, root, tf, rays, winners):
    """A host model of the device's 4-wide closest-hit walk (dev_traverse.hpp trav_node_vals / trav_pop /
    cull_far) on the exported traversal tree (Scene.export_traversal()), for counting what the traversal stack
    holds: per ray, the most pending entries at once, and whether the leaf holding triangle winners[i] (a
    leaf-order index, -1: none) was reached by popping an entry from slot >= LDS_STACK, i.e. one that the
    device keeps in its HBM spill column. A node's children that pass the slab test (float64 here: the count
    is a model, not a judge) and the far cull are visited nearest first, the others pushed far to near; a
    popped entry beyond cull_far(best) is dropped. No near cull (the first selection of the per-ray tests).
    Rays with a zero direction component are not walked (the device walks the reference's tree for them):
    their counts are 0."""
    n = rays.shape[0]
    ntri = tf.shape[0]
    ref_idx = wt[:, 0, 3].view(np.uint32).astype(np.int64)
    o32, d32 = np.ascontiguousarray(rays[:, 0:3], f32), np.ascontiguousarray(rays[:, 3:6], f32)
    acc = np.zeros((ntri, n), bool)
    tt = np.zeros((ntri, n), f32)
    for p in range(ntri):
        acc[p], tt[p], _, _ = tri_hit(tf[p, 0:3], tf[p, 3:6], tf[p, 6:9], o32, d32)
    boxes = wn.astype(np.float64)
    links = wn[:, 6].view(np.uint32)
    most = np.zeros(n, np.int64)
    after_spill = np.zeros(n, bool)
    for i in range(n):
        d = rays[i, 3:6].astype(np.float64)
        if np.any(d == 0) or not np.all(np.isfinite(rays[i, :6])) or rays[i, 6] > rays[i, 7]:
            continue
        o, inv = rays[i, 0:3].astype(np.float64), 1.0 / d
        best = float(rays[i, 7])
        far = lambda: abs(best) * 1e-3 + best + 1e-4  # cull_far
        stack, link, from_spill = [], root, False
        while True:
            if link & LEAF_BIT:
                start, count = (link & 0x7FFFFFFF) >> 3, link & 7
                for p in ref_idx[start:start + count]:
                    if p == winners[i] and from_spill:
                        after_spill[i] = True
                    if acc[p, i] and tt[p, i] < best:
                        best = float(tt[p, i])
            else:
                kids = []
                for c in range(4):
                    l = int(links[link, c])
                    if l == EMPTY_LINK:
                        continue
                    t0, t1 = (boxes[link, 0:6:2, c] - o) * inv, (boxes[link, 1:6:2, c] - o) * inv
                    tn, tx = np.minimum(t0, t1).max(), np.maximum(t0, t1).min()
                    if tn <= tx and not tn > far():
                        kids.append((tn, c, l))
                kids.sort()
                if kids:
                    for tn, _, l in reversed(kids[1:]):
                        stack.append((l, tn))
                    most[i] = max(most[i], len(stack))
                    link, from_spill = kids[0][2], from_spill
                    continue
            link = None
            while stack:
                slot = len(stack) - 1
                l, tn = stack.pop()
                if not tn > far():
                    link, from_spill = l, slot >= LDS_STACK
                    break
            if link is None:
                break
    return most, after_spill
