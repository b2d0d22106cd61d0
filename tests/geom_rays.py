"""Seeded rays for the generated geometry families (scenes/variants.py GEOM_SCENES): the kinds
tests/golden/make_kat_goldens.py `generated` records the reference on (kat_geom_<scene>.npz) and
tests/test_gpu_kat_geometry.py draws again from another seed for tests/ref_walk.py to judge.

Only the float32 rays matter; how they are drawn (float64 numpy) decides nothing."""
import numpy as np

f32 = np.float32
FLT_MAX = 3.402823466e38
KINDS = ["random", "camera", "shadow", "axis1", "axis2", "inplane", "offplane", "shared_exact", "shared_oblique",
         "surface", "near_threshold", "far", "sliver_graze", "mid_far"]
(K_RANDOM, K_CAMERA, K_SHADOW, K_AXIS1, K_AXIS2, K_INPLANE, K_OFFPLANE, K_SHARED_EXACT, K_SHARED_OBLIQUE, K_SURFACE,
 K_NEAR, K_FAR, K_SLIVER_GRAZE, K_MID) = range(len(KINDS))
# |cos| of the rays that leave the thinnest slivers (kind "sliver_graze"): at and above kGrazeCos, where the near
# cull is on and Moller-Trumbore's t on the origin triangle is rounding noise the reference may accept
SLIVER_COS = [0.02, 0.021, 0.025, 0.03, 0.04, 0.05, 0.07, 0.1]
# |cos| to the plane normal of the rays that leave a surface (kind "surface"), around dev_traverse.hpp kGrazeCos
SURFACE_COS = [1.0, 0.7, 0.3, 0.1, 0.05, 0.03, 0.021, 0.019, 0.01, 3e-3, 1e-3, 3e-4, 1e-4]


def _normalize(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _unit(rng, n):
    return _normalize(rng.normal(size=(n, 3)))


def _bary(rng, n, edges=True):
    u = rng.random(n).astype(f32)
    v = (rng.random(n) * (1 - u)).astype(f32)
    if edges:
        k = rng.random(n)
        u[k < 0.1] = 0
        v[(k >= 0.1) & (k < 0.2)] = 0
        e = (k >= 0.2) & (k < 0.3)
        v[e] = (f32(1) - u[e]).astype(f32)
        c = (k >= 0.3) & (k < 0.35)
        u[c], v[c] = 0, 0
    return u, v


def surface_points(rng, tri, cnrm, idx, edges=True):
    """Points on triangles idx as the path computes hit points ((v0 w + v1 u) + v2 v in float32), a share
    exactly on edges and vertices, and the interpolated shading normals there."""
    u, v = _bary(rng, idx.size, edges)
    w = (f32(1) - u - v).astype(f32)
    p = ((tri[idx, 0:3] * w[:, None] + tri[idx, 3:6] * u[:, None]) + tri[idx, 6:9] * v[:, None]).astype(f32)
    sn = ((cnrm[idx, 0:3] * w[:, None] + cnrm[idx, 3:6] * u[:, None]) + cnrm[idx, 6:9] * v[:, None]).astype(f32)
    with np.errstate(all="ignore"):
        sn = (sn / np.sqrt(np.sum(sn * sn, 1, keepdims=True, dtype=f32))).astype(f32)
    return p, sn


def geometry_rays(scene, tf, nf, eye, n, seed):
    """Rays for the generated scene `scene` (a GEOM_SCENES name), from its exported triangles tf and
    node boxes nf. Returns (rays [n', 8] float32, kind [n'], the plane normal of the triangle a ray
    leaves [n', 3] (0: none), that triangle [n'] (-1: none), the shading normal held there [n', 3])."""
    rng = np.random.default_rng(seed)
    tri, cnrm = tf[:, :9].astype(f32), tf[:, 9:18].astype(f32)
    ntri = tri.shape[0]
    e1, e2 = (tri[:, 3:6] - tri[:, 0:3]).astype(np.float64), (tri[:, 6:9] - tri[:, 0:3]).astype(np.float64)
    ng = np.cross(e1, e2)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    lo, hi = nf[0, :3].astype(np.float64), nf[0, 3:].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    # where the detail is: the box of the triangles no larger than 20 x the median extent
    ext = np.max(tri.reshape(ntri, 3, 3).max(1) - tri.reshape(ntri, 3, 3).min(1), axis=1)
    small = ext <= 20 * np.median(ext)
    flo, fhi = tri[small].reshape(-1, 3).min(0).astype(np.float64), tri[small].reshape(-1, 3).max(0).astype(np.float64)
    fhi = np.maximum(fhi, flo + 1e-3 * max(float(np.linalg.norm(fhi - flo)), 1e-6))
    eye = np.asarray(eye, np.float64)
    family = scene.rstrip("0123456789")
    kinds = [K_RANDOM, K_CAMERA, K_SHADOW, K_AXIS1, K_AXIS2, K_SHARED_OBLIQUE, K_SURFACE, K_NEAR, K_FAR, K_MID]
    if family == "flat":
        kinds += [K_INPLANE, K_OFFPLANE]
    if family in ("flat", "dupes") or scene in ("tiny4", "tiny5"):
        kinds += [K_SHARED_EXACT]
    if family == "slivers":
        kinds += [K_SLIVER_GRAZE]
    weight = {K_SURFACE: 2.0, K_SLIVER_GRAZE: 2.0, K_MID: 2.0, K_NEAR: 1.5 if family in ("scales", "flat") else 0.5, K_INPLANE: 0.5, K_OFFPLANE: 0.5}
    tot = sum(weight.get(k, 1.0) for k in kinds)
    out, kind, onrm, otri, osn = [], [], [], [], []

    def add(o, d, mn, mx, tag, idx=None, sn=None):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.linalg.norm(d, axis=1) > 0)
        mn = np.broadcast_to(np.asarray(mn, np.float64), ok.shape)[ok]
        mx = np.broadcast_to(np.asarray(mx, np.float64), ok.shape)[ok]
        m = int(ok.sum())
        out.append(np.concatenate([o[ok].astype(f32), _normalize(d[ok]), mn[:, None].astype(f32),
                                   mx[:, None].astype(f32)], 1))
        kind.append(np.full(m, tag, np.int32))
        onrm.append(np.zeros((m, 3), f32) if idx is None else ng[idx][ok].astype(f32))
        otri.append(np.full(m, -1, np.int32) if idx is None else idx[ok].astype(np.int32))
        osn.append(np.zeros((m, 3), f32) if sn is None else sn[ok].astype(f32))

    # rayTriangleIntersect rejects |det| < 1e-8, and |det| <= 2 area for a unit direction: triangles below
    # that (the deep end of `chain`) are in the tree but no ray can hit them, so most picks go to the others
    hittable = np.flatnonzero(np.linalg.norm(np.cross(e1, e2), axis=1) >= 1e-7)

    def pick(k):
        return np.where(rng.random(k) < 0.85, hittable[rng.integers(0, hittable.size, k)], rng.integers(0, ntri, k))

    def box_points(k):
        focus = (rng.random(k) < 0.5)[:, None]
        a = np.where(focus, flo, lo - 0.05 * (hi - lo))
        b = np.where(focus, fhi, hi + 0.05 * (hi - lo))
        return a + rng.random((k, 3)) * (b - a)

    def targets(k, share=0.6, scale=False):
        """Surface points of random triangles (every triangle alike, whatever its size) or box points;
        with scale also a length of the target's own size (its triangle's extent, or the scene's)."""
        idx = pick(k)
        p, _ = surface_points(rng, tri, cnrm, idx)
        surf = rng.random(k) < share
        pts = np.where(surf[:, None], p.astype(np.float64), box_points(k))
        return (pts, np.where(surf, ext[idx].astype(np.float64), diag)) if scale else pts

    def origins_for(tgt, size):
        """Half anywhere in the boxes, half a few target sizes from the target (detail far smaller than
        the scene is only met from nearby: a float32 direction resolves ~1e-7 of the distance), but not
        so near that t > 1e-3 rejects the target."""
        k = tgt.shape[0]
        near = tgt + _unit(rng, k).astype(np.float64) * np.maximum(size * rng.uniform(1.0, 6.0, k), rng.uniform(1.2e-3, 4e-3, k))[:, None]
        return np.where((rng.random(k) < 0.5)[:, None], near, box_points(k))

    def shared_points(k):
        """Vertices, edge midpoints and (a few) interior points of random triangles."""
        idx = pick(k)
        c = rng.integers(0, 3, k)
        a = tri.reshape(ntri, 3, 3)[idx, c].astype(np.float64)
        b = tri.reshape(ntri, 3, 3)[idx, (c + 1) % 3].astype(np.float64)
        w = rng.choice([0.0, 0.5, 0.25], k)[:, None]  # exact in float32 for the dyadic grids
        return a + (b - a) * w

    for tag in kinds:
        k = max(8, int(round(n * weight.get(tag, 1.0) / tot)))
        if tag == K_RANDOM:
            tgt, size = targets(k, scale=True)
            o = origins_for(tgt, size)
            add(o, tgt - o, 1e-8, FLT_MAX, tag)
        elif tag == K_CAMERA:  # min_t 1, max_t 1000: renderer.cpp:192
            add(np.repeat(eye[None], k, 0), targets(k, 0.7) - eye, 1.0, 1000.0, tag)
        elif tag == K_SHADOW:  # visibilityQuery: [Epsilon, dist - 1e-5], bdpt.h:498-505
            idx = pick(k)
            a, sn = surface_points(rng, tri, cnrm, idx)
            b = targets(k)
            b = np.where((rng.random(k) < 0.3)[:, None], a + (b - a) * 1.5, b)  # a share runs on through its target
            dd = (b.astype(f32) - a).astype(f32)
            dist = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).astype(f32)
            keep = dist > 1e-4
            add(a[keep], dd[keep], 1e-8, (dist[keep] - f32(1e-5)).astype(f32), tag, idx[keep], sn[keep])
        elif tag in (K_AXIS1, K_AXIS2):  # one / two zero direction components, half of them aimed at a surface
            dirn = np.zeros((k, 3))
            ax = rng.integers(0, 3, k)
            dirn[np.arange(k), ax] = rng.choice([-1.0, 1.0], k)
            if tag == K_AXIS1:
                dirn[np.arange(k), (ax + 1) % 3] = rng.normal(size=k)
            dirn = _normalize(dirn).astype(np.float64)
            tgt, size = targets(k, 1.0, scale=True)
            s = np.where(rng.random(k) < 0.5, np.maximum(size * rng.uniform(0.5, 6.0, k), rng.uniform(1.2e-3, 4e-3, k)),
                         np.exp(rng.uniform(np.log(2e-3), np.log(max(diag, 1.0)), k)))[:, None]
            o = np.where((rng.random(k) < 0.7)[:, None], tgt - dirn * s, box_points(k))
            add(o, dirn, 1e-8, FLT_MAX, tag)
        elif tag in (K_INPLANE, K_OFFPLANE):  # flat: in the grid's plane y = 0 (0 / 0 in its boxes' slab test) / just off it
            o = rng.uniform(-1.5, 1.5, (k, 3))
            o = np.where(rng.random((k, 3)) < 0.4, np.round(o * 4) / 4, o)  # some coordinates on the grid lines
            phi = rng.random(k) * 2 * np.pi
            dirn = np.stack([np.cos(phi), np.zeros(k), np.sin(phi)], 1)
            grid = rng.random(k) < 0.4  # along the grid lines: the shared edges themselves
            dirn[grid] = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0]])[rng.integers(0, 4, int(grid.sum()))]
            o[:, 1] = 0.0 if tag == K_INPLANE else rng.choice([1e-7, 1e-6, 1e-5, 1e-4, 1e-3], k) * rng.choice([-1, 1], k)
            add(o, dirn, 1e-8, np.where(rng.random(k) < 0.5, FLT_MAX, 1.0), tag)
        elif tag == K_SHARED_EXACT:  # axis-parallel rays straight at shared vertices / edges / duplicates: exact ties
            if family == "dupes":
                p = targets(k, 1.0)
            elif family == "tiny":  # the diagonal the two floor halves share
                x = rng.integers(-8, 9, k) / 8.0
                p = np.stack([x, np.zeros(k), x], 1)
            else:
                p = shared_points(k)
            dirn = np.zeros((k, 3))
            if family == "dupes":
                dirn[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
            else:
                dirn[:, 1] = -1.0  # the flat grid and the tiny floor lie in y = 0
                p[:, 1] = 0.0
            s = rng.choice([0.25, 0.5, 0.75], k)[:, None]  # below the emitter
            o = p - dirn * s
            sh = rng.random(k) < 0.3  # shadow segments that end just before / after the shared point
            mx = np.where(sh, s[:, 0] + rng.choice([-1e-5, 1e-5], k), FLT_MAX)
            add(o, dirn, 1e-8, mx, tag)
        elif tag == K_SHARED_OBLIQUE:
            tgt = shared_points(k)
            o = np.where((rng.random(k) < 0.3)[:, None], eye, origins_for(tgt, np.full(k, 0.05 * diag)))
            add(o, tgt - o, 1e-8, FLT_MAX, tag)
        elif tag == K_SURFACE:  # leaving a surface at |cos| from 1 down to 1e-4 to its plane
            idx = pick(k)
            o, sn = surface_points(rng, tri, cnrm, idx)
            t1 = _normalize(e1[idx]).astype(np.float64)
            t2 = np.cross(ng[idx], t1)
            phi = rng.random(k) * 2 * np.pi
            c = rng.choice(SURFACE_COS, k) * rng.choice([-1, 1], k)
            tang = t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None]
            dirn = tang * np.sqrt(1 - c * c)[:, None] + ng[idx] * c[:, None]
            aimed = rng.random(k) < 0.3  # a share toward other geometry, whatever the angle
            dirn = np.where(aimed[:, None], targets(k, 1.0) - o, dirn)
            sh = rng.random(k) < 0.3
            mx = np.where(sh, np.exp(rng.uniform(np.log(2e-3), np.log(max(diag, 1.0)), k)), FLT_MAX)
            add(o, dirn, 1e-8, mx, tag, idx, sn)
        elif tag == K_SLIVER_GRAZE:  # leaving the thinnest slivers at |cos| >= kGrazeCos, mostly from near the sharp end
            v = tri.reshape(ntri, 3, 3).astype(np.float64)
            corner = np.full(ntri, np.inf)
            for c in range(3):
                p, q = v[:, (c + 1) % 3] - v[:, c], v[:, (c + 2) % 3] - v[:, c]
                corner = np.minimum(corner, np.linalg.norm(np.cross(p, q), axis=1) /
                                    (np.linalg.norm(p, axis=1) * np.linalg.norm(q, axis=1)))
            idx = np.argsort(corner)[:30][rng.integers(0, 30, k)]
            o, sn = surface_points(rng, tri, cnrm, idx)
            t1 = _normalize(e1[idx]).astype(np.float64)
            t2 = np.cross(ng[idx], t1)
            phi = np.where(rng.random(k) < 0.7, rng.choice([0.0, np.pi], k) + rng.normal(size=k) * 0.05,
                           rng.random(k) * 2 * np.pi)  # mostly along the long side
            c = rng.choice(SLIVER_COS, k) * rng.choice([-1, 1], k)
            tang = t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None]
            add(o, tang * np.sqrt(1 - c * c)[:, None] + ng[idx] * c[:, None], 1e-8, FLT_MAX, tag, idx, sn)
        elif tag == K_NEAR:  # the hit 0.4e-3 .. 1.2e-3 away: between the near cull (5e-4) and t > 1e-3
            idx = pick(k)
            p, _ = surface_points(rng, tri, cnrm, idx, edges=False)
            dirn = _unit(rng, k).astype(np.float64)
            s = rng.uniform(0.4e-3, 1.2e-3, k)
            edge = rng.random(k) < 0.3  # on the threshold itself and its float neighbours
            s[edge] = rng.choice([1e-3, 1e-3 * (1 - 2e-7), 1e-3 * (1 + 2e-7), 5e-4, 0.999e-3, 1.001e-3], int(edge.sum()))
            add(p - dirn * s[:, None], dirn, 1e-8, FLT_MAX, tag)
        elif tag == K_MID:  # origins 1 - 90 scene diagonals away, aimed at vertices, edges and surface points: still the
            # culled, slack-free walk (within 100 diagonals), where the plane distances' rounding grows with the
            # distance and only the boxes' padding (kTriBoxPad x diagonal) keeps a hit at a box face inside its boxes
            dirn = _unit(rng, k).astype(np.float64)
            dist = diag * np.exp(rng.uniform(np.log(1.0), np.log(90.0), k))
            o = ((lo + hi) / 2 + dirn * dist[:, None]).astype(f32)
            tgt = np.where((rng.random(k) < 0.5)[:, None], shared_points(k), targets(k, 1.0))
            add(o, tgt - o, 1e-8, FLT_MAX, tag)
        elif tag == K_FAR:  # origins 100 - 10000 scene diagonals away (the slack test, the reference's own tree)
            dirn = _unit(rng, k).astype(np.float64)
            far = diag * np.exp(rng.uniform(np.log(100.0), np.log(10000.0), k))
            o = ((lo + hi) / 2 + dirn * far[:, None]).astype(f32)
            mx = np.where(rng.random(k) < 0.5, FLT_MAX, far * 1.5)
            add(o, targets(k, 0.8) - o, np.where(rng.random(k) < 0.5, 1.0, 1e-8), mx, tag)
    rays = np.concatenate(out)[:, :8]
    return (rays, np.concatenate(kind), np.concatenate(onrm), np.concatenate(otri), np.concatenate(osn))
