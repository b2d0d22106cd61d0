"""Per-function known-answer fixtures from the UNMODIFIED reference.

Run in the development container (needs oracle/_ref/ref_bdpt, built from
/root/reference by oracle/ref/Makefile):
    python tests/golden/make_kat_goldens.py

Each fixture holds seeded inputs and the reference's own outputs for one piece
of the BDPT path (ref_bdpt kat / sample_state, oracle/ref/ref_driver.cpp):
  kat_bsdf_<scene>.npz      BSDF::eval / pdf / sample (core.h:308-310) of every material
  kat_bsdf_edges.npz        the same on scenes/kat/bsdf_edges.obj (one material per BSDF kind and edge:
                            Ns 0 .. the largest float, Ks = 0, specw 0 and 1) over direction classes
                            around wi = reflect(wo), tiny and flushed Phong powers, zero and denormal
                            cosines, with the pdf of the swapped pair
  kat_fresnel.npz           GlassBSDF::FresnelDielectric (glass.h:40-53)
  kat_triangle.npz          rayTriangleIntersect (core.h:379-400)
  kat_intersect_<scene>.npz AcceleratorBVH::intersect + the any-hit query (accel.h:125-172, bvh.h:259-352)
  kat_splat.npz             BDPTIntegrator::splatToImagePlane (bdpt.h:485-496)
  kat_adversarial_<scene>.npz  AcceleratorBVH::intersect + the any-hit query on rays where the
                            product traversal's exactness argument is thinnest (grazing, ties,
                            surface origins, origins beyond 100 scene diagonals)
  kat_geom_<scene>.npz      the same two queries on the generated scenes of scenes/variants.py GEOM_SCENES
                            (`python make_kat_goldens.py generated`): one-leaf and first-split trees, a
                            zero-thick grid, exact duplicates, detail below the box padding, slivers, a
                            52-level chain; ray kinds of tests/geom_rays.py
  kat_sampler_<integ>.npz   Integrator::render(ray, sampler) from arbitrary std::mt19937 states
                            (integrator.h:31; bdpt.h:219, path.h:235, direct.h:449)
The sampling side (`python make_kat_goldens.py sampling`; draws enter as std::mt19937 output words):
  kat_sampling_canonical.npz  Sampler::next() (math.h:70) of one word: 0xFFFFFF00 .. 0xFFFFFFFF, 0, 1, around
                            every power of two, conversion ties, random
  kat_sampling_warp.npz     Warp::squareToUniformHemisphere / Triangle / Sphere and pdfs (math.h:119-151, :229-234)
  kat_sampling_emitter.npz  selectEmitter + sampleEmitterPosition (integrator.cpp:46-51, :73-100) on
                            scenes/kat/emit_edges.obj: draws on every CDF knot and its float neighbours, u0 around
                            every k / 5, triangle draws at 0 and the float below 1, random
  kat_sampling_camera.npz   the driver's cameraRay (renderer.cpp:165-195) at 64x64 and 80x48, spp 1 and 4
  kat_sampling_sphere.npz   sampleSphereByArea / BySolidAngle and raySphereIntersect (direct.h:37-69, :96-141)
  kat_sampler_edges_bdpt_<scene>.npz  BDPTIntegrator::render(ray, sampler) from states whose first 12 outputs are
                            0, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF and words on CDF knots (sample_state mode)
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "scenes"))
import variants  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "ref_bdpt")
TMP = tempfile.mkdtemp()
f32 = np.float32


def run(args):
    subprocess.run([REF, *args], check=True, capture_output=True, text=True)


def toml(scene, W=64, H=64, spp=1, rr=None, kind="bdpt", **kw):
    path = os.path.join(TMP, f"{scene}_{kind}_{W}x{H}.toml")
    with open(path, "w") as f:
        if kind == "bdpt":
            f.write(variants.toml_text(scene, W, H, spp, rr))
        elif kind == "path":
            f.write(variants.path_toml_text(scene, W, H, spp, **kw))
        else:
            f.write(variants.direct_toml_text(scene, W, H, spp, **kw))
    return path


def kat(scene_toml, W, H, kind, records: np.ndarray, width: int) -> np.ndarray:
    fin, fout = os.path.join(TMP, kind + ".in"), os.path.join(TMP, kind + ".out")
    records.astype(f32).tofile(fin)
    run(["kat", scene_toml, str(W), str(H), kind, fin, fout])
    return np.fromfile(fout, f32).reshape(-1, width)


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def directions(rng, n):
    """Local-frame directions: mostly upper hemisphere, some lower, some grazing."""
    d = unit(rng, n)
    up = rng.random(n) < 0.7
    d[up, 2] = np.abs(d[up, 2])
    g = rng.random(n) < 0.1  # grazing
    d[g, 2] = (rng.random(g.sum()) * 1e-3 * np.sign(rng.random(g.sum()) - 0.3)).astype(f32)
    d[g] /= np.linalg.norm(d[g], axis=1, keepdims=True)
    return d.astype(f32)


def bsdf_fixture(scene, n_per=800, seed=1):
    rng = np.random.default_rng(seed)
    t = toml(scene)
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    import bdpt_amd  # host-only scene ingest: the material count

    nmat = bdpt_amd.Scene(variants.obj_path(scene)).info()["materials"]
    mats, recs = [], []
    for m in range(nmat):
        wo, wi = directions(rng, n_per), directions(rng, n_per)
        u = rng.random((n_per, 2)).astype(f32)
        u[:8] = np.array([[0, 0], [0.5, 0.5], [0.999999, 0.999999], [1e-7, 0.3], [0.3, 1e-7], [0.25, 0.75],
                          [0.9, 0.1], [0.1, 0.9]], f32)
        recs.append(np.concatenate([np.full((n_per, 1), m, np.int32).view(f32), wo, wi, u], axis=1))
        mats.append(m)
    rec = np.concatenate(recs)
    out = kat(t, 64, 64, "bsdf", rec, 14)
    np.savez_compressed(os.path.join(HERE, f"kat_bsdf_{scene}.npz"), mat=rec[:, 0].view(np.int32), wo=rec[:, 1:4],
                        wi=rec[:, 4:7], u=rec[:, 7:9], eval=out[:, 0:3], pdf=out[:, 3], sample_f=out[:, 4:7],
                        sample_wi=out[:, 7:10], sample_pdf=out[:, 10], type=out[:, 11].view(np.int32),
                        null=out[:, 13])
    print("bsdf", scene, rec.shape[0], "records,", len(mats), "materials")


EDGES_OBJ = os.path.join(REPO, "scenes", "kat", "bsdf_edges.obj")
# direction classes of kat_bsdf_edges (the fixture's cls column)
CLS_REFLECT, CLS_NUDGED, CLS_MID_POWER, CLS_TINY_POWER, CLS_ZERO_Z, CLS_GRAZING, CLS_LOWER, CLS_RANDOM = range(8)
CLS_NAMES = ["reflect", "nudged", "mid_power", "tiny_power", "zero_z", "grazing", "lower", "random"]
MIN_LOG2_BELOW_1 = -float(np.log2(np.float64(np.nextafter(f32(1), f32(0)))))  # |log2| of the float below 1: 8.6e-8


def lobe_z(wo, wi):
    """The Phong lobe's cosine as eval / pdf compute it, dot(wi, reflect(wo)) in float32
    (glm: (x x' + y y') + z z'; mixture.h:68, phong.h:68, Frame::toLocal's z)."""
    wo, wi = wo.astype(f32), wi.astype(f32)
    return ((wi[:, 0] * -wo[:, 0] + wi[:, 1] * -wo[:, 1]).astype(f32) + wi[:, 2] * wo[:, 2]).astype(f32)


def power_classes(z, ex):
    """Per record: z > 1, z == 1, the power unflushed with ex |log2 z| in [60, 126], the power
    below 2^-126 (float64 classification of the float32 z)."""
    z64 = z.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(z64 > 0, float(ex) * np.abs(np.log2(np.where(z64 > 0, z64, 1.0))), np.inf)
    below1 = (z64 >= 0) & (z64 < 1)
    return z > 1, z == 1, below1 & (t >= 60) & (t <= 126), below1 & (t > 126) & (ex > 0)


def upper_unit(rng, n):
    d = unit(rng, n)
    d[:, 2] = np.maximum(np.abs(d[:, 2]), f32(0.05))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def with_lobe_cosine(rng, n, z):
    """(wo, wi) pairs whose lobe cosine is the float32 z exactly: wo = +z axis, wi = (x, y, z)
    (the products with wo's zeros are exact), and for z >= 1e-3 half of them about a random wo
    (there z is met up to the dot product's rounding)."""
    z = np.asarray(z, np.float64)
    phi = rng.random(n) * 2 * np.pi
    s = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(z, 1.0) ** 2))
    wo = np.tile(np.array([0, 0, 1], f32), (n, 1))
    wi = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1).astype(f32)
    g = (rng.random(n) < 0.5) & (z >= 1e-3)
    if g.any():
        o = upper_unit(rng, int(g.sum())).astype(np.float64)
        r = o * np.array([-1.0, -1.0, 1.0])
        a = np.cross(r, rng.normal(size=r.shape))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        wo[g] = o.astype(f32)
        wi[g] = (r * z[g, None] + a * s[g, None]).astype(f32)
    return wo, wi


def edge_directions(rng, n, ex):
    """(wo, wi, cls) for one material of exponent ex: the classes of the module docstring of
    tests/test_gpu_kat_connection.py, each drawn from a larger pool by quota."""
    pool = 40 * n
    # reflect / nudged: wi = reflect_z(wo), exactly or moved by +-1..8 ulp per component; the float32
    # lobe cosine dot(wo, wo) then lands just below, on or just above 1
    o = upper_unit(rng, pool)
    wi = o * np.array([-1, -1, 1], f32)
    k = rng.integers(-8, 9, size=(pool, 3))
    k[: pool // 4] = 0
    nudged = (np.ascontiguousarray(wi, f32).view(np.int32) + k.astype(np.int32)).view(f32)  # +-k ulp (no component is 0 or changes binade sign here)
    z = lobe_z(o, nudged)
    exact = (k == 0).all(1)
    take = []
    for sel, cnt in (((z > 1) & exact, n // 20), ((z == 1) & exact, n // 20), ((z < 1) & exact, n // 20),
                     ((z > 1) & ~exact, n // 12), ((z == 1) & ~exact, n // 12), ((z < 1) & ~exact, n // 12)):
        idx = np.flatnonzero(sel)[:cnt]
        assert idx.size == cnt, "the reflect / nudged pool is too small"
        take.append(idx)
    take = np.concatenate(take)
    wo_l, wi_l = [o[take]], [nudged[take]]
    cls_l = [np.where(exact[take], CLS_REFLECT, CLS_NUDGED)]
    # mid_power: ex |log2 z| in [60, 125] (an unflushed, small power); tiny_power: beyond 128 (below 2^-126)
    exx = float(ex)
    nm, nt = n // 7, n // 10
    if 0 < exx * MIN_LOG2_BELOW_1 <= 125:
        t = rng.uniform(max(60.0, exx * MIN_LOG2_BELOW_1), 125.0, nm)
        a, b = with_lobe_cosine(rng, nm, np.exp2(-t / exx))
        wo_l.append(a), wi_l.append(b), cls_l.append(np.full(nm, CLS_MID_POWER))
    if exx > 0:
        t = rng.uniform(max(128.0, exx * MIN_LOG2_BELOW_1), max(400.0, 3 * exx * MIN_LOG2_BELOW_1), nt)
        zt = np.exp2(-t / exx)
        zt[:4] = [0.0, 1e-40, 1e-30, 1e-45][: min(4, nt)]
        a, b = with_lobe_cosine(rng, nt, zt)
        wo_l.append(a), wi_l.append(b), cls_l.append(np.full(nt, CLS_TINY_POWER))
    # zero_z: wi.z or wo.z is +0, -0, +-1e-30 or a denormal
    nz = n // 10
    a, b = directions(rng, nz), directions(rng, nz)
    v = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40], f32), nz)
    which = rng.integers(0, 3, nz)
    a[which != 1, 2] = v[which != 1]
    b[which != 0, 2] = v[which != 0]
    wo_l.append(a), wi_l.append(b), cls_l.append(np.full(nz, CLS_ZERO_Z))
    # grazing: both within 1e-3 of the horizon, either side
    ng = n // 12
    a, b = unit(rng, ng), unit(rng, ng)
    a[:, 2] = (rng.random(ng) * 1e-3 * np.sign(rng.random(ng) - 0.3)).astype(f32)
    b[:, 2] = (rng.random(ng) * 1e-3 * np.sign(rng.random(ng) - 0.3)).astype(f32)
    wo_l.append(a), wi_l.append(b), cls_l.append(np.full(ng, CLS_GRAZING))
    # lower: wo, wi or both below the surface
    nl = n // 12
    a, b = upper_unit(rng, nl), upper_unit(rng, nl)
    side = rng.integers(0, 3, nl)
    a[side != 1, 2] *= -1
    b[side != 0, 2] *= -1
    wo_l.append(a), wi_l.append(b), cls_l.append(np.full(nl, CLS_LOWER))
    # random: the mix of the kat_bsdf_<scene> fixtures
    nr = n - sum(x.shape[0] for x in wo_l)
    wo_l.append(directions(rng, nr)), wi_l.append(directions(rng, nr)), cls_l.append(np.full(nr, CLS_RANDOM))
    return np.concatenate(wo_l).astype(f32), np.concatenate(wi_l).astype(f32), np.concatenate(cls_l).astype(np.int8)


def bsdf_edges_fixture(n_per=2000, n_sample=200, seed=60):
    """kat_bsdf_edges.npz: BSDF::eval / pdf of every material of scenes/kat/bsdf_edges.obj on
    the direction classes above, pdf also of the swapped pair (pdf_rev: what a connection's
    reverse pdf must equal), and BSDF::sample for the first n_sample records of each material."""
    rng = np.random.default_rng(seed)
    t = os.path.join(TMP, "bsdf_edges.toml")
    cam = variants.CBOX_CAMERA
    v3 = lambda v: "[ " + ", ".join(repr(float(x)) for x in v) + " ]"
    with open(t, "w") as f:
        f.write(f'[input]\nobjfile = "{EDGES_OBJ}"\n\n[camera]\neye = {v3(cam["eye"])}\nat = {v3(cam["at"])}\n'
                f'up = {v3(cam["up"])}\nfov = {float(cam["fov"])!r}\n\n[film]\nwidth = 64\nheight = 64\n\n'
                f'[renderer]\nrealtime = false\ntype = "bdpt"\nrrDepth = 5\nrrProb = 0.95\nspp = 1\n')
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    import bdpt_amd  # host-only scene ingest: material count, kinds and exponents

    sc = bdpt_amd.Scene(EDGES_OBJ)
    names, ns = edges_materials()
    assert sc.info()["materials"] == len(names)
    recs, clss, power = [], [], {}
    for m, name in enumerate(names):
        kind = sc.bsdf_type(m)[1]
        wo, wi, cls = edge_directions(rng, n_per, ns[m])
        u = rng.random((n_per, 2)).astype(f32)
        u[:8] = np.array([[0, 0], [0.5, 0.5], [0.999999, 0.999999], [1e-7, 0.3], [0.3, 1e-7], [0.25, 0.75],
                          [0.9, 0.1], [0.1, 0.9]], f32)
        recs.append(np.concatenate([np.full((n_per, 1), m, np.int32).view(f32), wo, wi, u], axis=1))
        clss.append(cls)
        # every class this material can hold is populated
        counts = np.bincount(cls, minlength=len(CLS_NAMES))
        exx = float(ns[m])
        reach_mid, reach_tiny = 0 < exx * MIN_LOG2_BELOW_1 <= 125, exx > 0
        for c, cname in enumerate(CLS_NAMES):
            if (c == CLS_MID_POWER and not reach_mid) or (c == CLS_TINY_POWER and not reach_tiny):
                continue
            assert counts[c] >= 100, (name, cname, counts[c])
        # the power classes of the materials that evaluate a Phong power (kind 5 Phong, 4 Mixture with
        # Ks != 0). Two of the four cannot exist for every exponent in float32: x^0 is 1 for every x
        # (Ns 0 has neither a mid nor a tiny power), and for the largest finite Ns the float below 1
        # already gives ex |log2 z| = 2.9e31 (no unflushed power but 1). They are required wherever a
        # float32 z can reach them.
        if kind == 5 or (kind == 4 and name not in ("mixKs0", "mixKs0Scaled")):
            gt1, eq1, mid, tiny = (int(x.sum()) for x in power_classes(lobe_z(wo, wi), ns[m]))
            power[name] = dict(Ns=float(ns[m]), z_gt_1=gt1, z_eq_1=eq1, mid_power=mid, tiny_power=tiny)
            assert gt1 >= 100 and eq1 >= 100, (name, gt1, eq1)
            assert mid >= 200 or not reach_mid, (name, mid)
            assert tiny >= 100 or not reach_tiny, (name, tiny)
    rec = np.concatenate(recs)
    swapped = rec.copy()
    swapped[:, 1:4], swapped[:, 4:7] = rec[:, 4:7], rec[:, 1:4]
    out = kat(t, 64, 64, "bsdf", rec, 14)
    rev = kat(t, 64, 64, "bsdf", swapped, 14)
    mat = rec[:, 0].view(np.int32)
    first = (np.arange(rec.shape[0]) % n_per) < n_sample  # the records that keep their sample outputs
    np.savez_compressed(os.path.join(HERE, "kat_bsdf_edges.npz"), mat=mat, wo=rec[:, 1:4], wi=rec[:, 4:7],
                        cls=np.concatenate(clss), eval=out[:, 0:3], pdf=out[:, 3], pdf_rev=rev[:, 3],
                        sample_idx=np.flatnonzero(first).astype(np.int32), u=rec[first, 7:9],
                        sample_f=out[first, 4:7], sample_wi=out[first, 7:10], sample_pdf=out[first, 10],
                        type=out[:, 11].view(np.int32)[::n_per].copy(), null=out[:, 13][::n_per].astype(np.int8),
                        names=np.array(names), ns=np.array(ns, f32))
    print("bsdf edges", rec.shape[0], "records,", len(names), "materials; largest Ns", float(max(ns)))
    for name, p in power.items():
        print("  ", name, p)


def edges_materials():
    """(names, Ns as float32) of scenes/kat/bsdf_edges.mtl in file order (= material index)."""
    names, ns = [], []
    with open(os.path.splitext(EDGES_OBJ)[0] + ".mtl") as f:
        for line in f:
            tok = line.split()
            if tok[:1] == ["newmtl"]:
                names.append(tok[1])
            elif tok[:1] == ["Ns"]:
                ns.append(f32(float(tok[1])))
    return names, ns


def fresnel_fixture(n=6000, seed=2):
    rng = np.random.default_rng(seed)
    eta = np.where(rng.random(n)[:, None] < 0.5, [[1.0, 1.5]], [[1.5, 1.0]]).astype(f32)
    cos_i = rng.random(n).astype(f32)
    cos_i[:6] = [0, 1, 1e-6, 0.5, 0.7453560, 0.7453559]  # around the critical angle from inside
    e = eta[:, 0] / eta[:, 1]
    sin2_t = e * e * np.maximum(0, 1 - cos_i * cos_i)
    cos_t = np.sqrt(np.maximum(0, 1 - sin2_t)).astype(f32)
    cos_t = np.where(rng.random(n) < 0.1, rng.random(n), cos_t).astype(f32)
    rec = np.concatenate([eta, cos_i[:, None], cos_t[:, None]], axis=1).astype(f32)
    out = kat(toml("caustic"), 64, 64, "fresnel", rec, 1)[:, 0]
    np.savez_compressed(os.path.join(HERE, "kat_fresnel.npz"), inp=rec, out=out)
    print("fresnel", n)


def triangle_fixture(n=10000, seed=3):
    rng = np.random.default_rng(seed)
    v = (rng.normal(size=(n, 9)) * rng.choice([0.01, 1.0, 100.0], size=(n, 1))).astype(f32)
    o = (rng.normal(size=(n, 3)) * 3).astype(f32)
    b = rng.random((n, 3))
    b[: n // 4] = np.stack([rng.random(n // 4) * 1.2 - 0.1, rng.random(n // 4) * 1.2 - 0.1,
                            np.zeros(n // 4)], 1)  # near and across the edges
    b[:, 2] = 1 - b[:, 0] - b[:, 1]
    target = b[:, 2:3] * v[:, 0:3] + b[:, 0:1] * v[:, 3:6] + b[:, 1:2] * v[:, 6:9]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    par = rng.random(n) < 0.05  # rays parallel to the triangle plane (|det| < 1e-8)
    e1, e2 = v[par, 3:6] - v[par, 0:3], v[par, 6:9] - v[par, 0:3]
    d[par] = e1 / np.linalg.norm(e1, axis=1, keepdims=True) + 0 * e2
    rays = np.concatenate([o, d.astype(f32), np.full((n, 1), 1e-8, f32), np.full((n, 1), 3.4e38, f32)], 1)
    rec = np.concatenate([rays, v], 1).astype(f32)
    out = kat(toml("caustic"), 64, 64, "tri", rec, 4)
    np.savez_compressed(os.path.join(HERE, "kat_triangle.npz"), rays=rec[:, :8], verts=rec[:, 8:], out=out)
    print("triangle", n, "hits", int(out[:, 0].sum()))


def scene_rays(rng, scene, n):
    """Camera rays, rays from inside the box in every direction (incl. axis-parallel),
    and shadow-ray segments between points inside the box."""
    eye = np.array(variants.SCENES[scene]["camera"]["eye"], f32)
    k = n // 4
    lo, hi = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 1.6, 1.0])
    # 1: camera rays toward the box (min_t 1, max_t 1000: renderer.cpp:192)
    tgt = lo + rng.random((k, 3)) * (hi - lo)
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r1 = np.concatenate([np.repeat(eye[None], k, 0), d, np.ones((k, 1)), np.full((k, 1), 1000.0)], 1)
    # 2: from inside the box, random directions (Epsilon / FLT_MAX, ContinuePathRandomWalk)
    o = lo + rng.random((k, 3)) * (hi - lo)
    d = unit(rng, k)
    r2 = np.concatenate([o, d, np.full((k, 1), 1e-8), np.full((k, 1), 3.402823466e38)], 1)
    # 3: axis-parallel directions (zero reciprocal components: the exact binary-tree path)
    o = lo + rng.random((k, 3)) * (hi - lo)
    d = np.zeros((k, 3))
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
    half = k // 2
    d[:half, (np.arange(half) + 1) % 3] = rng.normal(size=half)  # one zero component only
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r3 = np.concatenate([o, d, np.full((k, 1), 1e-8), np.full((k, 1), 3.402823466e38)], 1)
    # 4: shadow segments (visibilityQuery: [Epsilon, dist - 1e-5], bdpt.h:498-505)
    m = n - 3 * k
    a = lo + rng.random((m, 3)) * (hi - lo)
    b = lo + rng.random((m, 3)) * (hi - lo)
    d = b - a
    dist = np.linalg.norm(d, axis=1, keepdims=True)
    r4 = np.concatenate([a, d / dist, np.full((m, 1), 1e-8), dist - 1e-5], 1)
    return np.concatenate([r1, r2, r3, r4]).astype(f32)


def intersect_fixture(scene, n, seed):
    rng = np.random.default_rng(seed)
    rays = scene_rays(rng, scene, n)
    out = kat(toml(scene), 64, 64, "intersect", rays, 21)
    np.savez_compressed(os.path.join(HERE, f"kat_intersect_{scene}.npz"), rays=rays, out=out)
    print("intersect", scene, n, "hits", int(out[:, 0].sum()), "occluded", int(out[:, 20].sum()))


def _normalize(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _surface_points(rng, tri, idx, nrm=None):
    """Points on triangles idx as the path computes hit points (shade_hit /
    SurfaceInteraction: (v0 w + v1 u) + v2 v in float32), with a share exactly on
    edges and vertices. With nrm (the corner normals, [ntri, 9]) also the
    interpolated shading normals there (normalize((n0 w + n1 u) + n2 v), float32)."""
    n = idx.size
    u = rng.random(n).astype(f32)
    v = (rng.random(n) * (1 - u)).astype(f32)
    k = rng.random(n)
    u[k < 0.1] = 0
    v[(k >= 0.1) & (k < 0.2)] = 0
    e = (k >= 0.2) & (k < 0.3)
    v[e] = (f32(1) - u[e]).astype(f32)
    c = (k >= 0.3) & (k < 0.35)
    u[c], v[c] = 0, 0
    w = (f32(1) - u - v).astype(f32)
    v0, v1, v2 = tri[idx, 0:3], tri[idx, 3:6], tri[idx, 6:9]
    p = ((v0 * w[:, None] + v1 * u[:, None]) + v2 * v[:, None]).astype(f32)
    if nrm is None:
        return p
    n0, n1, n2 = nrm[idx, 0:3], nrm[idx, 3:6], nrm[idx, 6:9]
    sn = ((n0 * w[:, None] + n1 * u[:, None]) + n2 * v[:, None]).astype(f32)
    sn = (sn / np.sqrt(np.sum(sn.astype(f32) * sn, 1, keepdims=True, dtype=f32))).astype(f32)
    return p, sn


def adversarial_rays(scene, n, seed):
    """Rays chosen where the product traversal's exactness argument is thinnest
    (DESIGN.md §2 items 5-6): the computed hit of Moller-Trumbore near |det| = 1e-8,
    ties between triangles sharing an edge or a vertex, origins on surfaces, and
    origins beyond 100 scene diagonals, and (kinds 6, 7) grazing rays leaving the
    curved mesh, whose interpolated shading normal is not the triangle's plane
    normal. Returns (rays [n', 8] float32, kind [n'], the geometric normal of the
    triangle a ray leaves [n', 3] (0 for camera / free / far origins), that
    triangle [n'] (-1: none) and the shading normal the path holds there [n', 3])."""
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    import bdpt_amd

    rng = np.random.default_rng(seed)
    tf, ti, nf, _ = bdpt_amd.Scene(variants.obj_path(scene)).export()
    tri = tf[:, :9].astype(f32)
    cnrm = tf[:, 9:18].astype(f32)
    e1, e2 = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3]
    cr = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    area = 0.5 * np.linalg.norm(cr, axis=1)
    ok = area > 0
    ng = np.zeros_like(cr)
    ng[ok] = cr[ok] / np.linalg.norm(cr[ok], axis=1, keepdims=True)
    lo, hi = nf[0, :3].astype(np.float64), nf[0, 3:].astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    centre = (lo + hi) / 2
    big = np.argsort(-area)[:64]  # walls, floor, ceiling, box faces, light
    shapes, counts = np.unique(ti[:, 0], return_counts=True)
    curved = np.flatnonzero(ti[:, 0] == shapes[np.argmax(counts)])  # the tessellated sphere(s)
    FLT_MAX = 3.402823466e38
    k = n // 6
    out, kind, onrm, otri, osn = [], [], [], [], []

    def add(o, d, mn, mx, tag, nrm=None, tri_idx=None, sn=None):
        ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)  # degenerate triangles of a generated mesh
        if not ok.all():
            o, d = o[ok], d[ok]
            mn, mx = (mn if np.isscalar(mn) else mn[ok]), (mx if np.isscalar(mx) else mx[ok])
            nrm, tri_idx, sn = (None if x is None else np.asarray(x)[ok] for x in (nrm, tri_idx, sn))
        m = o.shape[0]
        onrm.append(np.zeros((m, 3), f32) if nrm is None else np.asarray(nrm, f32))
        otri.append(np.full(m, -1, np.int32) if tri_idx is None else np.asarray(tri_idx, np.int32))
        osn.append(np.zeros((m, 3), f32) if sn is None else np.asarray(sn, f32))
        out.append(np.concatenate([o, _normalize(d), np.broadcast_to(np.float32(mn), (m, 1)) if np.isscalar(mn)
                                   else mn[:, None], np.broadcast_to(np.float32(mx), (m, 1)) if np.isscalar(mx)
                                   else mx[:, None]], 1).astype(f32))
        kind.append(np.full(m, tag, np.int32))

    # 0: grazing continuation rays from points on the large triangles, |sin| from 0 to 1e-2
    idx = rng.choice(big, k)
    o, sn = _surface_points(rng, tri, idx, cnrm)
    t1 = _normalize(e1[idx])
    t2 = _normalize(np.cross(ng[idx], t1))
    phi = rng.random(k) * 2 * np.pi
    delta = rng.choice([0.0, 1e-9, 3e-9, 1e-8, 3e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.015, 0.02, 0.03, 0.05],
                       k) * rng.choice([-1, 1], k)
    d = t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None] + ng[idx] * delta[:, None]
    h = rng.choice([0.0, 0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, 1e-4], k)
    add((o + ng[idx] * h[:, None]).astype(f32), d, 1e-8, FLT_MAX, 0, ng[idx], idx, sn)
    # 1: grazing shadow segments between two points of the same large triangle (visibilityQuery)
    idx = rng.choice(big, k)
    (a, sn), b = _surface_points(rng, tri, idx, cnrm), _surface_points(rng, tri, idx)
    lift = rng.choice([0.0, 1e-7, 1e-5, 1e-3], k)[:, None] * ng[idx]
    a, b = (a + lift).astype(f32), (b + lift).astype(f32)
    dd = (b - a).astype(f32)
    dist = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).astype(f32)
    keep = dist > 1e-4
    add(a[keep], dd[keep], 1e-8, (dist[keep] - f32(1e-5)).astype(f32), 1, ng[idx][keep], idx[keep], sn[keep])
    # 2: rays through the curved mesh's vertices and edges (ties between neighbours, silhouettes)
    idx = rng.choice(curved, k)
    w = rng.choice(4, k)
    tgt = np.where((w == 0)[:, None], tri[idx, 0:3], np.where((w == 1)[:, None], (tri[idx, 0:3] + tri[idx, 3:6]) / 2,
                   _surface_points(rng, tri, idx)))
    eye = np.array(variants.SCENES[scene]["camera"]["eye"], np.float64)
    inner = lo + rng.random((k, 3)) * (hi - lo)
    o = np.where((rng.random(k) < 0.5)[:, None], eye, inner).astype(f32)
    add(o, tgt - o, 1e-8, FLT_MAX, 2)
    # 3: continuation rays from surface points of any triangle, both hemispheres, near-tangent included
    idx = rng.integers(0, tri.shape[0], k)
    o, sn = _surface_points(rng, tri, idx, cnrm)
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    flat = rng.random(k) < 0.3
    d[flat] -= ng[idx][flat] * np.sum(d[flat] * ng[idx][flat], 1, keepdims=True) * (1 - rng.choice(
        [1e-6, 1e-4, 1e-2], flat.sum()))[:, None]
    add(o, d, 1e-8, FLT_MAX, 3, ng[idx], idx, sn)
    # 4: origins 100 - 10000 scene diagonals away, aimed at surface points (the slack-test regime)
    dirn = rng.normal(size=(k, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    far = diag * np.exp(rng.uniform(np.log(100.0), np.log(10000.0), k))
    o = (centre + dirn * far[:, None]).astype(f32)
    tgt = _surface_points(rng, tri, rng.integers(0, tri.shape[0], k))
    mx = np.where(rng.random(k) < 0.5, FLT_MAX, far * 1.5).astype(f32)
    add(o, tgt - o, np.where(rng.random(k) < 0.5, 1.0, 1e-8).astype(f32), mx, 4)
    # 5: shadow segments between surface points of any two triangles
    m = n - 5 * k
    ia = rng.integers(0, tri.shape[0], m)
    a, sn = _surface_points(rng, tri, ia, cnrm)
    b = _surface_points(rng, tri, rng.integers(0, tri.shape[0], m))
    dd = (b - a).astype(f32)
    dist = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).astype(f32)
    keep = dist > 1e-4
    add(a[keep], dd[keep], 1e-8, (dist[keep] - f32(1e-5)).astype(f32), 5, ng[ia][keep], ia[keep], sn[keep])
    # 6: grazing continuation rays leaving the curved mesh: |cos| to the
    # triangle's plane from 0 to 0.1, while the interpolated shading normal the path
    # tests against (cull_near_for) is tilted from that plane's normal
    idx = rng.choice(curved, k)
    o, sn = _surface_points(rng, tri, idx, cnrm)
    t1 = _normalize(e1[idx])
    t2 = _normalize(np.cross(ng[idx], t1))
    phi = rng.random(k) * 2 * np.pi
    delta = rng.choice([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 3e-3, 1e-2, 0.015, 0.019, 0.021, 0.03, 0.05, 0.1],
                       k) * rng.choice([-1, 1], k)
    d = t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None] + ng[idx] * delta[:, None]
    h = rng.choice([0.0, 0.0, 1e-7, -1e-7, 1e-6, -1e-6], k)
    add((o + ng[idx] * h[:, None]).astype(f32), d, 1e-8, FLT_MAX, 6, ng[idx], idx, sn)
    # 7: grazing shadow segments from the curved mesh along its triangles' planes
    idx = rng.choice(curved, k)
    a, sn = _surface_points(rng, tri, idx, cnrm)
    t1 = _normalize(e1[idx])
    t2 = _normalize(np.cross(ng[idx], t1))
    phi = rng.random(k) * 2 * np.pi
    delta = rng.choice([0.0, 1e-6, 1e-4, 1e-2, 0.019, 0.03, 0.1], k) * rng.choice([-1, 1], k)
    d = _normalize(t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None] + ng[idx] * delta[:, None])
    ln = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), k))
    b = (a + d * ln[:, None]).astype(f32)
    dd = (b - a).astype(f32)
    dist = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).astype(f32)
    keep = dist > 1e-4
    add(a[keep], dd[keep], 1e-8, (dist[keep] - f32(1e-5)).astype(f32), 7, ng[idx][keep], idx[keep], sn[keep])
    return (np.concatenate(out), np.concatenate(kind), np.concatenate(onrm), np.concatenate(otri),
            np.concatenate(osn))


def adversarial_fixture(scene, n, seed):
    rays, kind, onrm, otri, osn = adversarial_rays(scene, n, seed)
    out = kat(toml(scene), 64, 64, "intersect", rays, 21)
    np.savez_compressed(os.path.join(HERE, f"kat_adversarial_{scene}.npz"), rays=rays, kind=kind, onrm=onrm,
                        otri=otri, osn=osn,
                        hit=out[:, 0].astype(np.int8), t=out[:, 1], u=out[:, 2], v=out[:, 3],
                        shape=out[:, 4].view(np.int32), prim=out[:, 5].view(np.int32),
                        occluded=out[:, 20].astype(np.int8))
    print("adversarial", scene, rays.shape[0], "rays; hits", int(out[:, 0].sum()), "occluded",
          int(out[:, 20].sum()), "per kind", np.bincount(kind))


# Seeds at which the reference's own results meet tests/test_geom_walk_cpu.py's conditions (hits and misses in
# every ray kind that can have them; flat's rays leaving the grid can only hit the small emitter: seed 84 has none).
GEOM_SEEDS = dict(tiny1=80, tiny2=81, tiny4=82, tiny5=83, flat=85, dupes=85, scales=86, slivers=87, chain=88)


def generated_fixture(name, n=2048, seed=0):
    """kat_geom_<name>.npz: a generated scene of variants.GEOM_SCENES (geometry classes the shipped
    scenes lack), rays of tests/geom_rays.py's kinds with the surfaces they leave, the reference's
    21-word intersect output on them, and the SHA-256 of the OBJ text the reference read."""
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import bdpt_amd
    import geom_rays

    cam = variants.GEOM_SCENES[name][2]
    obj = variants.geom_obj(name, os.path.join(TMP, "geom"))
    tf, _, nf, _ = bdpt_amd.Scene(obj).export()  # host-only ingest: the triangles and the scene box to aim at
    rays, kind, onrm, otri, osn = geom_rays.geometry_rays(name, tf, nf, cam["eye"], n, seed)
    f3 = lambda v: "[ " + ", ".join(repr(float(x)) for x in v) + " ]"
    path = os.path.join(TMP, f"geom_{name}.toml")
    with open(path, "w") as f:
        f.write(f'[input]\nobjfile = "{obj}"\n\n[camera]\neye = {f3(cam["eye"])}\nat = {f3(cam["at"])}\n'
                f'up = {f3(cam["up"])}\nfov = {float(cam["fov"])!r}\n\n[film]\nwidth = 64\nheight = 64\n\n'
                f'[renderer]\nrealtime = false\ntype = "bdpt"\nrrDepth = 5\nrrProb = 0.95\nspp = 1\n')
    out = kat(path, 64, 64, "intersect", rays, 21)
    dst = os.path.join(HERE, f"kat_geom_{name}.npz")
    np.savez_compressed(dst, rays=rays, kind=kind, onrm=onrm, otri=otri, osn=osn, out=out,
                        obj_sha256=np.array(variants.file_sha256(obj)))
    print("generated", name, rays.shape[0], "rays; hits", int(out[:, 0].sum()), "occluded", int(out[:, 20].sum()),
          "per kind", np.bincount(kind), os.path.getsize(dst), "bytes")


def splat_fixture(seed=5):
    rng = np.random.default_rng(seed)
    res = {}
    for (W, H) in [(64, 64), (512, 512), (80, 48)]:
        n = 4000
        p = (np.array([-1.2, -0.2, -1.2]) + rng.random((n, 3)) * np.array([2.4, 2.0, 6.0])).astype(f32)
        out = kat(toml("caustic", W, H), W, H, "splat", p, 2).view(np.int32)
        res[f"p_{W}x{H}"] = p
        res[f"xy_{W}x{H}"] = out
    np.savez_compressed(os.path.join(HERE, "kat_splat.npz"), **res)
    print("splat")


def states(rng, n):
    """std::mt19937 states: seeded and advanced (across the first twist, the lazy
    window's end, a whole state) and arbitrary words with arbitrary positions."""
    out = []
    for i in range(n):
        if i < n * 3 // 4:
            rs = np.random.RandomState(int(rng.integers(0, 2**32)))  # init_genrand == std::mt19937(seed)
            skip = int(rng.choice([0, 1, 2, 100, 225, 226, 227, 400, 623, 624, 625, 1000, 5000]))
            if skip:
                rs.randint(0, 2**32, size=skip, dtype=np.uint32)
            _, key, pos = rs.get_state()[:3]
            out.append(np.concatenate([key.astype(np.uint32), [np.uint32(pos)]]))
        else:
            key = rng.integers(0, 2**32, size=624, dtype=np.uint64).astype(np.uint32)
            out.append(np.concatenate([key, [np.uint32(rng.integers(0, 625))]]))
    return np.array(out, np.uint32)


def sampler_fixture(name, scene, toml_path, W, H, spp, rr, n, seed):
    rng = np.random.default_rng(seed)
    eye = np.array(variants.SCENES[scene]["camera"]["eye"], f32)
    tgt = np.array([-1.0, 0.0, -1.0]) + rng.random((n, 3)) * np.array([2.0, 1.6, 2.0])
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.repeat(eye[None], n, 0), d, np.ones((n, 1)), np.full((n, 1), 1000.0)], 1).astype(f32)
    st = states(rng, n)
    rec = np.concatenate([rays, st.view(f32)], 1)
    fin, fout = os.path.join(TMP, name + ".in"), os.path.join(TMP, name + ".out")
    rec.astype(f32).tofile(fin)
    # rr only for the BDPT scenes: ref_driver's setup() writes it to Config's
    # pt.rrDepth, which shares a union with di.bsdfSamples (core.h:201-240)
    run(["sample_state", toml_path, str(W), str(H), str(spp), str(rr if "bdpt" in name else 0), fin, fout, "-"])
    out = np.fromfile(fout, f32).reshape(n, 3 + 625 + 1 + 64)
    np.savez_compressed(os.path.join(HERE, f"kat_sampler_{name}.npz"), rays=rays, state_in=st, Li=out[:, :3],
                        state_out=out[:, 3:628].view(np.uint32), nsplat=out[:, 628].view(np.int32),
                        splats=out[:, 629:].reshape(n, 16, 4), width=W, height=H, spp=spp, rr=rr)
    print("sampler", name, n, "records; splat counts", np.bincount(out[:, 628].view(np.int32)))


# ------------------------------------------------------------------ the sampling side
# A draw enters the reference as the std::mt19937 output word it is converted from: the driver
# loads a generator state whose next outputs are exactly the given words (ref_driver.cpp
# samplerOfWords), which needs the inverse of the output tempering.
ONE_BELOW = np.nextafter(f32(1), f32(0))  # the largest float below 1
SPECIAL_WORDS = [0, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF]  # 0; the last word below the clamp; the first and last in it
SAMPLING_FILES = ["kat_sampling_canonical", "kat_sampling_warp", "kat_sampling_emitter", "kat_sampling_camera",
                  "kat_sampling_sphere", "kat_sampler_edges_bdpt_caustic", "kat_sampler_edges_bdpt_emit_edges"]
CAMERA_CONFIGS = [(64, 64, 1), (64, 64, 4), (80, 48, 1), (80, 48, 4)]  # W, H, spp
EDGE_DRAWS = 128  # outputs crafted per kat_sampler_edges state (a sample of rrDepth <= 8 draws 66 at most)


def temper(y):
    y = np.asarray(y, np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def untemper(y):
    """The state word whose tempered output is y (std::mt19937)."""
    y = np.asarray(y, np.uint32).copy()
    y ^= y >> np.uint32(18)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    t = y.copy()
    for _ in range(4):
        t = y ^ ((t << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = t
    t = y.copy()
    for _ in range(2):
        t = y ^ (t >> np.uint32(11))
    return t


def word_of(u):
    """A word that generate_canonical turns into the float32 u exactly (0 <= u < 1; u = 0 or
    u >= 2^-8, where u * 2^32 is an integer of at most 24 significant bits)."""
    u = np.asarray(u, f32)
    assert ((u == 0) | ((u >= f32(2.0 ** -8)) & (u < 1))).all()
    return (u.astype(np.float64) * 2.0 ** 32).astype(np.uint64).astype(np.uint32)


def canonical_np(w):
    """generate_canonical<float, 24> of one word as libstdc++ 11 computes it: the float32
    conversion, the division by 2^32 (exact) and the move to the float below 1."""
    f = np.asarray(w, np.uint32).astype(f32) / f32(4294967296.0)
    return np.where(f >= 1, ONE_BELOW, f).astype(f32)


def neighbours(k):
    """The float32 k and its two neighbours, within [0, 1): 0's lower neighbour and 1 and above are left out."""
    k = f32(k)
    c = [np.nextafter(k, f32(-1)), k, np.nextafter(k, f32(2))]
    return [x for x in c if 0 <= x < 1 and (x == 0 or x >= 2.0 ** -8)]


def emit_edges_tables():
    """(emitter records int32 [n, 12], CDF float32) of emit_edges as the device reads them
    (bdpt_scene_export_layout arrays 7 and 9)."""
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    import bdpt_amd

    sc = bdpt_amd.Scene(variants.obj_path("emit_edges"))
    return (np.frombuffer(sc.export_layout(7), np.int32).reshape(-1, 12).copy(),
            np.frombuffer(sc.export_layout(9), f32).copy())


def canonical_fixture(seed=70):
    rng = np.random.default_rng(seed)
    w, cls = [], []
    for name, ws in (("clamp_range", np.arange(0xFFFFFF00, 0x100000000, dtype=np.uint64)), ("zero_one", [0, 1]),
                     ("pow2", [x for k in range(1, 32) for x in (2 ** k - 1, 2 ** k, 2 ** k + 1)]),
                     # ties of the uint32 -> float32 conversion (round to even), either side
                     ("tie", [2 ** k + 2 ** (k - 24) * m for k in range(24, 32) for m in (1, 3)]),
                     ("random", rng.integers(0, 2 ** 32, 4096, dtype=np.uint64))):
        w.append(np.asarray(ws, np.uint64).astype(np.uint32))
        cls += [name] * len(w[-1])
    w = np.concatenate(w)
    out = kat(toml("caustic"), 64, 64, "canonical", w.view(f32), 1)[:, 0]
    np.savez_compressed(os.path.join(HERE, "kat_sampling_canonical.npz"), word=w, cls=np.array(cls), out=out)
    print("canonical", {c: cls.count(c) for c in dict.fromkeys(cls)}, "words >= 0xFFFFFF80:",
          int((w >= 0xFFFFFF80).sum()), "outputs equal to the float below 1:", int((out == ONE_BELOW).sum()))


def warp_fixture(seed=71):
    rng = np.random.default_rng(seed)
    e = np.array([0, 2.0 ** -32, 2.0 ** -24, 0.25, 0.5, 0.75, ONE_BELOW], f32)
    grid = np.stack(np.meshgrid(e, e, indexing="ij"), -1).reshape(-1, 2)
    u = np.concatenate([grid, canonical_np(rng.integers(0, 2 ** 32, (600, 2), dtype=np.uint64))]).astype(f32)
    out = kat(toml("caustic"), 64, 64, "warp", u, 10)
    np.savez_compressed(os.path.join(HERE, "kat_sampling_warp.npz"), u=u, n_grid=grid.shape[0], hemisphere=out[:, 0:3],
                        hemisphere_pdf=out[:, 3], triangle=out[:, 4:6], sphere=out[:, 6:9], sphere_pdf=out[:, 9])
    print("warp", u.shape[0], "records,", grid.shape[0], "on the edge grid")


def emitter_fixture(seed=72):
    """kat_sampling_emitter.npz: selectEmitter + sampleEmitterPosition on emit_edges. Classes:
    knot (u1 on every CDF knot of every emitter, its two float neighbours, 0 and the float below 1),
    select (u0 on k / 5 and two floats either side, the largest word), triangle (each triangle
    draw at 0 and at the float below 1), random."""
    rng = np.random.default_rng(seed)
    em, cdf = emit_edges_tables()
    ne = em.shape[0]
    rnd = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rec, cls = [], []
    for e in range(ne):
        w0 = word_of(f32((e + 0.5) / ne))
        knots = cdf[em[e, 3]: em[e, 3] + em[e, 1] + 1]
        us = [u for k in knots for u in neighbours(k)] + [f32(0), ONE_BELOW]
        w1 = np.concatenate([word_of(np.array(us, f32)), [1]]).astype(np.uint32)  # word 1: the float above 0
        r = np.stack([np.full(w1.size, w0, np.uint32), w1, rnd(w1.size), rnd(w1.size)], 1)
        rec.append(r), cls.append(np.full(w1.size, 0))
        for a in (0, 0xFFFFFFFF):  # triangle draws on their edges, every pairing and each alone
            for b in (0, 0xFFFFFFFF):
                rec.append(np.array([[w0, rnd(1)[0], a, b]], np.uint32)), cls.append([2])
            rec.append(np.stack([np.full(4, w0, np.uint32), rnd(4), np.full(4, a, np.uint32), rnd(4)], 1))
            rec.append(np.stack([np.full(4, w0, np.uint32), rnd(4), rnd(4), np.full(4, a, np.uint32)], 1))
            cls.append(np.full(8, 2))
    sel = []
    for k in range(ne + 1):
        x = f32(k / ne)
        for _ in range(2):
            x = np.nextafter(x, f32(-1))
        for _ in range(5):
            if 0 <= x < 1 and (x == 0 or x >= 2.0 ** -8):
                sel.append(x)
            x = np.nextafter(x, f32(2))
    w0 = np.concatenate([word_of(np.array(sel, f32)), [1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF]]).astype(np.uint32)
    rec.append(np.stack([w0, rnd(w0.size), rnd(w0.size), rnd(w0.size)], 1)), cls.append(np.full(w0.size, 1))
    rec.append(rnd(8000).reshape(2000, 4)), cls.append(np.full(2000, 3))
    rec, cls = np.concatenate(rec).astype(np.uint32), np.concatenate(cls).astype(np.int8)
    out = kat(toml("emit_edges"), 64, 64, "emitter", rec.view(f32), 10)
    np.savez_compressed(os.path.join(HERE, "kat_sampling_emitter.npz"), words=rec, cls=cls,
                        cls_names=np.array(["knot", "select", "triangle", "random"]), emitters=em, cdf=cdf,
                        id=out[:, 0].view(np.int32), emitter_pdf=out[:, 1], face=out[:, 2].view(np.int32),
                        pos=out[:, 3:6], n=out[:, 6:9], area_pdf=out[:, 9])
    print("emitter", rec.shape[0], "records; per class", np.bincount(cls), "per emitter",
          np.bincount(out[:, 0].view(np.int32)))


def camera_fixture(seed=73):
    rng = np.random.default_rng(seed)
    res = {}
    sp = np.array(SPECIAL_WORDS + [0x80000000], np.uint32)
    for W, H, spp in CAMERA_CONFIGS:
        edge = np.array([0, W - 1, W, (H - 1) * W, H * W - 1, (H // 2) * W + W // 2], np.int32)
        pix = np.concatenate([np.repeat(edge, sp.size * sp.size), rng.integers(0, W * H, 300).astype(np.int32)])
        pairs = np.stack(np.meshgrid(sp, sp, indexing="ij"), -1).reshape(-1, 2)
        w = np.concatenate([np.tile(pairs, (edge.size, 1)),
                            rng.integers(0, 2 ** 32, (300, 2), dtype=np.uint64).astype(np.uint32)])
        rec = np.concatenate([pix[:, None].view(np.uint32), w, np.full((pix.size, 1), spp, np.uint32)], 1)
        res[f"rec_{W}x{H}_spp{spp}"] = rec[:, :3].copy()
        res[f"dir_{W}x{H}_spp{spp}"] = kat(toml("caustic", W, H), W, H, "camera", rec.view(f32), 3)
    np.savez_compressed(os.path.join(HERE, "kat_sampling_camera.npz"), **res)
    print("camera", {k: v.shape[0] for k, v in res.items() if k.startswith("rec")})


def sphere_fixture(seed=74):
    """kat_sampling_sphere.npz: sampleSphereByArea / BySolidAngle from points outside, near the
    surface (both sides, the fmax(0, .) branch) and inside, and raySphereIntersect on random rays,
    tangent rays with a discriminant of exactly 0, and axis rays whose two roots are exact, with
    min_t and max_t on, just below and just above each root (min_t >= 0: every ray the path makes)."""
    rng = np.random.default_rng(seed)
    n = 500
    FLT_MAX = f32(3.402823466e38)
    rays, rc, rr, rcls = [], [], [], []
    m = 400  # random rays toward and past random spheres
    c2 = (rng.normal(size=(m, 3)) * 0.5).astype(f32)
    r2 = np.exp(rng.uniform(np.log(0.05), np.log(2.0), m)).astype(f32)
    o = (c2 + unit(rng, m) * (rng.uniform(0.2, 6, m) * r2)[:, None]).astype(f32)
    tgt = c2 + unit(rng, m) * (rng.choice([0.5, 0.99, 0.999999, 1.0, 1.000001, 1.01, 1.5], m) * r2)[:, None]
    d = _normalize(tgt - o)
    mn = rng.choice([1e-8, 1e-3, 1.0], m)
    mx = np.where(rng.random(m) < 0.5, FLT_MAX, np.linalg.norm(tgt - o, axis=1) * rng.choice([0.5, 1.0, 2.0], m))
    rays += list(np.concatenate([o, d, mn[:, None], mx[:, None]], 1))
    rc += list(c2)
    rr += list(r2)
    rcls += [0] * m
    # exact roots: o = c - k x, d = x: t = k - r and k + r; limits on and next to each root
    for k, r in ((4, 1), (3, 2), (8, 0.5), (1, 2), (2, 2)):  # the last two: the origin inside / on the sphere
        t1, t0 = f32(k - r), f32(k + r)
        near = lambda t: [np.nextafter(t, f32(-1e9)), t, np.nextafter(t, f32(1e9))]
        mins = [f32(1e-8)] + [x for x in near(t1) + near(t0) if x >= 0]
        maxs = [x for x in near(t1) + near(t0) if x > 0] + [FLT_MAX, f32(np.inf)]
        for axis in range(3):
            d = np.zeros(3, f32)
            d[axis] = 1
            cc = np.array([1.0, -2.0, 0.5], f32)
            for mn in mins:
                for mx in maxs:
                    rays.append(np.concatenate([cc - k * d, d, [mn, mx]])), rc.append(cc), rr.append(r), rcls.append(1)
    # tangent: o = c - k x + r y, d = x: the discriminant is exactly 0, the root k
    for k in range(1, 9):
        for r in (0.5, 1, 2, 4):
            for axis in range(3):
                d, s = np.zeros(3, f32), np.zeros(3, f32)
                d[axis], s[(axis + 1) % 3] = 1, r
                cc = np.array([0.5, 1.0, -1.5], f32)
                for mn, mx in ((1e-8, FLT_MAX), (k, FLT_MAX), (1e-8, k), (np.nextafter(f32(k), f32(0)), np.nextafter(f32(k), f32(99)))):
                    rays.append(np.concatenate([cc - k * d + s, d, [mn, mx]])), rc.append(cc), rr.append(r), rcls.append(2)
    rays, rc, rr = np.array(rays, f32), np.array(rc, f32), np.array(rr, f32)
    # the first n records also carry a sampling point about their sphere (the rest repeat them)
    cls = np.arange(n) % 5  # 0 far outside, 1 outside, 2 just outside, 3 just inside, 4 inside
    dist = np.choose(cls, [rng.uniform(3, 50, n), rng.uniform(1.05, 3, n),
                           1 + rng.choice([1e-7, 1e-6, 1e-4, 1e-3], n), 1 - rng.choice([1e-7, 1e-6, 1e-4, 1e-3], n),
                           rng.uniform(0.05, 0.95, n)])
    p = (rc[:n] + unit(rng, n) * (dist * rr[:n])[:, None]).astype(f32)
    u = canonical_np(rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64))
    u[:16] = np.array([[a, b] for a in (0, 0.5, ONE_BELOW, 0.25) for b in (0, 0.5, ONE_BELOW, 0.75)], f32)
    k = np.arange(rays.shape[0]) % n
    rec = np.concatenate([u[k], p[k], rc, rr[:, None], rays], 1).astype(f32)
    out = kat(toml("hardlight", kind="direct"), 64, 64, "sphere", rec, 16)
    first = np.arange(rays.shape[0]) < n
    np.savez_compressed(os.path.join(HERE, "kat_sampling_sphere.npz"),
                        u=u, p=p, center=rc[first], radius=rr[first], cls=cls.astype(np.int8),
                        area_pos=out[first, 0:3], area_ne=out[first, 3:6], area_wi=out[first, 6:9], area_pdf=out[first, 9],
                        solid_wi=out[first, 10:13], solid_pdf=out[first, 13],
                        rays=rays, ray_center=rc, ray_radius=rr, ray_cls=np.array(rcls, np.int8),
                        hit=out[:, 14].astype(np.int8), t=out[:, 15])
    print("sphere", n, "sampling records per class", np.bincount(cls), ";", rays.shape[0], "rays per class",
          np.bincount(rcls), "hits", int(out[:, 14].sum()))


def sampler_edges_fixture(scene, rr, n=32, seed=75):
    """kat_sampler_edges_bdpt_<scene>.npz: BDPTIntegrator::render(ray, sampler) from states whose
    next EDGE_DRAWS outputs are given words: the first 12 from SPECIAL_WORDS and the words that land
    on a CDF knot of the scene's emitters, the rest random. Stored as the outputs; the state is
    untemper(outputs) at `pos`, zeros elsewhere. No sample draws past them, so the state after the
    call is the same words at pos_out."""
    sys.path.insert(0, os.path.join(REPO, "bidirectional-path-tracing_amd"))
    import bdpt_amd

    rng = np.random.default_rng(seed)
    sc = bdpt_amd.Scene(variants.obj_path(scene))
    cdf = np.frombuffer(sc.export_layout(9), f32)
    knots = np.unique(cdf[(cdf >= 2.0 ** -8) & (cdf < 1)])
    special = np.concatenate([np.array(SPECIAL_WORDS, np.uint32), word_of(knots)]).astype(np.uint32)
    draws = rng.integers(0, 2 ** 32, (n, EDGE_DRAWS), dtype=np.uint64).astype(np.uint32)
    for i in range(n):
        if i < n // 2:  # every special word visits each of the first 12 draws
            draws[i, :12] = special[(i + 3 * np.arange(12)) % special.size]
        else:
            draws[i, :12] = rng.choice(special, 12)
    pos = rng.choice([0, 17, 200, 624 - EDGE_DRAWS], n).astype(np.uint32)
    st = np.zeros((n, 625), np.uint32)
    for i in range(n):
        st[i, pos[i]: pos[i] + EDGE_DRAWS] = untemper(draws[i])
        st[i, 624] = pos[i]
    W = H = 64
    eye = np.array(variants.SCENES[scene]["camera"]["eye"], f32)
    tgt = np.array([-1.0, 0.0, -1.0]) + rng.random((n, 3)) * np.array([2.0, 1.6, 2.0])
    d = tgt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.repeat(eye[None], n, 0), d, np.ones((n, 1)), np.full((n, 1), 1000.0)], 1).astype(f32)
    name = f"edges_bdpt_{scene}"
    fin, fout = os.path.join(TMP, name + ".in"), os.path.join(TMP, name + ".out")
    np.concatenate([rays, st.view(f32)], 1).astype(f32).tofile(fin)
    run(["sample_state", toml(scene, W, H, 16, rr), str(W), str(H), "16", str(rr), fin, fout, "-"])
    out = np.fromfile(fout, f32).reshape(n, 3 + 625 + 1 + 64)
    so = out[:, 3:628].view(np.uint32)
    assert np.array_equal(so[:, :624], st[:, :624]) and (so[:, 624] <= pos + EDGE_DRAWS).all(), "a sample drew past its words"
    np.savez_compressed(os.path.join(HERE, f"kat_sampler_{name}.npz"), rays=rays, draws=draws, pos=pos,
                        n_special=special.size, Li=out[:, :3], pos_out=so[:, 624].copy(),
                        nsplat=out[:, 628].view(np.int32), splats=out[:, 629:].reshape(n, 16, 4), width=W, height=H,
                        spp=16, rr=rr)
    print("sampler edges", scene, n, "states; draws used", (so[:, 624] - pos).min(), "..", (so[:, 624] - pos).max(),
          "; splat counts", np.bincount(out[:, 628].view(np.int32)), "; nonzero Li", int((out[:, :3] != 0).any(1).sum()))


def sampling_fixtures():
    import json

    canonical_fixture()
    warp_fixture()
    emitter_fixture()
    camera_fixture()
    sphere_fixture()
    sampler_edges_fixture("caustic", 8, seed=75)
    sampler_edges_fixture("emit_edges", 5, seed=76)
    path = os.path.join(HERE, "manifest.json")
    with open(path) as f:
        manifest = json.load(f)
    manifest["sampling_kat"] = {}
    for name in SAMPLING_FILES:
        with open(os.path.join(HERE, name + ".npz"), "rb") as f:
            b = f.read()
        g = np.load(os.path.join(HERE, name + ".npz"))
        manifest["sampling_kat"][name] = dict(bytes=len(b), arrays={k: list(g[k].shape) for k in g.files})
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1)
    print("sampling fixtures:", sum(m["bytes"] for m in manifest["sampling_kat"].values()), "bytes")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "sampling":  # only the sampling-side fixtures
        sampling_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "adversarial":  # only these fixtures
        for i, (sc, n) in enumerate([("caustic", 48000), ("hardlight", 48000), ("synth1m", 30000)]):
            adversarial_fixture(sc, n, seed=40 + i)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "generated":  # only the generated-geometry fixtures
        for name in variants.GEOM_SCENES:
            generated_fixture(name, seed=GEOM_SEEDS[name])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "bsdf_edges":  # only this fixture
        bsdf_edges_fixture()
        return
    if not os.path.exists(REF):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "ref")], check=True)
    for i, sc in enumerate(["caustic", "hardlight", "hardlight_mirror", "hardlight_phong", "cbox_low"]):
        bsdf_fixture(sc, seed=10 + i)
    fresnel_fixture()
    triangle_fixture()
    for i, (sc, n) in enumerate([("caustic", 12000), ("hardlight", 8000), ("cbox_low", 4000)]):
        intersect_fixture(sc, n, seed=20 + i)
    splat_fixture()
    for i, (sc, n) in enumerate([("caustic", 48000), ("hardlight", 48000), ("synth1m", 30000)]):
        adversarial_fixture(sc, n, seed=40 + i)
    bsdf_edges_fixture()
    for name in variants.GEOM_SCENES:
        generated_fixture(name, seed=GEOM_SEEDS[name])
    sampler_fixture("bdpt_caustic", "caustic", toml("caustic", 64, 64, 16, 8), 64, 64, 16, 8, 160, 30)
    sampler_fixture("bdpt_hardlight_rr12", "hardlight", toml("hardlight", 64, 64, 16, 12), 64, 64, 16, 12, 100, 31)
    sampler_fixture("path_caustic", "caustic", toml("caustic", 64, 64, 16, kind="path"), 64, 64, 16, 5, 80, 32)
    sampler_fixture("direct_hardlight", "hardlight",
                    toml("hardlight", 64, 64, 16, kind="direct", strategy="mis", emitter_samples=2, bsdf_samples=2),
                    64, 64, 16, 5, 80, 33)
    sampling_fixtures()


if __name__ == "__main__":
    main()
