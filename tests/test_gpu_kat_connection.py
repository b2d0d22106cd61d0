"""What every BDPT connection evaluates, per function and per compilation.

connectToLight, connectToCamera and connectVertices go through local_for + bsdf_eval_pdfs
(dev_shade.hpp): the fused one-powf form of eval / pdf / reverse pdf and the diffuse frame
skip, which bsdf_eval / bsdf_pdf (test_gpu_kat.py) never reach. The frame kernels compile
them three ways; bdpt_bsdf_eval_pdfs / bdpt_bsdf_local_for run each:
  exact  IEEE weights: bit-equal to the reference's BSDF::eval / pdf, the reverse pdf to
         pdf of the swapped pair
  ng     the build without glossy lobes: the same bits on diffuse, mirror and glass records
  fast   the default frame kernels' arithmetic: the same bits wherever no Phong power enters,
         within the allowance below where one does

Fixture: tests/golden/kat_bsdf_edges.npz (make_kat_goldens.py bsdf_edges_fixture, from the
unmodified reference) on scenes/kat/bsdf_edges.obj: Phong at Ns 0, 1, 100, 1000 and the largest
finite float, mixtures with Ks = 0, specw 0, specw 1 and ordinary, diffuse, mirror, glass and
the null BSDF; directions with wi = reflect(wo) exactly and nudged by 1..8 ulp (the float32 lobe
cosine z lands below, on and above 1), z chosen for small unflushed powers (ex |log2 z| in
[60, 126]) and for powers below 2^-126, zero / signed-zero / 1e-30 / denormal cosines, grazing,
lower hemisphere, and the random mix of the other BSDF fixtures.

Allowance of the fast build (pow_w = exp2(ex * log2 z) on v_log_f32 / v_exp_f32, both 1 ulp by
the ISA): log2 z carries a relative 2^-23, the product ex * log2 z another 2^-24, which move the
result by ln2 * ex |log2 z| * (2^-23 + 2^-24) relatively, and exp2 adds its own 2^-23; K = 2
covers second-order terms: A = K (ln2 ex |log2 z| (2^-23 + 2^-24) + 2^-23). After the power,
eval is at most four float32 operations (times the Ks factor, plus Kd / pi, times scale, times
cos) and the mixture pdf three, each rounded once on either side: + 4 * 2^-23. Every term of
those sums is non-negative, so the relative bound of the power term bounds the sum. Where the
reference's power is below 2^-126 the hardware may return 0 for it: the power's whole
contribution, at most 2 (ex + 2) / (2 pi) * power, is allowed as an absolute difference there.
"""
import os

import numpy as np
import pytest

import bdpt_amd
import variants
from conftest import REPO, load_golden
from test_kat_connection_cpu import bits_equal, np_dot, np_to_local

pytestmark = pytest.mark.gpu

GOLD = os.path.join(REPO, "tests", "golden")
EDGES_OBJ = os.path.join(REPO, "scenes", "kat", "bsdf_edges.obj")
BSDF_SCENES = ["caustic", "hardlight", "hardlight_mirror", "hardlight_phong", "cbox_low"]
f32 = np.float32
TOL = 1e-4  # the suite's per-pixel frame bound (test_gpu_parity.py)
K = 2.0
U = 2.0 ** -23
# records on the device after the upload (bdpt_capi.cpp device_bsdfs: a Mixture with Ks = 0 and
# scale 1 becomes a diffuse record)
DIFFUSE = ("light", "diffuse", "mixKs0")
DELTA = ("mirror", "glass")
NO_POWER = DIFFUSE + DELTA + ("mixKs0Scaled",)  # no output holds a Phong power
PHONG = ("phongNs0", "phongNs1", "phongNs100", "phongNs1000", "phongNsMax")
MIX_POWER_PDF = ("mixSpecw1", "mixOrdinary")  # mixtures whose pdf holds the lobe's (specw != 0)

_cache = {}


def edges():
    if "g" not in _cache:
        g = dict(np.load(os.path.join(GOLD, "kat_bsdf_edges.npz")))
        g["names"] = [str(x) for x in g["names"]]
        g["live"] = g["null"][g["mat"]] == 0
        _cache["g"] = g
    return _cache["g"]


def integrator(obj):
    if obj not in _cache:
        cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.CBOX_CAMERA), width=32, height=32, spp=1, rr_depth=5)
        it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(obj), cfg)
        it.init()
        _cache[obj] = it
    return _cache[obj]


def eq(a, b):
    """Element-wise: the same bits, or equal values (+0 and -0)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (a == b)


def mats_named(g, names):
    return np.isin(g["mat"], [g["names"].index(n) for n in names])


def lobe_z(wo, wi):
    return np_dot(wi, np.asarray(wo, f32) * np.array([-1, -1, 1], f32))


# ------------------------------------------------------------------ exact build
def test_gpu_exact_eval_pdfs_match_reference_on_edges():
    """f = BSDF::eval, fwd = BSDF::pdf, rev = BSDF::pdf of the swapped pair, bit for bit, on every
    material and direction class of the edge fixture."""
    g = edges()
    k = g["live"]
    f, fwd, rev = integrator(EDGES_OBJ).bsdf_eval_pdfs(g["mat"][k], g["wo"][k], g["wi"][k])
    for name, got, ref in (("f", f, g["eval"][k]), ("fwd", fwd, g["pdf"][k]), ("rev", rev, g["pdf_rev"][k])):
        bad = ~eq(got, ref).reshape(got.shape[0], -1).all(1)
        assert not bad.any(), (name, int(bad.sum()), np.unique(np.array(g["names"])[g["mat"][k][bad]]),
                               np.bincount(g["cls"][k][bad]))


@pytest.mark.parametrize("scene", BSDF_SCENES)
def test_gpu_exact_eval_pdfs_match_reference_on_scene_fixtures(scene):
    g = np.load(os.path.join(GOLD, f"kat_bsdf_{scene}.npz"))
    live = g["null"] == 0
    it = integrator(variants.obj_path(scene))
    f, fwd, _ = it.bsdf_eval_pdfs(g["mat"][live], g["wo"][live], g["wi"][live])
    assert bits_equal(f, g["eval"][live]) and bits_equal(fwd, g["pdf"][live])


def test_gpu_eval_pdf_sample_match_reference_on_edges():
    """The walks' bsdf_eval / bsdf_pdf / bsdf_sample on the edge fixture: Ns > 100 and z ~ 1."""
    g = edges()
    it = integrator(EDGES_OBJ)
    k = g["live"]
    assert bits_equal(it.bsdf_eval(g["mat"][k], g["wo"][k], g["wi"][k]), g["eval"][k])
    assert bits_equal(it.bsdf_pdf(g["mat"][k], g["wo"][k], g["wi"][k]), g["pdf"][k])
    assert bits_equal(it.bsdf_pdf(g["mat"][k], g["wi"][k], g["wo"][k]), g["pdf_rev"][k])
    s = g["sample_idx"]
    ls = g["live"][s]
    sf, swi, spdf = it.bsdf_sample(g["mat"][s][ls], g["wo"][s][ls], g["u"][ls])
    assert bits_equal(sf, g["sample_f"][ls]) and bits_equal(swi, g["sample_wi"][ls])
    assert bits_equal(spdf, g["sample_pdf"][ls])
    for m, name in enumerate(g["names"]):
        t, _ = it.scene.bsdf_type(m)
        assert t == int(g["type"][m]), name


# ------------------------------------------------------------------ ng build
def ng_scene(tmp):
    """The light, diffuse, mirror and glass materials of bsdf_edges.mtl as a scene of their own
    (a table the build without glossy lobes accepts): (obj path, their names in index order)."""
    keep = ["light", "diffuse", "mirror", "glass"]
    with open(os.path.splitext(EDGES_OBJ)[0] + ".mtl") as f:
        blocks = f.read().split("newmtl ")[1:]
    blocks = {b.split()[0]: b for b in blocks}
    (tmp / "ng.mtl").write_text("".join("newmtl " + blocks[n] for n in keep))
    lines = ["mtllib ng.mtl", "vn 0 1 0", "vn 0 -1 0"]
    for i, n in enumerate(keep):
        lines += [f"v {2 * i} {2 if i == 0 else 0} 0", f"v {2 * i + 1} {2 if i == 0 else 0} 0",
                  f"v {2 * i} {2 if i == 0 else 0} {1 if i == 0 else -1}", f"o {n}", f"usemtl {n}",
                  "f {0}//{3} {1}//{3} {2}//{3}".format(3 * i + 1, 3 * i + 2, 3 * i + 3, 2 if i == 0 else 1)]
    (tmp / "ng.obj").write_text("\n".join(lines) + "\n")
    return str(tmp / "ng.obj"), keep


def test_gpu_ng_build_matches_goldens_on_diffuse_mirror_glass(tmp_path):
    g = edges()
    obj, keep = ng_scene(tmp_path)
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.CBOX_CAMERA), width=32, height=32, spp=1, rr_depth=5)
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(obj), cfg)
    for m, name in enumerate(keep):
        k = g["mat"] == g["names"].index(name)
        assert it.scene.bsdf_type(m)[0] == int(g["type"][g["names"].index(name)])
        mat = np.full(int(k.sum()), m, np.int32)
        f, fwd, rev = it.bsdf_eval_pdfs(mat, g["wo"][k], g["wi"][k], build="ng")
        assert bits_equal(f, g["eval"][k]), name
        assert bits_equal(fwd, g["pdf"][k]), name
        assert bits_equal(rev, g["pdf_rev"][k]), name
        n, v = local_for_inputs(int(k.sum()))
        loc = it.bsdf_local_for(mat, n, v, build="ng")
        assert bits_equal(loc[:, 2], np_dot(v, n)) and not loc[:, :2].any(), name
        # and the other compilations on the same table
        for build in ("exact", "fast"):
            f2, fwd2, rev2 = it.bsdf_eval_pdfs(mat, g["wo"][k], g["wi"][k], build=build)
            assert bits_equal(f2, f) and bits_equal(fwd2, fwd) and bits_equal(rev2, rev), (name, build)


def test_gpu_ng_build_is_refused_on_a_glossy_or_null_table():
    g = edges()
    one = np.array([[0, 0, 1]], f32)
    for obj in (EDGES_OBJ, variants.obj_path("hardlight")):  # glossy + null records; one Mixture
        it = integrator(obj)
        for call in (it.bsdf_eval_pdfs, it.bsdf_local_for):
            with pytest.raises(bdpt_amd.BdptError) as e:
                call([g["names"].index("diffuse") if obj == EDGES_OBJ else 0], one, one, build="ng")
            assert e.value.code == bdpt_amd.ERR_UNSUPPORTED


# ------------------------------------------------------------------ local_for
def local_for_inputs(n, seed=5):
    """Unit normals (the reference's interpolated and flat shading normals of the hardlight
    fixture, the axes, |n.x| == |n.y| ties, n along z) and world directions (the hits' own
    -d, random ones, some orthogonal to n)."""
    rng = np.random.default_rng(seed)
    gi = np.load(os.path.join(GOLD, "kat_intersect_hardlight.npz"))
    hit = gi["out"][:, 0] == 1
    nrm, d = gi["out"][hit, 10:13], -gi["rays"][hit, 3:6]
    idx = rng.integers(0, nrm.shape[0], n)
    nn, v = nrm[idx].astype(f32).copy(), d[idx].astype(f32).copy()
    r = rng.normal(size=(n, 3))
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(f32)
    v[n // 3:] = r[n // 3:]
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                        [0.5, 0.5, 0.70710677], [-0.5, 0.5, 0.70710677], [0.6, -0.6, 0.52915025]], f32)
    nn[: special.shape[0] * 4] = np.tile(special, (4, 1))
    v[:6] = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0]], f32)  # orthogonal to n
    return nn, v


@pytest.mark.parametrize("build", ["exact", "fast"])
def test_gpu_local_for_matches_numpy_frame(build):
    """z = (v.x n.x + v.y n.y) + v.z n.z for every kind; x and y the float32 restatement of
    make_frame / to_local for the kinds that keep a frame, 0 for diffuse records."""
    g = edges()
    it = integrator(EDGES_OBJ)
    per = 600
    nn, v = local_for_inputs(per)
    for m, name in enumerate(g["names"]):
        loc = it.bsdf_local_for(np.full(per, m, np.int32), nn, v, build=build)
        assert bits_equal(loc[:, 2], np_dot(v, nn)), name
        if name in DIFFUSE:
            assert not loc[:, :2].any(), name
        else:
            assert bits_equal(loc, np_to_local(nn, v)), name
    assert np.abs(v[:, 0]).max() > 0.9 and np.abs(np_to_local(nn, v)[:, :2]).max() > 0.9  # x, y are exercised


# ------------------------------------------------------------------ fast build
def test_gpu_fast_build_is_bit_equal_where_no_phong_power_enters():
    """Diffuse and delta records, mixtures with Ks = 0 and specw == 0 (all three outputs), the
    cosine pdfs of the specw == 0 mixture with Ks != 0, and every fwd / rev with z < 0."""
    g = edges()
    k = g["live"]
    mat, wo, wi = g["mat"][k], g["wo"][k], g["wi"][k]
    f, fwd, rev = integrator(EDGES_OBJ).bsdf_eval_pdfs(mat, wo, wi, build="fast")
    gk = {x: g[x][k] for x in ("mat", "eval", "pdf", "pdf_rev")}
    gk["names"] = g["names"]
    plain = mats_named(gk, NO_POWER)
    assert plain.sum() == 2000 * len(NO_POWER)
    assert eq(f[plain], gk["eval"][plain]).all()
    cos_pdf = plain | mats_named(gk, ("mixSpecw0",)) | (lobe_z(wo, wi) < 0)
    assert (lobe_z(wo, wi) < 0)[~plain].sum() > 1000
    assert eq(fwd[cos_pdf], gk["pdf"][cos_pdf]).all()
    assert eq(rev[cos_pdf], gk["pdf_rev"][cos_pdf]).all()


def test_gpu_fast_build_phong_outputs_within_the_log_exp_allowance(capsys):
    """Measured on an MI355X: worst error / allowance 0.360 (phongNs1000 fwd / rev; 0.31 - 0.35
    for the other Phong pdfs, 0.09 - 0.32 for eval) over the records whose reference power is
    >= 2^-126."""
    g = edges()
    it = integrator(EDGES_OBJ)
    worst = {}
    for name in PHONG + MIX_POWER_PDF + ("mixSpecw0",):
        m = g["names"].index(name)
        k = g["mat"] == m
        wo, wi, ex = g["wo"][k], g["wi"][k], float(g["ns"][m])
        f, fwd, rev = it.bsdf_eval_pdfs(g["mat"][k], wo, wi, build="fast")
        z = lobe_z(wo, wi).astype(np.float64)
        eval_on = (wi[:, 2] >= 0) & (wo[:, 2] >= 0)
        zc = np.clip(z, 0.0, None)  # the pdfs take z >= 0 as it is, eval clamps to [0, 1]
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            t_pdf = np.where(zc > 0, ex * np.abs(np.log2(np.where(zc > 0, zc, 1.0))), np.inf if ex > 0 else 0.0)
            p_pdf = np.where(zc > 0, np.exp2(-t_pdf * np.sign(1 - zc)), 0.0 if ex > 0 else 1.0)
        t_ev, p_ev = np.where(z > 1, 0.0, t_pdf), np.where(z > 1, 1.0, p_pdf)
        coef = 2.0 * (ex + 2.0) / (2.0 * np.pi)
        checks = [("f", f, g["eval"][k], np.repeat(eval_on[:, None], 3, 1), t_ev[:, None], p_ev[:, None])]
        if name != "mixSpecw0":
            on = z >= 0
            checks += [("fwd", fwd, g["pdf"][k], on, t_pdf, p_pdf), ("rev", rev, g["pdf_rev"][k], on, t_pdf, p_pdf)]
        for what, got, ref, bearing, t, p in checks:
            same = eq(got, ref)
            assert same[~bearing].all(), (name, what, "an output without a Phong power differs")
            t, p = np.broadcast_to(t, got.shape), np.broadcast_to(p, got.shape)
            flushed = p < 2.0 ** -126
            A = K * (np.log(2.0) * np.where(np.isfinite(t), t, 0.0) * (U + U / 2) + U) + 4 * U
            ref64, got64 = ref.astype(np.float64), got.astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                allow = A * np.abs(ref64) + np.where(flushed, coef * p, 0.0) + 2.0 ** -147
                err = np.abs(got64 - ref64)
            ok = same | (np.isfinite(got) & (err <= allow))
            bad = bearing & ~ok
            assert not bad.any(), (name, what, int(bad.sum()), got[bad][:4], ref[bad][:4], np.bincount(
                np.broadcast_to(g["cls"][k].reshape((-1,) + (1,) * (got.ndim - 1)), got.shape)[bad]))
            live = bearing & ~flushed & np.isfinite(ref) & (ref != 0) & ~same
            # the allowance itself stays under the frame bound on every unflushed record
            assert (A[bearing & ~flushed & np.isfinite(ref)] < TOL).all(), (name, what)
            if live.any():
                worst[(name, what)] = float((err[live] / allow[live]).max())
    with capsys.disabled():
        for key, r in sorted(worst.items()):
            print(f"\nfast build {key[0]:12s} {key[1]:3s} worst error / allowance {r:.3f}", end="")
        print(f"\nfast build worst error / allowance overall {max(worst.values()):.3f}")
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------ fast scalar operations
def magnitudes(rng, n, signed=True):
    x = np.exp2(rng.uniform(-100, 100, n)) * (rng.choice([-1.0, 1.0], n) if signed else 1.0)
    return x.astype(f32)


def ulps(got, exact):
    """|got - exact| in units of the float32 spacing at exact."""
    with np.errstate(over="ignore"):  # (quotients beyond the float range are masked by the caller)
        ref = exact.astype(f32)
    return np.abs(got.astype(np.float64) - exact) / np.spacing(np.abs(ref)).astype(np.float64)


def test_gpu_fast_scalar_ops_within_documented_ulps(capsys):
    """rcp_w, sqrt_w, rsqrt_w within 1 ulp of the float64 value (v_rcp_f32 / v_sqrt_f32 /
    v_rsq_f32: 1 ulp), div_w = x * rcp(y) within 2 (the reciprocal's ulp plus the product's
    rounding), over magnitudes in [2^-100, 2^100]; div_w where the quotient is a normal float.
    Measured on an MI355X: rcp_w 0.881, sqrt_w 0.911, rsqrt_w 0.844, div_w 1.783 ulp."""
    rng = np.random.default_rng(11)
    n = 200000
    x, y, xp = magnitudes(rng, n), magnitudes(rng, n), magnitudes(rng, n, signed=False)
    x64, y64, xp64 = x.astype(np.float64), y.astype(np.float64), xp.astype(np.float64)
    res = {
        "rcp_w": (ulps(bdpt_amd.debug_math("rcp_w", x), 1.0 / x64), 1.0),
        "sqrt_w": (ulps(bdpt_amd.debug_math("sqrt_w", xp), np.sqrt(xp64)), 1.0),
        "rsqrt_w": (ulps(bdpt_amd.debug_math("rsqrt_w", xp), 1.0 / np.sqrt(xp64)), 1.0),
    }
    q = x64 / y64
    normal = (np.abs(q) >= 2.0 ** -126) & (np.abs(q) < 2.0 ** 127)
    assert normal.sum() > n // 2
    res["div_w"] = (ulps(bdpt_amd.debug_math("div_w", x, y), q)[normal], 2.0)
    with capsys.disabled():
        for fn, (e, bound) in res.items():
            print(f"\n{fn}: worst {e.max():.3f} ulp (bound {bound:g})", end="")
        print()
    for fn, (e, bound) in res.items():
        assert e.max() <= bound, (fn, e.max())


def test_gpu_pow_w_within_the_log_exp_allowance(capsys):
    """pow_w itself over x in (0, 1] (and just above 1) and exponents 0 .. 1e4, where the result
    is a normal float: relative error within A of the module docstring; y == 0 gives exactly 1,
    also for x == 0. Measured on an MI355X: worst error / allowance 0.428."""
    rng = np.random.default_rng(12)
    n = 200000
    y = rng.choice(np.array([0, 1, 2, 9.803922, 29.411765, 100, 1000, 2500, 4000, 10000], f32), n)
    with np.errstate(divide="ignore"):
        x = np.exp2(-rng.uniform(0, 126, n) / np.maximum(y.astype(np.float64), 1.0)).astype(f32)
    x[:1000] = np.nextafter(f32(1), f32(2))
    x[1000:2000] = f32(1)
    x[2000:2100] = f32(0)
    got = bdpt_amd.debug_math("pow_w", x, y).astype(np.float64)
    assert (got[y == 0] == 1.0).all() and (y[2000:2100] == 0).any()
    t = y.astype(np.float64) * np.abs(np.log2(np.where(x > 0, x.astype(np.float64), 1.0)))
    exact = np.where(x > 0, np.exp2(np.where(x > 1, t, -t)), np.where(y == 0, 1.0, 0.0))
    normal = (exact >= 2.0 ** -126) & (x > 0)
    A = K * (np.log(2.0) * t * (U + U / 2) + U)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.abs(got - exact) / exact / A)[normal]
    with capsys.disabled():
        print(f"\npow_w: worst error / allowance {ratio.max():.3f} over {int(normal.sum())} normal results")
    assert ratio.max() <= 1.0
    assert (got[(x == 0) & (y > 0)] == 0).all()


def test_gpu_fast_scalar_ops_give_no_nan_where_ieee_gives_none(capsys):
    """Zero, denormal, huge and infinite inputs of rcp_w / sqrt_w / rsqrt_w / div_w: only that no
    NaN appears where the IEEE operation has none. What they return is printed (recorded in
    DESIGN.md section 1). pow_w's values outside its contract (x in [0, 1] or just above, finite
    y >= 0) are printed too, without an assertion.

    On an MI355X no NaN appears. Far from IEEE, since denormal inputs read as 0 and denormal
    results are flushed: rcp_w(+-3e38) = +-0, sqrt_w(1e-40) = 0, rsqrt_w(1e-40) = inf,
    div_w(1e-40, 1e-40) = inf, div_w(2^-126, 1e-40) = inf, div_w(3e38, 3e38) = 0. (Before div_w
    passed its product through v_div_fixup_f32, div_w(+-0, +-1e-40) and div_w(+-inf, +-3e38)
    were NaN: 0 * inf and inf * 0.) pow_w(1, inf) = NaN, pow_w(1e-40, y > 0) = 0."""
    tiny, huge, inf = f32(1e-40), f32(3e38), f32(np.inf)
    one = np.array([0.0, -0.0, tiny, -tiny, f32(2.0 ** -126), huge, -huge, inf, -inf], f32)
    pos = np.array([0.0, tiny, f32(2.0 ** -126), huge, inf], f32)
    xa, ya = (a.reshape(-1).astype(f32) for a in np.meshgrid(one, one, indexing="ij"))
    pz = np.array([0.0, tiny, f32(2.0 ** -126), 0.5, 1.0, np.nextafter(f32(1), f32(2)), huge, inf], f32)
    py = np.array([0.0, tiny, 1.0, 100.0, huge, inf], f32)
    px, pyy = (a.reshape(-1).astype(f32) for a in np.meshgrid(pz, py, indexing="ij"))
    with np.errstate(all="ignore"):
        cases = [("rcp_w", one, None, f32(1) / one), ("sqrt_w", pos, None, np.sqrt(pos)),
                 ("rsqrt_w", pos, None, f32(1) / np.sqrt(pos)), ("div_w", xa, ya, xa / ya),
                 ("pow_w", px, pyy, np.power(px.astype(np.float64), pyy.astype(np.float64)).astype(f32))]
    failures = []
    with capsys.disabled():
        for fn, a, b, ieee in cases:
            got = bdpt_amd.debug_math(fn, a, b)
            print(f"\n{fn} on edge inputs:")
            for i in range(a.size):
                arg = f"{a[i]:g}" if b is None else f"{a[i]:g}, {b[i]:g}"
                note = ""
                if np.isnan(got[i]) and not np.isnan(ieee[i]):
                    note = "   <-- NaN where IEEE has none"
                    if fn != "pow_w":
                        failures.append((fn, arg, float(ieee[i])))
                if got[i] != ieee[i] or note:
                    print(f"  {fn}({arg}) = {got[i]:g} (IEEE {ieee[i]:g}){note}")
    assert not failures, failures


# ------------------------------------------------------------------ frame
@pytest.mark.parametrize("build", ["default", "split"])
def test_gpu_high_ns_frame_matches_reference(build, golden_manifest, monkeypatch):
    """A Phong lobe of Ns 4000 in a frame, on the default frame kernel and on the short-subpath
    build (BDPT_SPLIT_MAX_RR raised to the frame's rrDepth), against the reference's frame."""
    name = "G13_hardlight_phong_ns4000_32x32_spp4"
    m = golden_manifest["framebuffers"][name]
    monkeypatch.delenv("BDPT_NG_BUILD", raising=False)
    if build == "split":
        monkeypatch.setenv("BDPT_SPLIT_MAX_RR", str(m["rr_depth"]))
    else:
        monkeypatch.delenv("BDPT_SPLIT_MAX_RR", raising=False)
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**variants.SCENES[m["scene"]]["camera"]), width=m["width"],
                          height=m["height"], spp=m["spp"], rr_depth=m["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(m["scene"])), cfg)
    it.init()
    fb = it.render_frame().reshape(-1, 3).astype(np.float64)
    st = it.stats()
    assert st["kernel"] == ("bdpt_frame_kernel_split" if build == "split" else "bdpt_frame_kernel")
    assert st["kernel_glossy"] == 1 and st["samples"] == m["samples"]
    ref = load_golden(name).reshape(-1, 3).astype(np.float64)
    err = np.linalg.norm(fb - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-8)
    print(f"{name} on {st['kernel']}: max per-pixel rel L2 {err.max():.3g}")
    assert np.isfinite(fb).all() and err.max() <= TOL
