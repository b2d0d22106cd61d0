"""The sampling-side fixtures (tests/golden/kat_sampling_*.npz, kat_sampler_edges_*.npz, made by
make_kat_goldens.py `sampling` from the unmodified reference) hold the records that
tests/test_gpu_kat_sampling.py relies on, checked without a GPU: every edge class is populated,
the word -> state inversion the fixtures rest on is an inversion, and the reference's own
answers say what std::generate_canonical does with the largest draws."""
import ctypes
import json
import os
import sys

import numpy as np

import bdpt_amd
from conftest import REPO

GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, GOLD)
import make_kat_goldens as mk  # noqa: E402

f32 = np.float32


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def test_fixtures_are_present_and_listed():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        m = json.load(f)
    assert sorted(m["sampling_kat"]) == sorted(mk.SAMPLING_FILES)
    total = os.path.getsize(os.path.join(GOLD, "G14_emit_edges_32x32_spp4.npz"))
    assert "G14_emit_edges_32x32_spp4" in m["framebuffers"]
    for name, ent in m["sampling_kat"].items():
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) == ent["bytes"], name
        g = np.load(path)
        assert {k: list(g[k].shape) for k in g.files} == ent["arrays"], name
        total += ent["bytes"]
    assert total < 300 * 1024, total


def test_untemper_inverts_temper():
    w = np.random.default_rng(5).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    w[:4] = [0, 1, 0x80000000, 0xFFFFFFFF]
    assert np.array_equal(mk.temper(mk.untemper(w)), w)
    assert np.array_equal(mk.untemper(mk.temper(w)), w)
    # temper is std::mt19937's: output 0 of seed 5489 is 3499211612 from state word x[397] ^ twist(x[0], x[1])
    rs = np.random.RandomState(5489)
    out = rs.randint(0, 2 ** 32, 3, dtype=np.uint32)
    key = rs.get_state()[1]  # the state after the first twist
    assert np.array_equal(mk.temper(key[:3]), out) and out[0] == 3499211612


def test_canonical_records():
    g = load("kat_sampling_canonical")
    w, cls, out = g["word"], g["cls"], g["out"]
    n = {c: int((cls == c).sum()) for c in np.unique(cls)}
    assert n == dict(clamp_range=256, zero_one=2, pow2=93, tie=16, random=4096)
    assert set(range(0xFFFFFF00, 0x100000000)) <= set(int(x) for x in w)
    assert {0, 1} <= set(int(x) for x in w[cls == "zero_one"])
    for k in range(1, 32):
        assert {2 ** k - 1, 2 ** k, 2 ** k + 1} <= set(int(x) for x in w[cls == "pow2"]), k
    assert int((w >= 0xFFFFFF80).sum()) >= 128
    # the reference's answers alone: next() stays in [0, 1), also for the draws that round to 1
    assert ((out >= 0) & (out < 1)).all()
    assert (out[w >= 0xFFFFFF80] == mk.ONE_BELOW).all()
    # and they are the conversion the device restates (float32(word) / 2^32, moved below 1)
    assert np.array_equal(mk.canonical_np(w).view(np.uint32), out.view(np.uint32))


def test_warp_and_sphere_records():
    g = load("kat_sampling_warp")
    u = g["u"]
    assert int(g["n_grid"]) == 49 and u.shape[0] == 49 + 600 and ((u >= 0) & (u < 1)).all()
    for a in (0, mk.ONE_BELOW):
        for b in (0, mk.ONE_BELOW):
            assert ((u[:, 0] == f32(a)) & (u[:, 1] == f32(b))).any()
    s = load("kat_sampling_sphere")
    assert np.array_equal(np.bincount(s["cls"]), [100] * 5)
    d = np.linalg.norm(s["p"].astype(np.float64) - s["center"], axis=1) / s["radius"]
    cls = s["cls"]  # 0 far outside, 1 outside, 2 / 3 within 1e-3 radii of the surface, 4 inside
    assert (d[cls <= 1] > 1).all() and (d[cls == 4] < 1).all() and (np.abs(d[(cls == 2) | (cls == 3)] - 1) < 2e-3).all()
    # inside, sinThetaMaxSquared > 1 takes the fmax(0, .) branch: cosThetaMax = 0, pdf = 1 / (2 pi);
    # near the surface both sides of it occur
    inv2pi = f32(0.15915494309189535)
    assert (s["solid_pdf"][cls == 4] == inv2pi).all() and np.isfinite(s["solid_wi"]).all()
    near = s["solid_pdf"][(cls == 2) | (cls == 3)]
    assert (near == inv2pi).any() and (near != inv2pi).any() and np.isfinite(near).all()
    assert np.array_equal(np.bincount(s["ray_cls"]), [400, 672, 384])
    for c in range(3):  # random, exact roots against min_t / max_t, discriminant exactly 0: hits and misses in each
        h = s["hit"][s["ray_cls"] == c]
        assert 0 < h.sum() < h.size, c
    assert (s["rays"][:, 6] >= 0).all()


def test_emitter_records():
    g = load("kat_sampling_emitter")
    em, cdf, cls, w = g["emitters"], g["cdf"], g["cls"], g["words"]
    assert [str(x) for x in g["cls_names"]] == ["knot", "select", "triangle", "random"]
    assert em.shape[0] == 5 and sorted(em[:, 1]) == [1, 2, 2, 3, 33]
    assert np.array_equal(np.bincount(cls), [132, 27, 100, 2000])
    u = mk.canonical_np(w)
    for e in range(5):
        k = cdf[em[e, 3]: em[e, 3] + em[e, 1] + 1]
        sel = (cls == 0) & (g["id"] == e)
        got = set(u[sel, 1].view(np.uint32).tolist())
        for knot in k:  # every knot and its float neighbours below 1, 0, the float above 0, the float below 1
            for x in mk.neighbours(knot):
                assert f32(x).view(np.uint32) in got, (e, knot, x)
        assert {0, f32(2.0 ** -32).view(np.uint32), mk.ONE_BELOW.view(np.uint32)} <= got, e
        faces = g["face"][g["id"] == e]
        assert faces.min() == 0 and faces.max() == em[e, 1] - 1, e  # its first face and its last are selected
        t = u[(cls == 2) & (g["id"] == e), 2:]
        for a in (0, mk.ONE_BELOW):
            for b in (0, mk.ONE_BELOW):
                assert ((t[:, 0] == f32(a)) & (t[:, 1] == f32(b))).any(), (e, a, b)
    # equal consecutive knots (the zero-area face) and distinct knots one and two ulp apart (the 33 faces' tail)
    z = em[3]
    kz = cdf[z[3]: z[3] + z[1] + 1]
    assert kz[1] == kz[2]
    k33 = cdf[em[1, 3]: em[1, 3] + 34]
    gaps = np.diff(k33.view(np.int32))
    assert (gaps == 1).any() and (gaps == 2).any() and (gaps >= 1).all()
    areas = np.diff(k33.astype(np.float64))
    assert areas.max() / areas[areas > 0].min() >= 1e4  # the face areas span at least 1e4 : 1
    # u0 on k / 5 and two floats either side (within [0, 1)), and the words of the clamp range
    u0 = set(u[cls == 1, 0].view(np.uint32).tolist())
    for k in range(6):
        x = f32(k / 5)
        for step in range(-2, 3):
            y = x
            for _ in range(abs(step)):
                y = np.nextafter(y, f32(2 if step > 0 else -1))
            if 0 <= y < 1 and y >= 2.0 ** -8:
                assert y.view(np.uint32) in u0, (k, step)
    assert {0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF} <= set(w[cls == 1, 0].tolist())
    # selectEmitter's min(id, n - 1) cannot bind for a draw below 1: u0 * n rounds to n for no float
    # u0 <= 1 - 2^-24 (n * 2^-24 is a whole ulp of the floats below n or more), so the largest draw
    # selects n - 1 by truncation alone; recorded here for every emitter count the float can tell apart
    n = np.arange(1, 4097, dtype=f32)
    assert ((mk.ONE_BELOW * n) < n).all()
    assert (g["id"][(w[:, 0] >= 0xFFFFFF00)] == 4).all()


def test_camera_records():
    g = load("kat_sampling_camera")
    for W, H, spp in mk.CAMERA_CONFIGS:
        rec, d = g[f"rec_{W}x{H}_spp{spp}"], g[f"dir_{W}x{H}_spp{spp}"]
        assert rec.shape == (450, 3) and d.shape == (450, 3)
        pix = rec[:, 0].view(np.int32)
        assert pix.min() == 0 and pix.max() == W * H - 1
        assert {0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0} <= set(rec[:, 1].tolist()) & set(rec[:, 2].tolist())
    # spp == 1 draws nothing: the same pixel gives the same direction whatever the words
    rec, d = g["rec_80x48_spp1"], g["dir_80x48_spp1"]
    same = rec[:, 0] == rec[0, 0]
    assert same.sum() > 1 and (d[same].view(np.uint32) == d[0].view(np.uint32)).all()
    rec, d = g["rec_80x48_spp4"], g["dir_80x48_spp4"]
    same = rec[:, 0] == rec[0, 0]
    assert len({tuple(x) for x in d[same].view(np.uint32).tolist()}) > 1  # the jitter branch moves it


def test_sampler_edges_records():
    for scene in ("caustic", "emit_edges"):
        g = load(f"kat_sampler_edges_bdpt_{scene}")
        draws, pos = g["draws"], g["pos"]
        assert draws.shape == (32, mk.EDGE_DRAWS) and (pos + mk.EDGE_DRAWS <= 624).all()
        assert (g["pos_out"] > pos).all() and (g["pos_out"] <= pos + mk.EDGE_DRAWS).all()
        first = draws[:, :12]
        for w in mk.SPECIAL_WORDS:
            assert (first == w).any(), (scene, hex(w))
        assert int(g["n_special"]) > len(mk.SPECIAL_WORDS)  # words that land on a CDF knot
        assert (g["Li"] != 0).any()


def test_debug_sampling_symbol_and_argument_checks():
    L = bdpt_amd.lib()
    out = np.zeros(4, np.uint32)
    got = ctypes.c_int32(7)
    assert L.bdpt_debug_sampling(None, None, 0, 0, 0, 1, out.ctypes.data, out.ctypes.data,
                                 ctypes.byref(got)) == bdpt_amd.ERR_INVALID
    with open(os.path.join(REPO, "include", "bdpt_amd.h")) as f:
        header = f.read()
    for name, (code, _, _) in bdpt_amd.SAMPLING_FNS.items():
        assert f"#define BDPT_SAMPLING_{name.upper()} {code}\n" in header, name
    for name, code in bdpt_amd.EMITTER_PLACEMENTS.items():
        assert f"#define BDPT_EMITTERS_{name.upper()} {code}\n" in header, name
