"""Display output without a GPU: the threshold tables of bdpt_display_thresholds against the curves in float64,
properties of the numpy restatements (display_numpy, meter_numpy) that the GPU tests take as the expected
bits, the PNG and PPM writers against the stdlib's zlib and the texture reader, the ctypes mirrors of the two
new structs, and the command line's refusals."""
import ctypes
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bdpt_amd
import display_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(os.path.dirname(bdpt_amd.LIB_PATH), "tinyrender_amd")
f32 = np.float32


def curve(encode, y):
    """The encode's curve in float64 (Python's own pow)."""
    y = float(y)
    if encode == "srgb":
        return 12.92 * y if y <= 0.0031308 else 1.055 * math.pow(y, 1.0 / 2.4) - 0.055
    if encode == "gamma22":
        return math.pow(y, 1.0 / 2.2)
    return y


# ---------------------------------------------------------------- thresholds
@pytest.mark.parametrize("encode", dc.ENCODES)
def test_thresholds_are_the_smallest_floats_that_reach_each_step(encode):
    T = dc.thresholds(encode)
    assert T.dtype == np.float32 and T.shape == (255,)
    assert (np.diff(T.astype(np.float64)) > 0).all() and T[0] > 0 and T[-1] < 1
    for k in range(1, 256):
        t, target = T[k - 1], (k - 0.5) / 255.0
        assert curve(encode, t) >= target > curve(encode, np.nextafter(t, f32(0))), (encode, k)


def test_thresholds_refuse_an_unknown_encode():
    with pytest.raises(bdpt_amd.BdptError, match="encode"):
        bdpt_amd.display_thresholds(7)


# ---------------------------------------------------------------- display_numpy
@pytest.mark.parametrize("encode", dc.ENCODES)
@pytest.mark.parametrize("tone", dc.TONES)
def test_display_numpy_is_monotone_in_the_input(tone, encode):
    """A ramp of 4096 values from 0 to 4 (and on to 1e6) in steps of 2^-10 and more: far more than the few ulps by
    which the rounded quotient of the tone curves can fail to be monotone between neighbouring floats, so the codes
    must never fall."""
    ramp = np.concatenate([np.arange(4096, dtype=f32) / f32(1024), np.array([8, 100, 65536, 1e6, np.inf], f32)])
    img = np.repeat(ramp[None, :, None], 3, axis=2)
    s = bdpt_amd.DisplaySettings(exposure=1.0, white=2.0, tone=tone, encode=encode)
    code = bdpt_amd.display_numpy(img, dc.thresholds(encode), s)[0, :, 0].astype(int)
    assert (np.diff(code) >= 0).all() and code[0] == 0 and code[-1] == 255


@pytest.mark.parametrize("tone", dc.TONES)
def test_display_numpy_sends_nonpositive_and_nan_to_zero(tone):
    img = np.array([[[0.0, -0.0, -1.0], [np.nan, -np.inf, -1e-30]]], f32)
    s = bdpt_amd.DisplaySettings(exposure=3.0, white=1.5, tone=tone)
    assert not bdpt_amd.display_numpy(img, dc.thresholds("srgb"), s).any()


@pytest.mark.parametrize("encode", dc.ENCODES)
@pytest.mark.parametrize("white", [1.0, 1.7, 4.0, 300.0])
def test_reinhard_reaches_255_at_and_above_white(white, encode):
    """At x = w the curve is ((w (1 + w / w^2)) / (1 + w) = 1 up to a few roundings, and the last threshold is
    below 0.999; beyond w it only rises."""
    w = f32(white)
    xs = np.array([w, np.nextafter(w, f32(np.inf)), w * f32(1.5), w * f32(64), 65536, np.inf], f32)
    img = np.repeat(xs[None, :, None], 3, axis=2)
    s = bdpt_amd.DisplaySettings(exposure=1.0, white=white, tone="reinhard", encode=encode)
    assert (bdpt_amd.display_numpy(img, dc.thresholds(encode), s) == 255).all()
    below = bdpt_amd.display_numpy(np.full((1, 1, 3), w * f32(0.5), f32), dc.thresholds(encode), s)
    assert (below < 255).all()


@pytest.mark.parametrize("encode", dc.ENCODES)
def test_all_256_codes_occur_on_the_edge_image(encode):
    """Under the clamp tone at exposure 1: T_k gives k, the float below it k - 1 (so the GPU test's demand for
    all 256 codes holds for the restatement alone)."""
    img = dc.edge_image(encode)
    s = bdpt_amd.DisplaySettings(exposure=1.0, tone="clamp", encode=encode, channels=4)
    out = bdpt_amd.display_numpy(img, dc.thresholds(encode), s)
    assert out.shape == (dc.EDGE_H, dc.EDGE_W, 4) and (out[..., 3] == 255).all()
    assert np.array_equal(np.unique(out[..., :3]), np.arange(256))
    T = dc.thresholds(encode)
    at = (np.arange(765) * 10) % img.size
    got = out[..., :3].reshape(-1)[at].reshape(255, 3).astype(int)
    k = np.arange(1, 256)
    assert np.array_equal(got, np.stack([k - 1, k, k], axis=1)) and np.array_equal(img.reshape(-1)[at][1::3], T)


# ---------------------------------------------------------------- meter_numpy
def python_meter(color, aov, s, norm=1.0):
    """The header's steps as a plain Python loop: (T, bin counts, b_key, b_white)."""
    counts = {}
    H, W = color.shape[:2]
    for i in range(H):
        for j in range(W):
            r, g, b = (f32(v) * f32(norm) for v in color[i, j])
            Y = f32(f32(f32(0.212671) * r) + f32(f32(0.715160) * g)) + f32(f32(0.072169) * b)
            u = struct.unpack("<I", struct.pack("<f", float(f32(Y))))[0] >> 19
            if not 16 <= u < 4080:
                continue
            if aov is not None and not f32(aov[i, j, 7]) * f32(norm) > 0:
                continue
            counts[u] = counts.get(u, 0) + 1
    T = sum(counts.values())
    found = []
    for pm in (s.key_permille, s.white_permille):
        rank, run = (T * pm + 999) // 1000, 0
        for u in sorted(counts):
            run += counts[u]
            if run >= rank:
                found.append(u)
                break
    return T, counts, found


def test_meter_numpy_counts_and_bins_equal_a_python_loop():
    H, W = 3, 5
    with np.errstate(all="ignore"):
        color = dc.frame(5, H, W)
        color[1, 2] = (1e-39, 1e-39, 1e-39)  # a denormal luminance: not counted
        color[2, 4] = (3e38, 3e38, 3e38)     # overflows to inf: not counted
        aov = dc.guides(6, H, W)
        for a in (None, aov):
            for s in (bdpt_amd.MeterSettings(), bdpt_amd.MeterSettings(key_permille=1, white_permille=1000)):
                T, counts, (bk, bw) = python_meter(color, a, s)
                words = bdpt_amd.meter_numpy(color, a, s)
                hist = bdpt_amd.meter_histogram_numpy(color, a)
                assert T > 3 and words[2] == T and int(hist.sum()) == T
                assert {int(u): int(hist[u]) for u in np.nonzero(hist)[0]} == counts
                assert words[3] == bk | bw << 16
                Yk = np.array([bk << 19 | 1 << 18], np.uint32).view(f32)[0]
                assert words[:1].view(f32)[0] == f32(s.key) / Yk


def test_meter_numpy_doubling_the_image_halves_the_exposure_exactly():
    color = dc.frame(7, 9, 11, specials=False)
    s = bdpt_amd.MeterSettings()
    a, b = bdpt_amd.meter_numpy(color, None, s), bdpt_amd.meter_numpy(color * f32(2), None, s)
    assert a[2] == b[2] > 0
    assert a[:1].view(f32)[0] == f32(2) * b[:1].view(f32)[0]
    assert (b[3] & 0xFFFF) - (a[3] & 0xFFFF) == 16 and (b[3] >> 16) - (a[3] >> 16) == 16  # one stop: 16 bins


def test_meter_numpy_returns_the_fallbacks_on_a_frame_of_zeros():
    s = bdpt_amd.MeterSettings(fallback_exposure=2.5, fallback_white=7.0)
    w = bdpt_amd.meter_numpy(np.zeros((4, 6, 3), f32), None, s)
    assert w[:2].view(f32).tolist() == [2.5, 7.0] and w[2] == 0 and w[3] == 0
    prev = np.array([1, 2], f32).view(np.uint32).tolist() + [5, 0]
    assert np.array_equal(bdpt_amd.meter_numpy(np.zeros((4, 6, 3), f32), None, s, prev=prev), w)


def test_meter_numpy_one_lit_pixel_is_its_own_key():
    color = np.zeros((4, 6, 3), f32)
    color[2, 3] = (0.5, 0.25, 0.125)
    w = bdpt_amd.meter_numpy(color, None, bdpt_amd.MeterSettings())
    Y = (f32(0.212671) * f32(0.5) + f32(0.715160) * f32(0.25)) + f32(0.072169) * f32(0.125)
    b = int(np.array([Y], f32).view(np.uint32)[0] >> 19)
    assert w[2] == 1 and w[3] == b | b << 16
    centre = np.array([b << 19 | 1 << 18], np.uint32).view(f32)[0]
    assert w[:1].view(f32)[0] == f32(0.18) / centre and abs(centre / Y - 1) <= 1 / 32  # the bin is 1/16 of a stop wide


def test_meter_numpy_rate_one_ignores_prev():
    color = dc.frame(8, 6, 7, specials=False)
    prev = np.array([123.0, 5.0], f32).view(np.uint32).tolist() + [9, 0]
    s1 = bdpt_amd.MeterSettings(rate=1.0)
    assert np.array_equal(bdpt_amd.meter_numpy(color, None, s1, prev=prev), bdpt_amd.meter_numpy(color, None, s1))
    s = bdpt_amd.MeterSettings(rate=0.25)
    e_m = bdpt_amd.meter_numpy(color, None, s)[:1].view(f32)[0]
    e = bdpt_amd.meter_numpy(color, None, s, prev=prev)[:1].view(f32)[0]
    assert e == f32(123.0) + (e_m - f32(123.0)) * f32(0.25)


# ---------------------------------------------------------------- PNG / PPM
def image(seed, H, W, ch):
    return np.random.default_rng(seed).integers(0, 256, (H, W, ch)).astype(np.uint8)


@pytest.mark.parametrize("H,W,ch", [(1, 1, 3), (1, 1, 4), (23, 37, 3), (23, 37, 4), (150, 147, 3)])
def test_png_round_trips_through_the_stdlib(H, W, ch):
    """(150 x 147 x 3: 66 300 raw bytes, past one stored block of 65 535.)"""
    px = image(H * W + ch, H, W, ch)
    data = bdpt_amd.encode_png(px, W, H, ch)
    chunks = dc.png_chunks(data)  # signature and every CRC
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2 if ch == 3 else 6, 0, 0, 0)
    z = chunks[1][1]
    raw = zlib.decompress(z)
    assert len(raw) == H * (1 + W * ch) and struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    # stored blocks only: 2 header bytes, 5 per block, 4 of Adler-32
    assert len(z) == 2 + 5 * -(-len(raw) // 65535) + len(raw) + 4
    assert np.array_equal(dc.decode_png(data), px)


def test_png_file_and_refusals(tmp_path):
    px = image(3, 5, 4, 3)
    bdpt_amd.save_png(px, 4, 5, str(tmp_path / "a.png"))
    assert (tmp_path / "a.png").read_bytes() == bdpt_amd.encode_png(px, 4, 5)
    with pytest.raises(bdpt_amd.BdptError, match="channels"):
        bdpt_amd.encode_png(np.zeros(8, np.uint8), 2, 2, 2)
    n = ctypes.c_int64(0)
    rc = bdpt_amd.lib().bdpt_encode_png(px.ctypes.data, 4, 5, 3, px.ctypes.data, 10, ctypes.byref(n))
    assert rc == bdpt_amd.ERR_INVALID and n.value == len(bdpt_amd.encode_png(px, 4, 5))
    with pytest.raises(bdpt_amd.BdptError) as e:
        bdpt_amd.save_png(px, 4, 5, str(tmp_path / "missing" / "a.png"))
    assert e.value.code == bdpt_amd.ERR_IO


def test_ppm_bytes_are_the_header_and_the_data(tmp_path):
    px = image(4, 23, 37, 3)
    bdpt_amd.save_ppm(px, 37, 23, str(tmp_path / "a.ppm"))
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n37 23\n255\n" + px.tobytes()


def test_a_saved_ppm_is_accepted_as_a_texture(tmp_path):
    px = image(5, 4, 4, 3)
    bdpt_amd.save_ppm(px, 4, 4, str(tmp_path / "shown.ppm"))
    (tmp_path / "quad.mtl").write_text("newmtl tex\nillum 7\nKd 0.5 0.5 0.5\nmap_Kd shown.ppm\n\n"
                                      "newmtl lamp\nillum 7\nKd 0 0 0\nKe 10 10 10\n")
    (tmp_path / "quad.obj").write_text(
        "mtllib quad.mtl\n"
        "v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\nv -0.2 2 -0.2\nv 0.2 2 -0.2\nv 0.2 2 0.2\nv -0.2 2 0.2\n"
        "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 1 0\nvn 0 -1 0\n"
        "o floor\nusemtl tex\nf 1/1/1 4/4/1 3/3/1 2/2/1\n"
        "o light\nusemtl lamp\nf 5//2 6//2 7//2 8//2\n")
    scene = bdpt_amd.Scene(str(tmp_path / "quad.obj"))
    info = scene.texture_info()
    assert scene.info()["triangles"] == 4 and len(scene.textures()) == 1, info


# ---------------------------------------------------------------- struct layout
STRUCTS = [("bdpt_meter_params", bdpt_amd._MeterParams), ("bdpt_display_params", bdpt_amd._DisplayParams)]


def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bdpt_amd.h"', "int main(void) {"]
    for cname, mirror in STRUCTS:
        lines.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'    printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o",
                        str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    layout = {}
    for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        cname, key, val = ln.split()
        layout[(cname, key)] = int(val)
    for cname, mirror in STRUCTS:
        assert ctypes.sizeof(mirror) == layout[(cname, "size")], cname
        for fname, _ in mirror._fields_:
            assert getattr(mirror, fname).offset == layout[(cname, fname)], (cname, fname)
    m = bdpt_amd.MeterSettings().c(2.0)
    assert (m.norm, m.key_permille, m.white_permille) == (2.0, 500, 990) and abs(m.key - 0.18) < 1e-7
    d = bdpt_amd.DisplaySettings(tone="filmic", encode="gamma22", channels=4).c()
    assert (d.tone, d.encode, d.channels) == (2, 1, 4)


# ---------------------------------------------------------------- command line
@pytest.mark.parametrize("args,words", [
    (["--display", "--tone", "aces"], ["--tone", "aces"]),
    (["--display", "--exposure", "0x"], ["--exposure", "0x"]),
    (["--display", "--exposure", "auto:0"], ["--exposure", "auto:0"]),
    (["--display", "--exposure", "auto:0.18:2"], ["--exposure", "auto:0.18:2"]),
    (["--display=gif"], ["--display=gif"]),
    (["--display", "--encode", "rec709"], ["--encode", "rec709"]),
    (["--tone", "filmic"], ["--tone", "--display"]),
    (["--exposure", "1.5"], ["--exposure", "--display"]),
    (["--display", "--sample-window", "0:1:0"], ["--display", "--sample-window"]),
])
def test_command_line_refuses_display_misuse_before_any_device(args, words, tmp_path):
    import variants

    toml = tmp_path / "scene.toml"
    toml.write_text(variants.toml_text("hardlight", 16, 16, 16))
    r = subprocess.run([CLI, str(toml)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert all(w in r.stderr for w in words), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["scene.toml"]
