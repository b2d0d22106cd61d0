"""What tests/test_display_cpu.py and tests/test_gpu_display.py share: the synthetic inputs of the display
output (bdpt_meter, bdpt_display) and their expected results from the numpy restatements, each computed once.
A plain module: no test lives here, and nothing in it needs a GPU (the threshold tables come from the library's
host-only bdpt_display_thresholds)."""
import functools

import numpy as np

import bdpt_amd
import sweep_cases as sw

f32 = np.float32
EDGE_H, EDGE_W = 23, 37  # 2553 floats: room for the 765 edge values, no multiple of the block or of 4 pixels
TONES, ENCODES = ("clamp", "reinhard", "filmic"), ("srgb", "gamma22", "linear")


@functools.lru_cache(maxsize=None)
def thresholds(encode):
    t = bdpt_amd.display_thresholds(encode)
    t.setflags(write=False)
    return t


def sprinkle_specials(a):
    """NaN, +inf, -inf, a negative and -0 over a's floats, in place, at the co-prime periods 17, 19, 29, 31 and
    41 (sweep_cases.sprinkle holds 7, 11 and 13)."""
    flat = a.reshape(-1)
    flat[3::17] = np.nan
    flat[5::19] = np.inf
    flat[6::29] = -np.inf
    flat[8::31] = f32(-0.5)
    flat[9::41] = f32(-0.0)
    return a


@functools.lru_cache(maxsize=None)
def edge_image(encode):
    """37 x 23 x 3: for every k the threshold T_k itself and its float32 neighbours on both sides (765 values, at
    every tenth float: 10 is co-prime to 2553, so no two share a place), the rest sweep_cases.planes (values in
    [0, 2) with 0, 1e-20 and 1e6) with the specials sprinkled in. Shown with the clamp tone at exposure 1 an edge
    value reaches the search as it is."""
    img = sprinkle_specials(sw.planes(41 + ENCODES.index(encode), EDGE_H, EDGE_W, 3))
    T = thresholds(encode)
    edges = np.stack([np.nextafter(T, f32(0)), T, np.nextafter(T, f32(2))], axis=1).reshape(-1).astype(f32)
    assert edges.size == 765
    img.reshape(-1)[(np.arange(765) * 10) % img.size] = edges
    img.setflags(write=False)
    return img


def frame(seed, H, W, specials=True):
    """A float32 colour frame (H, W, 3) in [0, 2) with sweep_cases' extremes, optionally the specials too."""
    img = sw.planes(seed, H, W, 3)
    return sprinkle_specials(img) if specials else img


def guides(seed, H, W):
    """Feature buffers (H, W, 8) of which the meter reads the coverage alone: about a third of the pixels
    uncovered (0), a few with a negative or NaN coverage, the rest 1."""
    rng = np.random.default_rng(seed)
    aov = np.zeros((H, W, 8), f32)
    cov = (rng.random((H, W)) > 0.3).astype(f32)
    flat = cov.reshape(-1)
    flat[4::53] = f32(-1.0)
    flat[7::59] = np.nan
    aov[..., 7] = cov
    return aov


def constant_frame(H, W, value=0.25):
    """Every pixel the same grey: every lane of every wave counts into one bin."""
    return np.full((H, W, 3), value, f32)


def png_chunks(data):
    """[(type, payload)] of a PNG's chunks, after checking the signature and every chunk's CRC-32 with zlib."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(kind + body) == crc, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    return chunks


def decode_png(data):
    """The pixels of an 8-bit RGB / RGBA PNG whose scanlines all have filter type 0: uint8 (H, W, channels).
    Inflated with the stdlib's zlib, which also checks the stream's Adler-32."""
    import struct
    import zlib
    chunks = png_chunks(data)
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (2, 6)
    ch = 3 if colour == 2 else 4
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * ch)
    assert not rows[:, 0].any()  # filter type 0 on every scanline
    return rows[:, 1:].reshape(H, W, ch).copy()
