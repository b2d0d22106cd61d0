"""What tests/test_temporal_cpu.py and tests/test_gpu_temporal.py share: a synthetic scene whose colour and
feature buffers are generated in numpy - a floor plane, a nearer slab that gives a depth step, and a miss
region above the horizon - with the geometry that says which pixels of a second camera lie in the band the
slab's move uncovers. A plain module: no test lives here, and nothing in it needs a GPU."""
import numpy as np

import bdpt_amd

f32 = np.float32

# camera A looks down at the slab; camera B is A panned and dollied
CAM_A = bdpt_amd.Camera(eye=(0.0, 2.2, 5.0), at=(0.0, 0.9, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
CAM_B = bdpt_amd.Camera(eye=(0.45, 2.2, 4.6), at=(0.12, 0.9, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
# the slab: the rectangle x in [-X, X], y in [0, Y] of the plane z = Z, facing +z; the floor is y = 0
SLAB_X, SLAB_Y, SLAB_Z = 0.7, 1.3, 2.0
FLOOR_ALBEDO, SLAB_ALBEDO = (0.6, 0.5, 0.4), (0.2, 0.7, 0.9)


def directions(consts, W, H):
    """The pixel centres' ray directions by the camera-ray formula, in float64 from the 72 constants: (H, W, 3)
    unit vectors (not the device's bits: CPU tests may pass any unit vectors)."""
    k = np.asarray(consts, np.float64)
    c2w = k[16:32].reshape(4, 4).T  # (column-major)
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    x = ((j + 0.5) / W) * 2 - 1
    y = (1 - (i + 0.5) / H) * 2 - 1
    cam = np.stack([x * k[66] * k[67], y * k[66], -np.ones_like(x)], -1)
    d = cam @ c2w[:3, :3].T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def cast(eye, d):
    """Closest hit of the rays eye + t d with the slab and the floor, t in [1, 1000]: (t, surface) with surface
    0 = miss, 1 = floor, 2 = slab."""
    eye = np.asarray(eye, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = np.where(d[..., 1] < 0, -eye[1] / d[..., 1], np.inf)
        ts = np.where(d[..., 2] < 0, (SLAB_Z - eye[2]) / d[..., 2], np.inf)
    ps = eye + np.where(np.isfinite(ts), ts, 0.0)[..., None] * d
    on = np.isfinite(ts) & (np.abs(ps[..., 0]) <= SLAB_X) & (ps[..., 1] >= 0) & (ps[..., 1] <= SLAB_Y)
    ts = np.where(on, ts, np.inf)
    t = np.minimum(tf, ts)
    hit = (t >= 1) & (t <= 1000)
    return np.where(hit, t, 0.0), np.where(hit, np.where(ts < tf, 2, 1), 0)


def buffers(cam, W, H):
    """(aov (H, W, 8) float32 as a full frame's bdpt_render_aov would hold it - coverage 1 on a hit -, dirs
    (H, W, 3) float32, surface (H, W), consts (72,)) of the synthetic scene seen from `cam`."""
    consts = bdpt_amd.camera_constants(cam, W, H)
    d = directions(consts, W, H)
    t, surf = cast(cam.eye, d)
    aov = np.zeros((H, W, 8), f32)
    for s, alb, n in ((1, FLOOR_ALBEDO, (0, 1, 0)), (2, SLAB_ALBEDO, (0, 0, 1))):
        aov[surf == s, 0:3] = alb
        aov[surf == s, 3:6] = n
    aov[..., 6] = t
    aov[..., 7] = surf > 0
    return aov, d.astype(f32), surf, consts


def colours(seed, W, H, n=1):
    """n random colour frames in [0, 2): (n, H, W, 3) float32."""
    return np.random.default_rng(seed).random((n, H, W, 3), dtype=np.float32) * f32(2)


def floor_classes(W, H, margin_px=2.0, max_depth=6.0):
    """Of camera B's floor pixels, by the geometry alone (float64): `hidden`, whose world point camera A saw
    only through the slab, by a margin of margin_px of A's pixels on every side (so every tap of its place in
    A's frame is a slab pixel), and `open`, which A saw at a place margin_px inside its image and away from the
    slab's outline by the same margin, no farther than max_depth from B (farther out the floor is seen at so
    grazing an angle that neighbouring pixels' depths differ by more than the default sigma_depth, and a history
    tap half a pixel away is rightly refused). (H, W) bool each."""
    _, dB, surfB, _ = buffers(CAM_B, W, H)
    tB, _ = cast(CAM_B.eye, dB.astype(np.float64))
    X = np.asarray(CAM_B.eye, np.float64) + tB[..., None] * dB.astype(np.float64)
    eA = np.asarray(CAM_A.eye, np.float64)
    kA = np.asarray(bdpt_amd.camera_constants(CAM_A, W, H), np.float64)
    w2c = kA[0:16].reshape(4, 4).T
    Xc = X @ w2c[:3, :3].T + w2c[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = Xc[..., 0] / (-Xc[..., 2] * kA[66] * kA[67])
        v = Xc[..., 1] / (-Xc[..., 2] * kA[66])
        s = (SLAB_Z - eA[2]) / (X[..., 2] - eA[2])  # where eye_A -> X crosses the slab's plane
    fx, fy = (u + 1) * 0.5 * W - 0.5, (1 - v) * 0.5 * H - 0.5
    P = eA + s[..., None] * (X - eA)
    crosses = (s > 0) & (s < 1)
    # margin_px of A's pixels at the slab, in world units
    m = margin_px * 2 * kA[66] / H * np.linalg.norm(np.asarray([0, SLAB_Y / 2, SLAB_Z]) - eA)
    inside = crosses & (np.abs(P[..., 0]) <= SLAB_X - m) & (P[..., 1] >= m) & (P[..., 1] <= SLAB_Y - m)
    outside = ~crosses | (np.abs(P[..., 0]) >= SLAB_X + m) | (P[..., 1] >= SLAB_Y + m)
    floorB = surfB == 1
    in_image = (fx >= margin_px) & (fx <= W - 1 - margin_px) & (fy >= margin_px) & (fy <= H - 1 - margin_px)
    return floorB & inside, floorB & outside & in_image & (-Xc[..., 2] >= 1) & (tB <= max_depth)
