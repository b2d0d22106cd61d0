"""The grid-stride post-process kernels (aov_kernels.hip, adaptive_kernels.hip) at the sizes of real frames:
past one sweep of their capped grid (4096 blocks of 256 lanes), with more than one block count per lane of the
select's scan block and a partial last lane, and with the feature-buffer kernel striding over its tiles. Every
other test hands these kernels less than one sweep, so only here does the loop's `+= gridDim.x * 256` run.

Inputs are synthetic (tests/sweep_cases.py); every comparison is np.array_equal on the float bits against the
project's numpy restatement of the same operation, which is these kernels' contract. Each test asserts that its
shape is beyond what it claims to reach, so a later change of shape cannot fall back under one sweep unseen."""
import numpy as np
import pytest

import bdpt_amd
import variants
from bdpt_amd import SampleWindow
from conftest import gpu_available
from sweep_cases import (BLOCK, PIXEL1, PIXEL4, SEL_BLOCK, SEL_ITEMS, SELECT_DENSITIES, SELECT_EPS, SELECT_MAX,
                         SELECT_SHAPES, SELECT_STEP, SWEEP, UNIT1, UNIT4, planes, sample_counts, select_case,
                         select_layout)
from test_gpu_parity import TOL, integrator, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

assert SWEEP == 4096 * 256
f32 = np.float32
HL_RR = variants.SCENES["hardlight"]["rr_depth"]
SIGMAS = dict(sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.1)  # tests/test_gpu_denoise.py's

_small = []


def small():
    """The host-array entry points take H and W from the array: any context serves."""
    if not _small:
        _small.append(integrator("hardlight", 8, 8, 8, HL_RR))
    return _small[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cdiv(a, b):
    return -(-a // b)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def beyond_one_sweep(S, v, rs, rv, unit):
    """The part of the outputs that only a second sweep writes is there, and it is not all zero."""
    tail = slice(SWEEP * unit, None)
    for got, ref in ((S, rs), (v, rv)):
        assert got.reshape(-1)[tail].size > 0 and got.reshape(-1)[tail].any()
        assert np.array_equal(bits(got).reshape(-1)[tail], bits(ref).reshape(-1)[tail])


# ------------------------------------------------ 1, 2. one float or four floats a lane
@pytest.mark.parametrize("K,shape", [(2, UNIT1), (3, UNIT1), (2, UNIT4)], ids=["unit1-K2", "unit1-K3", "unit4-K2"])
def test_gpu_batch_moments_past_one_sweep(K, shape):
    H, W = shape
    n = H * W * 3
    unit = 4 if shape == UNIT4 else 1
    assert (n % 4 == 0) == (unit == 4) and n // unit > SWEEP  # batch_moments_kernel<unit>: a second sweep
    assert unit == 4 or n % 2 == 1
    pl = planes(10 * K + unit, K, H, W, 3)
    S, v = small().batch_moments(pl)
    rs, rv = bdpt_amd.batch_moments_numpy(pl)
    assert same_bits(S, rs) and same_bits(v, rv)
    beyond_one_sweep(S, v, rs, rv, unit)


@pytest.mark.parametrize("shape", [UNIT1, UNIT4], ids=["unit1", "unit4"])
def test_gpu_adaptive_resolve_past_one_sweep(shape):
    H, W = shape
    K, n = 2, H * W * 3
    unit = 4 if shape == UNIT4 else 1
    assert (n % 4 == 0) == (unit == 4) and n // unit > SWEEP  # adaptive_resolve_kernel<unit>: a second sweep
    pl = planes(20 + unit, K, 2, H, W, 3)
    m = sample_counts(30 + unit, H, W)
    assert m[0, 0] == 0 and m[-1, -1] == 6 and m.min() == 0 and m.max() == 6
    S, v = small().adaptive_resolve(pl, m, 6 * K)
    rs, rv = bdpt_amd.adaptive_resolve_numpy(pl, m, 6 * K)
    assert same_bits(S, rs) and same_bits(v, rv)
    assert np.isfinite(S).all() and S[-1, -1].any()
    beyond_one_sweep(S, v, rs, rv, unit)


def test_gpu_compose_layers_past_one_sweep():
    H, W = UNIT1
    n = H * W * 3
    assert n > SWEEP and n % 4 != 0  # layers_compose_kernel: a second sweep of floats
    layers = planes(41, 3, H, W, 3)
    got = small().compose_layers(layers, (0, 2))
    want = layers[0] + layers[2]  # float32, ascending
    assert want.dtype == np.float32 and same_bits(got, want)
    assert not same_bits(got, layers[0] + layers[1])
    assert got.reshape(-1)[SWEEP:].any()


def test_gpu_shared_guide_is_the_plane_sum_past_one_sweep():
    """planes_sum_kernel forms the guide of bdpt_denoise_planes' shared mode: the filtered guide has the bits of
    bdpt_denoise of the planes' float32 sum (tests/test_gpu_denoise_planes.py states it at 40 x 28)."""
    H, W = UNIT1
    n = H * W * 3
    assert n > SWEEP and n % 4 != 0  # planes_sum_kernel: a second sweep of floats
    it = integrator("hardlight", W, H, 4, HL_RR)
    pl = planes(42, 2, H, W, 3)
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3], aov[..., 5], aov[..., 6], aov[..., 7] = 0.5, 1.0, 2.0, 1.0
    aov[:, 300] = 0.0  # a column of miss pixels
    kw = dict(iterations=1, demodulate=True, **SIGMAS)
    out, og = it.denoise_planes(pl, aov, "shared", return_guide=True, **kw)
    G = pl[0] + pl[1]
    assert same_bits(og, it.denoise(G, aov, **kw))
    assert np.isfinite(out).all() and og.reshape(-1)[SWEEP:].any()
    assert not same_bits(og, it.denoise(pl[0], aov, **kw))


# ------------------------------------------------------ 3. one pixel or four pixels a lane
def relight_loop(groups, gains):
    """relight's docstring: gains[g] * groups[g] summed in ascending group order, each product and sum float32."""
    acc = gains[0][None, None, :] * groups[0]
    for g in range(1, groups.shape[0]):
        acc = acc + gains[g][None, None, :] * groups[g]
    assert acc.dtype == np.float32
    return acc


@pytest.mark.parametrize("shape", [PIXEL1, PIXEL4], ids=["unit1", "unit4"])
def test_gpu_relight_and_combine_past_one_sweep(shape):
    H, W = shape
    px = H * W
    if shape == PIXEL1:  # relight_kernel<1>, group_planes_combine_kernel<1>: a second sweep of pixels
        assert px % 2 == 1 and (px * 3) % 12 != 0 and px > SWEEP
    else:  # <4>: a second sweep of 4-pixel units
        assert (px * 3) % 12 == 0 and px // 4 > SWEEP
    first = SWEEP * 3 * (1 if shape == PIXEL1 else 4)  # floats of one sweep
    pl = planes(50 + H, 2, 2, H, W, 3)  # (n_groups, n_inner, H, W, 3)
    gains = f32([[1.5, 0.0, 0.75], [0.3, -2.0, 1.1]])  # one gain 0, one negative
    weights = f32([0.7, 1.9])
    it = small()
    got = it.combine_group_planes(pl, gains, weights)
    assert same_bits(got, bdpt_amd.combine_group_planes_numpy(pl, gains, weights))
    assert got.reshape(-1)[first:].any()
    groups = np.ascontiguousarray(pl[:, 1])
    got = it.relight(groups, gains)
    assert same_bits(got, relight_loop(groups, gains))
    assert got.reshape(-1)[first:].any() and (got[..., 1] <= 0).all() and (got[..., 1] < 0).any()


# ------------------------------------------------------------------- 4. the contact sheet
@pytest.mark.parametrize("with_gains", [False, True], ids=["copied", "gains"])
def test_gpu_strategies_sheet_past_one_sweep(with_gains):
    n_s, n_t, H, W = 2, 2, 300, 300
    total = n_s * n_t * H * W * 3
    assert total > SWEEP  # strategies_sheet_kernel: a second sweep of the sheet's floats
    pl = planes(60, n_s, n_t, H, W, 3)
    gains = f32([[[2.0, 0.5, 1.25], [0.0, 0.0, 0.0]], [[0.3, 0.7, 1.1], [4.0, 0.125, 3.0]]]) if with_gains else None
    got = small().strategies_sheet(pl, gains)
    assert got.shape == (n_t * H, n_s * W, 3)
    assert same_bits(got, bdpt_amd.strategies_sheet_numpy(pl, gains))
    assert got.reshape(-1)[SWEEP:].any()
    assert np.array_equal(got[H:, W:], pl[1, 1] * (gains[1, 1] if with_gains else f32(1)))  # (s, t) = (1, 2): the last tile


# --------------------------------------------------------------------------- 5. select
@pytest.mark.parametrize("dilate", [False, True], ids=["plain", "dilate"])
@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=["513x512", "591x593", "1184x1184"])
def test_gpu_select_with_several_blocks_per_scan_lane(shape, dilate):
    H, W = shape
    N = H * W
    nblocks, per, lanes, last = select_layout(N)
    # adaptive_select_scan_kernel: per >= 2 block counts a lane, and a last working lane that owns fewer
    assert nblocks > SEL_BLOCK and per >= 2 and nblocks % per != 0 and 1 <= last < per and lanes <= SEL_BLOCK
    assert (nblocks, per) == {513: (257, 2), 591: (343, 2), 1184: (1369, 6)}[H]
    if shape == UNIT1:
        assert N % 16 != 0  # the block counts do not start where the flag bytes end
    it = small()
    seen = {}
    for density in SELECT_DENSITIES:
        S, var, m, thr = select_case(density, H, W, dilate)
        lst, m2 = it.adaptive_select(S, var, m, thr, SELECT_EPS, SELECT_STEP, SELECT_MAX, dilate)
        count = lst.size  # (the wrapper cuts the list at the count the library reports)
        rl, rm = bdpt_amd.adaptive_select_numpy(S, var, m, thr, SELECT_EPS, SELECT_STEP, SELECT_MAX, dilate)
        assert lst.dtype == np.int32 and count == rl.size, (density, count, rl.size)
        assert np.array_equal(lst, rl), (density, np.flatnonzero(lst != rl)[:4])
        assert np.all(np.diff(lst) > 0), density
        assert np.array_equal(m2, rm), density
        seen[density] = count
    print(f"{H} x {W}: {nblocks} blocks, {per} a lane, active {seen}")
    assert 0.3 * N < seen["random"] < 0.7 * N
    assert seen["all"] == N and seen["none"] == 0 and seen["last_pixel"] == 1
    assert seen["one_per_block"] == N // SEL_ITEMS  # (the last block is partial: it has no pixel 1023)
    assert seen["odd_blocks"] == sum(min(SEL_ITEMS, N - b * SEL_ITEMS) for b in range(1, nblocks, 2))


# ------------------------------------------------- 6. the driver's start and sample map
def test_gpu_adaptive_driver_past_one_sweep():
    """adaptive_start_kernel and adaptive_samples_kernel run only inside render_adaptive: one pass of two
    batches, one sample each, over more pixels than one sweep. The frame is the resolve of the two full-list
    windows (the suite's tolerance: the splats' atomic additions come in another order in another render)."""
    H, W = PIXEL1
    N, K = H * W, 2
    assert N > SWEEP and N % 2 == 1  # a second sweep of pixels in both kernels
    it = integrator("cbox_low", W, H, K, 5)
    frame, var, samples = it.render_adaptive(1e6, n_batches=K, step=1, max_passes=1)
    assert it.adaptive == dict(passes=1, samples=N * K, active=[N])
    assert samples.shape == (H, W) and np.all(samples == K)
    assert np.isfinite(frame).all() and np.isfinite(var).all() and frame.reshape(-1)[3 * SWEEP:].any()
    full = np.arange(N, dtype=np.int32)
    ref_it = integrator("cbox_low", W, H, K, 5)
    pl = np.stack([ref_it.render_pixels(full, w) for w in bdpt_amd.adaptive_windows(K, 1, 0)])
    assert [(w.first, w.stride, w.count) for w in bdpt_amd.adaptive_windows(K, 1, 0)] == [(0, 2, 1), (1, 2, 1)]
    ref, _ = bdpt_amd.adaptive_resolve_numpy(pl, np.ones((H, W), np.int32), K)
    worst = rel_l2(frame, ref).max()
    print("one pass of", N, "pixels against the resolve of its windows: max per-pixel rel L2", worst)
    assert worst <= TOL, f"max per-pixel rel L2 {worst:.3g}"


# ------------------------------------------------------------- 7. the feature buffers' tile stride
def test_gpu_aov_strides_over_its_tiles():
    """aov_kernel runs at most slots / 64 blocks of one 8 x 8 tile each and strides over the tiles beyond. On
    the MI355X (256 CUs) this context reports a grid of 1024 blocks and 262 144 slots, so at most 4096 blocks:
    the frame chosen from those figures is 725 x 723, 8281 tiles, and its shards take every third row (2821
    tiles each). A lane's pixel depends on nothing but its own ray, so the frame must equal, bit for bit, the
    one assembled from interleaved row shards that each fit one sweep of tiles: the path
    tests/test_gpu_aov.py pins to bdpt_intersect."""
    cam = variants.SCENES["cbox_low"]["camera"]
    probe = integrator("cbox_low", 8, 8, 2, 5)
    st = probe.stats()
    grid, slots = st["grid"], st["slots"]
    max_grid = slots // 64
    assert grid >= 1 and slots == grid * BLOCK and max_grid >= 1
    t = int(np.ceil(np.sqrt(2 * max_grid + 1)))
    W, H = 8 * t - 3, 8 * t - 5  # neither a multiple of 8
    ntiles = t * t
    assert W % 8 and H % 8 and cdiv(W, 8) * cdiv(H, 8) == ntiles and ntiles > 2 * max_grid  # the tile stride, twice
    print(f"grid {grid}, slots {slots}, at most {max_grid} blocks; frame {W} x {H}: {ntiles} tiles")
    full = integrator("cbox_low", W, H, 2, 5)
    assert full.stats()["slots"] == slots  # (the slots do not depend on the frame size)
    whole = full.render_aov().copy()
    assert full.stats()["samples"] == W * H * 2
    shard_tiles = lambda nrows: t * cdiv(nrows, 8)  # t tile columns
    stride = next(s for s in range(2, H) if shard_tiles(cdiv(H, s)) <= max_grid)
    shards = integrator("cbox_low", W, H, 2, 5)
    for r in range(stride):
        assert shard_tiles(len(range(r, H, stride))) <= max_grid  # this shard's tiles fit one sweep
        shards.render_aov(row_offset=r, row_stride=stride)
    assert np.isfinite(whole).all() and (whole[..., 7] > 0).mean() > 0.5
    assert whole[-1, -1].any() and whole[0, 0].any()
    assert same_bits(whole, shards.aov), np.argwhere(bits(whole) != bits(shards.aov))[:4]


# ---------------------------------------------- outputs a float off the 16-byte boundary
def offset_outputs(n, which):
    """(sum, var) device tensors of n floats inside larger ones, each at a 16-byte boundary or one float past
    it, between sentinels."""
    import torch

    out = []
    for off in which:
        buf = torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out.append((buf, 4 + off))
    return out


def view(buf_at, n):
    buf, at = buf_at
    host = buf.cpu().numpy()
    assert np.all(host[:at] == -7.0) and np.all(host[at + n:] == -7.0), "written outside the output"
    return host[at:at + n]


@pytest.mark.parametrize("offsets", [(1, 0), (0, 1), (1, 1)], ids=["sum", "var", "both"])
def test_gpu_moments_and_resolve_with_outputs_off_the_vector_boundary(offsets):
    """n % 4 == 0, but an output starts one float past a 16-byte boundary: the launchers must take the dword
    kernels, whose results have the bits of the 16-byte kernels' (and of the numpy loop)."""
    import torch

    H, W, K = 8, 12, 3  # test_gpu_adaptive's "unit4" shape
    n = H * W * 3
    assert n % 4 == 0
    it = integrator("hardlight", W, H, 6 * K, HL_RR)
    dev = torch.device("cuda", 0)
    pl = planes(70, K, 2, H, W, 3)
    m = sample_counts(71, H, W)
    t_pl, t_m = torch.from_numpy(pl).to(dev), torch.from_numpy(m).to(dev)
    assert t_pl.data_ptr() % 16 == 0
    results = []
    for which in ((0, 0), offsets):
        (s_m, v_m), (s_r, v_r) = offset_outputs(n, which), offset_outputs(n, which)
        assert [(b.data_ptr() + 4 * at) % 16 for b, at in (s_m, v_m)] == [4 * o for o in which]
        torch.cuda.synchronize()
        # the moments of the K * 2 planes taken as 2 K batches, then the resolve of the K pairs
        it.batch_moments_device(t_pl.data_ptr(), 2 * K, W, H, s_m[0].data_ptr() + 4 * s_m[1], v_m[0].data_ptr() + 4 * v_m[1])
        it.adaptive_resolve_device(t_pl.data_ptr(), t_m.data_ptr(), K, int(m.sum()), s_r[0].data_ptr() + 4 * s_r[1],
                                   v_r[0].data_ptr() + 4 * v_r[1])
        it.synchronize()
        results.append([view(x, n) for x in (s_m, v_m, s_r, v_r)])
    for aligned, shifted in zip(*results):
        assert np.array_equal(aligned.view(np.uint32), shifted.view(np.uint32))
    rs, rv = bdpt_amd.batch_moments_numpy(pl.reshape(2 * K, H, W, 3))
    qs, qv = bdpt_amd.adaptive_resolve_numpy(pl, m, 6 * K)
    for got, ref in zip(results[1], (rs, rv, qs, qv)):
        assert np.array_equal(got.view(np.uint32), bits(ref).reshape(-1))
