"""What tests/test_gpu_sweeps.py and tests/test_sweeps_cpu.py share: the launch arithmetic of the grid-stride
post-process kernels (aov_kernels.hip, adaptive_kernels.hip), the shapes that reach past one sweep of their
capped grid and past one block count per scan lane, and the synthetic inputs at those shapes. A plain module:
no test lives here, and nothing in it needs a GPU or the library."""
import numpy as np

f32 = np.float32

# The launchers cap the grid at 4096 blocks of 256 lanes (tests/test_sweeps_cpu.py reads the figures from the
# sources): one sweep covers SWEEP work units, and only the loop's `+= gridDim.x * 256` reaches a later one.
GRID_CAP, BLOCK = 4096, 256
SWEEP = GRID_CAP * BLOCK

# adaptive_select: a block owns kSelBlock * kSelRounds pixels, and the one scan block gives each of its
# kSelBlock lanes `per` consecutive block counts.
SEL_BLOCK, SEL_ROUNDS = 256, 4
SEL_ITEMS = SEL_BLOCK * SEL_ROUNDS

# (H, W). UNIT1: 350 463 pixels, 1 051 389 floats, an odd count just beyond one sweep of floats.
# UNIT4: 4 205 568 floats, so more than one sweep of 4-float units.
UNIT1, UNIT4 = (591, 593), (1184, 1184)
# relight / combine_group_planes own pixels, or 4 pixels when vectorised: an odd pixel count beyond one sweep of
# pixels, and a pixel count that is a multiple of 4 beyond one sweep of 4-pixel units.
PIXEL1, PIXEL4 = (1025, 1025), (2052, 2048)
# adaptive_select: 257 blocks (per 2, the last working lane owns one block); 343 blocks (a partial lane, the
# flag bytes no multiple of 16); 1369 blocks (per 6).
SELECT_SHAPES = [(513, 512), UNIT1, UNIT4]
SELECT_DENSITIES = ["random", "all", "none", "last_pixel", "one_per_block", "odd_blocks"]


def select_layout(n_pixels):
    """(blocks, per, working lanes, blocks of the last working lane) of adaptive_select_scan_kernel."""
    nblocks = -(-n_pixels // SEL_ITEMS)
    per = -(-nblocks // SEL_BLOCK)
    lanes = -(-nblocks // per)
    return nblocks, per, lanes, nblocks - (lanes - 1) * per


def sprinkle(a):
    """synthetic_pairs' extremes (tests/test_gpu_adaptive.py) over a's floats, in place: zeros, 1e-20 (whose
    square is a float32 denormal) and 1e6, at periods 7, 11 and 13, so at no period of a block or a sweep."""
    flat = a.reshape(-1)
    flat[0::7] = 0.0
    flat[1::11] = f32(1e-20)
    flat[2::13] = f32(1e6)
    return a


def planes(seed, *shape):
    """float32 planes of `shape` in [0, 2) with the extremes sprinkled in."""
    rng = np.random.default_rng(seed)
    return sprinkle(rng.random(shape, dtype=np.float32) * f32(2))


def sample_counts(seed, H, W):
    """adaptive_resolve's m: random in [0, 6], the first pixel 0 (nothing traced) and the last one 6."""
    m = np.random.default_rng(seed).integers(0, 7, (H, W)).astype(np.int32)
    m[0, 0], m[H - 1, W - 1] = 0, 6
    return m


SELECT_EPS, SELECT_STEP, SELECT_MAX = 1e-3, 1, 4


def select_case(density, H, W, dilate):
    """(S, var, m, threshold) of one adaptive_select case, to run with SELECT_EPS, SELECT_STEP, SELECT_MAX.

    "random": S and var random with the extremes, m in [0, 4] (so some pixels are at their budget), the threshold
    at the quantile of the pixels' own metric that leaves about half of them active: the median, or with dilate
    the 0.93 quantile, since 1 - 0.93^9 is 0.48. The other densities name the active set A exactly, whatever
    dilate is: var is positive on A alone and the threshold 0, so noisy(p) is "p in A", and m is at the budget
    outside A, so what the dilation adds is refused again."""
    N = H * W
    rng = np.random.default_rng(1000 + N + 7 * SELECT_DENSITIES.index(density) + int(dilate))
    S = rng.random((H, W, 3), dtype=np.float32)
    var = rng.random((H, W, 3), dtype=np.float32) * f32(0.5)
    if density == "random":
        sprinkle(S), sprinkle(var.reshape(-1)[5:])  # (a view: other floats than S's)
        m = rng.integers(0, SELECT_MAX + 1, (H, W)).astype(np.int32)
        s = S.astype(np.float64).sum(-1) + SELECT_EPS
        metric = var.astype(np.float64).sum(-1) / (s * s)
        return S, var, m, float(np.sqrt(np.quantile(metric, 0.93 if dilate else 0.5)))
    p = np.arange(N)
    A = {"all": np.ones(N, bool), "none": np.zeros(N, bool), "last_pixel": p == N - 1,
         "one_per_block": p % SEL_ITEMS == SEL_ITEMS - 1, "odd_blocks": (p // SEL_ITEMS) % 2 == 1}[density].reshape(H, W)
    var = np.where(A[..., None], var + f32(0.125), f32(0)).astype(np.float32)
    m = np.where(A, rng.integers(0, SELECT_MAX, (H, W)), SELECT_MAX).astype(np.int32)
    return S, var, m, 0.0
