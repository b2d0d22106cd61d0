"""What tests/test_gpu_sweeps.py rests on, checked without a GPU: the launch figures its shapes are worked out
from still stand in the kernels' sources, the shapes reach what they claim, and the numpy restatements it
compares against run at those shapes and agree with independent forms of themselves."""
import os
import re
import time

import numpy as np

import bdpt_amd
from conftest import REPO
from sweep_cases import (BLOCK, GRID_CAP, PIXEL1, PIXEL4, SEL_BLOCK, SEL_ITEMS, SEL_ROUNDS, SELECT_DENSITIES, SELECT_EPS,
                         SELECT_MAX, SELECT_SHAPES, SELECT_STEP, SWEEP, UNIT1, UNIT4, planes, sample_counts, select_case,
                         select_layout)

CSRC = os.path.join(REPO, "bidirectional-path-tracing_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_launch_caps_and_select_constants_are_what_the_sweep_tests_assume():
    assert (GRID_CAP, BLOCK, SWEEP) == (4096, 256, 4096 * 256) and (SEL_BLOCK, SEL_ROUNDS, SEL_ITEMS) == (256, 4, 1024)
    cap = re.compile(r"std::min<size_t>\(\((\w+) \+ 255\) / 256, 4096\)")
    aov, ad = source("aov_kernels.hip"), source("adaptive_kernels.hip")
    # every capped launcher: ceil(units / 256) blocks, at most 4096, and no other cap anywhere in the two files
    assert sorted(cap.findall(aov)) == ["n", "n", "total", "units", "units", "units"]
    assert cap.findall(ad) == ["items"]
    for text in (aov, ad):
        assert len(cap.findall(text)) == text.count("std::min<size_t>")
    launcher = {"strategies_sheet": "total", "relight": "units", "group_planes_combine": "units", "layers_compose": "n",
                "batch_moments": "units", "planes_sum": "n"}
    for name, units in launcher.items():
        body = aov[aov.index(f"hipError_t launch_{name}("):]
        body = body[:body.index("\n}\n")]
        assert f"std::min<size_t>(({units} + 255) / 256, 4096)" in body and "dim3(blocks), dim3(256)" in body, name
    assert re.search(r"static unsigned stride_blocks\(size_t items\) \{ return static_cast<unsigned>\(std::min<size_t>", ad)
    for name in ("adaptive_resolve", "adaptive_start", "adaptive_samples"):
        body = ad[ad.index(f"hipError_t launch_{name}("):]
        body = body[:body.index("\n}\n")]
        assert "stride_blocks(" in body and "dim3(256)" in body, name
    # the kernels step by the whole grid of 256-lane blocks
    step = "static_cast<size_t>(gridDim.x) * 256"
    assert aov.count(step) == 5 and aov.count("i += gridDim.x * 256u") == 1 and ad.count(step) == 3
    assert re.search(r"constexpr int kSelBlock = 256, kSelRounds = 4, kSelItems = kSelBlock \* kSelRounds,", ad)
    assert "const uint32_t per = (nblocks + kSelBlock - 1) / kSelBlock;" in ad
    assert "dim3(1), dim3(dev::kSelBlock), 0, st, block_count, nblocks, count" in ad  # one scan block
    assert "constexpr int kAovTile = 8;" in aov and "const int64_t max_grid = nslots / dev::kAovBlock;" in aov


def test_shapes_reach_what_they_claim():
    for (H, W), unit in ((UNIT1, 1), (UNIT4, 4)):
        n = H * W * 3
        assert (n % 4 == 0) == (unit == 4) and SWEEP < n // unit < 2 * SWEEP  # the smallest: a second sweep, no third
    assert UNIT1[0] * UNIT1[1] * 3 == 1051389 and UNIT4[0] * UNIT4[1] * 3 == 4205568
    px1, px4 = PIXEL1[0] * PIXEL1[1], PIXEL4[0] * PIXEL4[1]
    assert px1 % 2 == 1 and SWEEP < px1 < 2 * SWEEP and (3 * px4) % 12 == 0 and SWEEP < px4 // 4 < 2 * SWEEP
    assert [select_layout(H * W) for H, W in SELECT_SHAPES] == [(257, 2, 129, 1), (343, 2, 172, 1), (1369, 6, 229, 1)]
    assert select_layout(512 * 512) == (256, 1, 256, 1)  # the largest frame with one block count a lane
    assert (UNIT1[0] * UNIT1[1]) % 16 != 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_references_run_at_the_sweep_shapes():
    """The restatements at the sizes of the GPU tests, each against another form of itself: the moments against
    float64, the resolve with every pixel at spp / K samples against the moments of E + T (the same bits), the
    select against a per-pixel reading of its own outputs."""
    t0 = time.perf_counter()
    for K, (H, W) in ((2, UNIT1), (3, UNIT1), (2, UNIT4)):
        pl = planes(K, K, H, W, 3)
        S, v = bdpt_amd.batch_moments_numpy(pl)
        S64, v64 = bdpt_amd.batch_moments_numpy(pl, np.float64)
        assert S.dtype == np.float32 and S.shape == (H, W, 3)
        assert np.abs(S - S64).max() <= 2.0 ** -23 * K * np.abs(S64).max()
        # d_b = x_b - mu is off by a few ulps of the float's largest plane value x, so d_b d_b by that times 2 x; the
        # squares of 1e-20 are float32 denormals, exact to 2^-149
        x2 = np.abs(pl).max(0).astype(np.float64) ** 2
        assert np.all(np.abs(v - v64) <= 8 * K * (2.0 ** -23 * np.maximum(v64, x2) + 2.0 ** -149))
    t1 = time.perf_counter()
    for H, W in (UNIT1, UNIT4):
        pl = planes(H, 2, 2, H, W, 3)
        S, v = bdpt_amd.adaptive_resolve_numpy(pl, np.full((H, W), 6, np.int32), 12)
        rs, rv = bdpt_amd.batch_moments_numpy(pl[:, 1] + pl[:, 0])
        assert np.array_equal(bits(S), bits(rs)) and np.array_equal(bits(v), bits(rv))
        m = sample_counts(H, H, W)
        S, v = bdpt_amd.adaptive_resolve_numpy(pl, m, 12)
        t = bdpt_amd.adaptive_splat_scale(12, H * W, 2, int(m.sum()))
        splats = pl[0, 0] * t + pl[1, 0] * t  # all that a pixel without samples of its own holds
        assert np.isfinite(S).all() and v.min() >= 0 and np.array_equal(bits(S[m == 0]), bits(splats[m == 0]))
    t2 = time.perf_counter()
    for H, W in SELECT_SHAPES:
        N = H * W
        for dilate in (False, True):
            for density in SELECT_DENSITIES:
                S, var, m, thr = select_case(density, H, W, dilate)
                lst, m2 = bdpt_amd.adaptive_select_numpy(S, var, m, thr, SELECT_EPS, SELECT_STEP, SELECT_MAX, dilate)
                assert lst.dtype == np.int32 and np.all(np.diff(lst) > 0)
                assert np.array_equal(lst, np.flatnonzero((m2 - m).reshape(-1) == SELECT_STEP)) and m2.max() <= SELECT_MAX
                if density == "random":
                    assert 0.3 * N < lst.size < 0.7 * N, (H, W, dilate, lst.size / N)
                elif density == "one_per_block":
                    assert np.array_equal(lst, np.arange(SEL_ITEMS - 1, N, SEL_ITEMS))
                elif density == "odd_blocks":
                    assert np.array_equal(lst, np.flatnonzero((np.arange(N) // SEL_ITEMS) % 2 == 1))
                else:
                    assert lst.size == {"all": N, "none": 0, "last_pixel": 1}[density] and (lst.size != 1 or lst[0] == N - 1)
    t3 = time.perf_counter()
    print(f"moments {t1 - t0:.2f} s, resolve {t2 - t1:.2f} s, select {t3 - t2:.2f} s")
