"""Sample batches, their moments and the variance-guided filter on the device.

python tools/batch_var_probe.py timings [scene] [reps]: for 512^2 and 1024^2, bdpt_batch_moments at
K = 8, bdpt_denoise_var at its default iterations against bdpt_denoise at the same iteration count, and
an 8-spp frame rendered as 8 batches against one 8-spp bdpt_render. Device buffers, the library's HIP
events around the kernels of each call (bdpt_stats.kernel_ms), 3 warm-up calls, then `reps` calls:
median, min and max in ms; for the batched render also the host clock around the 8 asynchronous
launches and one synchronise.

python tools/batch_var_probe.py grid: the grid the header's BDPT_DENOISE_VAR_* defaults come from:
HardLight 64 x 64, 8 spp in 8 batches, against its 256-spp frame; iterations 3..5 x sigma_color 0.5, 1,
2, 4, 8; the mean squared error of every point, of the unfiltered sum and of bdpt_denoise's defaults.

One JSON object on stdout."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bidirectional-path-tracing_amd"), os.path.join(REPO, "scenes")]
import bdpt_amd  # noqa: E402
import variants  # noqa: E402

WARMUP = 3
K = 8


def integrator(name, width, height, spp):
    sc = variants.SCENES[name]
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=width, height=height, spp=spp,
                          rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path(name)), cfg)
    it.init()
    return it


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def timed(it, call, reps):
    ms = []
    for r in range(WARMUP + reps):
        call()
        it.synchronize()
        if r >= WARMUP:
            ms.append(it.stats()["kernel_ms"])
    return spread(ms)


def timings(name, reps):
    dev = torch.device("cuda", 0)
    out = dict(scene=name, reps=reps, warmup=WARMUP, batches=K, device=torch.cuda.get_device_name(0),
               kernel_build=bdpt_amd.kernel_build_hash(), sizes={})
    iterations = bdpt_amd.denoise_var_settings().iterations
    for side in (512, 1024):
        n = side * side
        planes = torch.zeros(K * n * 3, dtype=torch.float32, device=dev)
        rgb, var, den = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(3))
        aov = torch.zeros(n * 8, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        it = integrator(name, side, side, K)
        wins = bdpt_amd.batch_windows(K, K)
        res = {}
        # the 8-spp frame in one call, and as 8 one-sample batches: per-call kernel times summed, and
        # the host clock around the 8 asynchronous launches
        res["bdpt_render_spp8"] = timed(it, lambda: it.render_device(rgb.data_ptr()), reps)
        sums, walls = [], []
        for r in range(WARMUP + reps):
            planes.zero_()
            torch.cuda.synchronize()
            total = 0.0
            for b, w in enumerate(wins):
                it.render_device(planes.data_ptr() + b * n * 12, window=w)
                it.synchronize()
                total += it.stats()["kernel_ms"]
            planes.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it.render_batches_device(K, planes.data_ptr())
            it.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                sums.append(total), walls.append(wall)
        res["render_8_batches_kernel_sum"] = spread(sums)
        res["render_8_batches_host_clock"] = spread(walls)
        res["batches_over_render"] = round(res["render_8_batches_kernel_sum"]["median_ms"] /
                                           res["bdpt_render_spp8"]["median_ms"], 3)
        res["batch_moments_k8"] = timed(
            it, lambda: it.batch_moments_device(planes.data_ptr(), K, side, side, rgb.data_ptr(), var.data_ptr()), reps)
        it.render_aov_device(aov.data_ptr())
        it.synchronize()
        res[f"denoise_var_{iterations}_iterations"] = timed(
            it, lambda: it.denoise_var_device(rgb.data_ptr(), var.data_ptr(), aov.data_ptr(), den.data_ptr()), reps)
        assert bool(torch.isfinite(den).all()) and bool(torch.isfinite(var).all())
        res[f"denoise_{iterations}_iterations"] = timed(
            it, lambda: it.denoise_device(rgb.data_ptr(), aov.data_ptr(), den.data_ptr(),
                                          settings=bdpt_amd.DenoiseSettings(iterations=iterations)), reps)
        res["denoise_var_over_denoise"] = round(res[f"denoise_var_{iterations}_iterations"]["median_ms"] /
                                                res[f"denoise_{iterations}_iterations"]["median_ms"], 3)
        it.close()
        out["sizes"][f"{side}x{side}"] = res
    return out


def grid():
    ref = integrator("hardlight", 64, 64, 256).render_frame().astype(np.float64)
    it = integrator("hardlight", 64, 64, 8)
    it.render_batches(K)
    noisy, _ = it.batch_moments()
    it.render_aov()

    def mse(x):
        return float(np.mean((x - ref) ** 2))

    points = {}
    for iterations in (3, 4, 5):
        for sigma_color in (0.5, 1.0, 2.0, 4.0, 8.0):
            points[f"{iterations}/{sigma_color:g}"] = mse(it.denoise_var(iterations=iterations, sigma_color=sigma_color))
    best = min(points, key=points.get)
    return dict(scene="hardlight", frame="64x64, 8 spp in 8 batches, against 256 spp", unfiltered_sum=mse(noisy),
                denoise_defaults=mse(it.denoise()), denoise_var_defaults=mse(it.denoise_var()),
                grid_iterations_over_sigma_color=points, best=best)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "timings"
    if mode == "grid":
        print(json.dumps(grid()))
    else:
        print(json.dumps(timings(sys.argv[2] if len(sys.argv) > 2 else "caustic",
                                 int(sys.argv[3]) if len(sys.argv) > 3 else 15)))
