"""Adaptive sampling on the device.

python tools/adaptive_probe.py timings [reps]: Caustic 512^2, 8 spp: bdpt_render_pixels on the full list
against bdpt_render_strategies(1, 2), and bdpt_adaptive_resolve / bdpt_adaptive_select at K = 8 for 512^2
and 1024^2. Device buffers, the library's HIP events around the kernels of each call
(bdpt_stats.kernel_ms), 3 warm-up calls, then `reps` calls: median, min and max in ms.

python tools/adaptive_probe.py mse: Caustic 256^2 and HardLight 64^2, budget 64 spp in 8 batches of
8 passes, at three thresholds: the mean squared error against a 1024-spp frame (another seed) of the
adaptive frame and of a uniform frame of (nearly) the same number of traced samples, and the share of
pixels per sample count.

One JSON object on stdout."""
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "bidirectional-path-tracing_amd"), os.path.join(REPO, "scenes")]
import bdpt_amd  # noqa: E402
import variants  # noqa: E402

WARMUP = 3
K = 8


def integrator(name, width, height, spp, seed_base=None):
    sc = variants.SCENES[name]
    kw = {} if seed_base is None else dict(seed_base=seed_base)
    cfg = bdpt_amd.Config(camera=bdpt_amd.Camera(**sc["camera"]), width=width, height=height, spp=spp,
                          rr_depth=sc["rr_depth"], **kw)
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


def timings(reps):
    dev = torch.device("cuda", 0)
    out = dict(reps=reps, warmup=WARMUP, batches=K, device=torch.cuda.get_device_name(0),
               kernel_build=bdpt_amd.kernel_build_hash())
    side, n = 512, 512 * 512
    it = integrator("caustic", side, side, 8)
    fb = torch.zeros(2 * n * 3, dtype=torch.float32, device=dev)
    full = torch.arange(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    a = timed(it, lambda: it.render_strategies_device(fb.data_ptr(), 1, 2), reps)
    b = timed(it, lambda: it.render_pixels_device(full.data_ptr(), n, fb.data_ptr()), reps)
    assert it.stats()["kernel"] == "bdpt_frame_kernel_pixels"
    out["caustic_512_spp8"] = dict(render_strategies_1x2=a, render_pixels_full_list=b,
                                   pixels_over_strategies=round(b["median_ms"] / a["median_ms"], 4))
    it.close()
    out["state"] = {}
    for side in (512, 1024):
        n = side * side
        it = integrator("hardlight", side, side, 16)
        g = torch.Generator(device=dev).manual_seed(1)
        planes = torch.rand(K * 2 * n * 3, dtype=torch.float32, device=dev, generator=g)
        m = torch.ones(n, dtype=torch.int32, device=dev)
        S, var = (torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2))
        lst = torch.zeros(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        res = dict(resolve_k8=timed(it, lambda: it.adaptive_resolve_device(planes.data_ptr(), m.data_ptr(), K, n,
                                                                            S.data_ptr(), var.data_ptr()), reps))
        s = S.view(-1, 3).sum(1).double() + 1e-3
        thr = float(torch.sqrt(torch.median(var.view(-1, 3).sum(1).double() / (s * s))))

        def select(dilate):
            m.fill_(1)  # (m_max keeps every call's work the same: about half the pixels listed)
            it.adaptive_select_device(S.data_ptr(), var.data_ptr(), m.data_ptr(), lst.data_ptr(), cnt.data_ptr(), thr,
                                      1e-3, 1, 2, dilate)

        res["select"] = timed(it, lambda: select(False), reps)
        res["select_listed"] = int(cnt[0])
        res["select_dilated"] = timed(it, lambda: select(True), reps)
        res["select_dilated_listed"] = int(cnt[0])
        it.close()
        out["state"][f"{side}x{side}"] = res
    return out


def mse_table():
    out = dict(batches=K, step=1, passes=8, budget_spp=64, reference_spp=1024, scenes={})
    for name, side in (("caustic", 256), ("hardlight", 64)):
        ref = integrator(name, side, side, 1024, seed_base=12345).render_frame().astype(np.float64)
        rows = []
        for thr in (0.05, 0.1, 0.2):
            it = integrator(name, side, side, 64)
            frame, _, samples = it.render_adaptive(thr, n_batches=K, step=1, max_passes=8)
            traced = it.adaptive["samples"]
            mean_spp = traced / (side * side)
            u_spp = max(1, round(mean_spp))
            uni = integrator(name, side, side, u_spp, seed_base=777).render_frame().astype(np.float64)
            counts, share = np.unique(samples, return_counts=True)
            rows.append(dict(threshold=thr, passes=it.adaptive["passes"], active=it.adaptive["active"],
                             mean_spp=round(mean_spp, 3), uniform_spp=u_spp,
                             mse_adaptive=float(np.mean((frame - ref) ** 2)), mse_uniform=float(np.mean((uni - ref) ** 2)),
                             share_by_samples={int(c): round(float(s) / samples.size, 4) for c, s in zip(counts, share)}))
        out["scenes"][f"{name}_{side}"] = rows
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "timings"
    if mode == "timings":
        print(json.dumps(timings(int(sys.argv[2]) if len(sys.argv) > 2 else 15)))
    elif mode == "mse":
        print(json.dumps(mse_table()))
    else:
        sys.exit(__doc__)
