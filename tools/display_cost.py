"""Cost of the display output: kernel_ms of bdpt_meter and bdpt_display on device buffers of a 1-spp Caustic
frame - the meter with and without the feature buffers and on a constant image (every lane in one bin), the
display per tone at 3 and 4 channels, meter + display chained - next to a default bdpt_reproject and a one-iteration bdpt_denoise on the same buffers, and next to the host alternative (the float
frame copied out, then display_numpy), in one process; one JSON line per size. Each figure is
the median of --repeat timed calls after a warm-up call.

    python tools/display_cost.py [--sizes 512,1024] [--repeat 9]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("bidirectional-path-tracing_amd", "scenes"):
    sys.path.insert(0, os.path.join(REPO, sub))
import torch  # noqa: E402  (the HIP runtime both bind to, as tests/conftest.py)

import bdpt_amd  # noqa: E402
import variants  # noqa: E402


def median_ms(it, call, repeat):
    ms = []
    for k in range(repeat + 1):  # the first call warms up
        call()
        it.synchronize()
        if k:
            ms.append(it.stats()["kernel_ms"])
    return round(statistics.median(ms), 4)


def measure(size, repeat):
    sc = variants.SCENES["caustic"]
    cam = bdpt_amd.Camera(**sc["camera"])
    cfg = bdpt_amd.Config(camera=cam, width=size, height=size, spp=1, rr_depth=sc["rr_depth"])
    it = bdpt_amd.BDPTIntegrator(bdpt_amd.Scene(variants.obj_path("caustic")), cfg)
    dev = "cuda:0"
    buf = lambda c, dt=torch.float32: torch.zeros(size, size, c, dtype=dt, device=dev)  # noqa: E731
    rgb, aov, hist_a, hist_b, out, den = buf(3), buf(8), buf(8), buf(8), buf(3), buf(3)
    flat = torch.full((size, size, 3), 0.25, device=dev)
    px3, px4 = buf(3, torch.uint8), buf(4, torch.uint8)
    words = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    it.render_device(rgb.data_ptr())
    it.render_aov_device(aov.data_ptr())
    it.reproject_device(cam, rgb.data_ptr(), aov.data_ptr(), 0, out.data_ptr(), hist_a.data_ptr(), cur_samples=1)
    it.synchronize()
    res = dict(size=size)
    res["reproject_ms"] = median_ms(it, lambda: it.reproject_device(cam, rgb.data_ptr(), aov.data_ptr(), hist_a.data_ptr(),
                                                                    out.data_ptr(), hist_b.data_ptr(), cur_samples=1), repeat)
    d1 = bdpt_amd.DenoiseSettings(iterations=1)
    res["denoise_1iter_ms"] = median_ms(it, lambda: it.denoise_device(rgb.data_ptr(), aov.data_ptr(), den.data_ptr(), settings=d1), repeat)

    def meter(color, guides):
        return lambda: it.meter_device(color.data_ptr(), guides.data_ptr() if guides is not None else 0, 0, words.data_ptr())

    res["meter_ms"] = median_ms(it, meter(rgb, None), repeat)
    res["meter_aov_ms"] = median_ms(it, meter(rgb, aov), repeat)
    res["meter_constant_ms"] = median_ms(it, meter(flat, None), repeat)
    it.meter_device(rgb.data_ptr(), aov.data_ptr(), 0, words.data_ptr())
    for tone in bdpt_amd.TONES:
        for ch, px in ((3, px3), (4, px4)):
            s = bdpt_amd.DisplaySettings(tone=tone, channels=ch)
            res[f"display_{tone}_{ch}_ms"] = median_ms(
                it, lambda: it.display_device(rgb.data_ptr(), px.data_ptr(), words.data_ptr(), settings=s), repeat)

    def chain():  # (kernel_ms is per call: the two calls are timed one by one and added)
        it.meter_device(rgb.data_ptr(), aov.data_ptr(), 0, words.data_ptr())
        it.synchronize()
        ms = it.stats()["kernel_ms"]
        it.display_device(rgb.data_ptr(), px3.data_ptr(), words.data_ptr())
        it.synchronize()
        return ms + it.stats()["kernel_ms"]

    chain()
    res["meter_display_ms"] = round(statistics.median(chain() for _ in range(repeat)), 4)
    # the host alternative: the float frame copied out and displayed with numpy
    T = bdpt_amd.display_thresholds("srgb")
    w = words.cpu().numpy().view("uint32")
    host = []
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame = rgb.cpu().numpy()
        t1 = time.perf_counter()
        bdpt_amd.display_numpy(frame, T, bdpt_amd.DisplaySettings(), meter=w)
        host.append((t1 - t0, time.perf_counter() - t1))
    res["host_copy_ms"] = round(1e3 * statistics.median(h[0] for h in host), 3)
    res["host_numpy_ms"] = round(1e3 * statistics.median(h[1] for h in host), 3)
    res["counted"] = int(w[2])
    it.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    for size in (int(s) for s in a.sizes.split(",")):
        print(json.dumps(measure(size, a.repeat)), flush=True)


if __name__ == "__main__":
    main()
