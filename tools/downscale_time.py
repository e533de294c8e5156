"""Device time of the FFT downscale mode (FFTUP_FLAG_DOWNSCALE) against its mirror upscale plan, in one process.

    python tools/downscale_time.py [--out profiles/downscale_4096x2048_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o down -- python tools/downscale_time.py --trace 50

Downscale 4096x2048 -> 2048x1024 fp32, 8-bit input converted on upload (planar kernels), against the size-generic upscale plan
2048x1024 -> 4096x2048 (FFTUP_FLAG_GENERIC_KERNELS).  Reports the ordered frame (fftup_execute, medians of alternating batches),
the overlapped frame of a ring of 4 (fftup_execute_ring), the per-kernel times (fftup_profile_kernels) and the byte counts of
fftup_info.  Prints one JSON object and writes it to --out.  --trace N: only N ordered frames of the downscale plan (for a tracer).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    big, small = (4096, 2048), (2048, 1024)
    rgb_big, rgb_small = synth.frame(5, *big), synth.frame(5, *small)
    if a.trace:
        with v.Upscaler(*big, 0.5, 0, 0.2, 0, v.FLAG_DOWNSCALE) as down:
            down.upload_rgb8(rgb_big)
            print("downscale 4096x2048 -> 2048x1024 fp32: %.1f us per ordered frame" % (down.execute(a.trace) * 1e3))
        return
    res = {"device": None, "down": {}, "up": {}}
    with v.Upscaler(*big, 0.5, 0, 0.2, 0, v.FLAG_DOWNSCALE) as down, \
            v.Upscaler(*small, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS) as up:
        res["device"] = down.device_name
        down.upload_rgb8(rgb_big)
        up.upload_rgb8(rgb_small)
        down.execute(a.iters)
        up.execute(a.iters)
        td, tu = [], []
        for _ in range(a.batches):                      # (alternating: both plans see the same clocks)
            td.append(down.execute(a.iters))
            tu.append(up.execute(a.iters))
        for name, plan, t in (("down", down, td), ("up", up, tu)):
            k = plan.profile_kernels(a.iters)
            res[name] = {"description": plan.description, "in": "%dx%d" % (plan.width, plan.height),
                         "out": "%dx%d" % (plan.out_width, plan.out_height), "frame_us": float(np.median(t)) * 1e3,
                         "frame_us_min": float(np.min(t)) * 1e3, "kernels": plan.kernel_names,
                         "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6,
                         "kernel_alg_MB": [x / 1e6 for x in plan.kernel_alg_bytes]}
    for name, W, H, u, flags, rgb in (("down", *big, 0.5, v.FLAG_DOWNSCALE, rgb_big), ("up", *small, 2.0, v.FLAG_GENERIC_KERNELS, rgb_small)):
        with v.Upscaler(W, H, u, 0, 0.2, 0, flags, 4) as p:
            for s in range(4):
                p.upload_rgb8(rgb, s)
            p.execute_ring(8)
            tr = [p.execute_ring(40) / 40 for _ in range(5)]
        res[name]["ring4_frame_us"] = float(np.median(tr)) * 1e3
    d, u = res["down"], res["up"]
    res["down_over_up"] = d["frame_us"] / u["frame_us"]
    res["down_alg_TBps"] = d["alg_MB"] / d["frame_us"]              # (MB per us = TB/s)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
