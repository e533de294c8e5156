"""Device time of an FFTUP_FLAG_ANY_SIZE plan (Bluestein transforms) against the size-generic plan of the neighbouring smooth size,
in one process.

    python tools/anysize_time.py [--out profiles/anysize_1366x768_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o anysize -- python tools/anysize_time.py --trace 50

1366x768 -> 2732x1536 fp32 (rows 1366 and 2732 through Bluestein transforms, columns untouched), 8-bit input converted on upload,
against 1372x768 -> 2744x1536 with FFTUP_FLAG_GENERIC_KERNELS (the same kernels with Stockham rows).  Reports the ordered frame
(fftup_execute, medians of alternating batches), the per-kernel times (fftup_profile_kernels) and the Bluestein lengths and tile
width the plan chose (fftup_plan_describe).  Prints one JSON object and writes it to --out.  --trace N: only N ordered frames of
the any-size plan (for a tracer).
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
    odd, smooth = (1366, 768), (1372, 768)
    rgb_odd, rgb_smooth = synth.frame(5, *odd), synth.frame(5, *smooth)
    if a.trace:
        with v.Upscaler(*odd, 2.0, 0, 0.2, 0, v.FLAG_ANY_SIZE) as p:
            p.upload_rgb8(rgb_odd)
            print("any-size 1366x768 -> 2732x1536 fp32: %.1f us per ordered frame" % (p.execute(a.trace) * 1e3))
        return
    res = {"device": None, "anysize": {}, "smooth": {}}
    with v.Upscaler(*odd, 2.0, 0, 0.2, 0, v.FLAG_ANY_SIZE) as bz, v.Upscaler(*smooth, 2.0, 0, 0.2, 0, v.FLAG_GENERIC_KERNELS) as sm:
        res["device"] = bz.device_name
        bz.upload_rgb8(rgb_odd)
        sm.upload_rgb8(rgb_smooth)
        bz.execute(a.iters)
        sm.execute(a.iters)
        tb, ts = [], []
        for _ in range(a.batches):                      # (alternating: both plans see the same clocks)
            tb.append(bz.execute(a.iters))
            ts.append(sm.execute(a.iters))
        for name, plan, t in (("anysize", bz, tb), ("smooth", sm, ts)):
            k = plan.profile_kernels(a.iters)
            res[name] = {"description": plan.description, "in": "%dx%d" % (plan.width, plan.height),
                         "out": "%dx%d" % (plan.out_width, plan.out_height), "frame_us": float(np.median(t)) * 1e3,
                         "frame_us_min": float(np.min(t)) * 1e3, "kernels": plan.kernel_names,
                         "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6}
    b, s = res["anysize"], res["smooth"]
    res["anysize_over_smooth"] = b["frame_us"] / s["frame_us"]
    res["kernel_ratio"] = [x / y if y else None for x, y in zip(b["kernel_us"], s["kernel_us"])]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
