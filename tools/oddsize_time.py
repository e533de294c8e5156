"""Device time of FFTUP_FLAG_ODD_SIZE plans against an even neighbour each, in one process.

    python tools/oddsize_time.py [--out-prefix profiles/oddsize]

Ordered us/frame (fftup_execute, medians of alternating batches), fp32, 8-bit input converted on upload:
  smooth      1215x675 -> 2430x1350 (odd, every length 3,5-smooth: Stockham stages of radix 3 and 5 only)
              against 1200x672 -> 2400x1344 with FFTUP_FLAG_GENERIC_KERNELS (the same engine, the same four launches)
  bluestein   1365x767 -> 2730x1534 with FFTUP_FLAG_ANY_SIZE (Bluestein rows AND columns)
              against 1366x768 -> 2732x1536 with FFTUP_FLAG_ANY_SIZE (Bluestein rows, Stockham columns) -- not like for like
Per pair: the frame times, the per-kernel times (fftup_profile_kernels), time per output pixel and its ratio, and what
fftup_plan_describe says.  Prints one JSON object per pair and writes <prefix>_<in>_time.json.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pair(v, synth, odd, odd_flags, even, even_flags, batches, iters):
    rgb_o, rgb_e = synth.frame(5, *odd), synth.frame(5, *even)
    res = {"device": None, "odd": {}, "even": {}}
    with v.Upscaler(*odd, 2.0, 0, 0.2, 0, odd_flags) as po, v.Upscaler(*even, 2.0, 0, 0.2, 0, even_flags) as pe:
        res["device"] = po.device_name
        po.upload_rgb8(rgb_o)
        pe.upload_rgb8(rgb_e)
        po.execute(iters)
        pe.execute(iters)
        to, te = [], []
        for _ in range(batches):                        # (alternating: both plans see the same clocks)
            to.append(po.execute(iters))
            te.append(pe.execute(iters))
        for name, plan, t in (("odd", po, to), ("even", pe, te)):
            k = plan.profile_kernels(iters)
            us = float(np.median(t)) * 1e3
            res[name] = {"description": plan.description, "in": "%dx%d" % (plan.width, plan.height),
                         "out": "%dx%d" % (plan.out_width, plan.out_height), "frame_us": us, "frame_us_min": float(np.min(t)) * 1e3,
                         "frame_us_max": float(np.max(t)) * 1e3, "ns_per_output_pixel": us * 1e3 / (plan.out_width * plan.out_height),
                         "kernels": plan.kernel_names, "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6}
    o, e = res["odd"], res["even"]
    res["odd_over_even"] = o["frame_us"] / e["frame_us"]
    res["odd_over_even_per_output_pixel"] = o["ns_per_output_pixel"] / e["ns_per_output_pixel"]
    res["kernel_ratio"] = [x / y if y else None for x, y in zip(o["kernel_us"], e["kernel_us"])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    pairs = [((1215, 675), v.FLAG_ODD_SIZE, (1200, 672), v.FLAG_GENERIC_KERNELS),
             ((1365, 767), v.FLAG_ODD_SIZE | v.FLAG_ANY_SIZE, (1366, 768), v.FLAG_ANY_SIZE)]
    for odd, of, even, ef in pairs:
        res = pair(v, synth, odd, of, even, ef, a.batches, a.iters)
        print(json.dumps(res))
        if a.out_prefix:
            out = "%s_%dx%d_time.json" % (a.out_prefix, odd[0], odd[1])
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
