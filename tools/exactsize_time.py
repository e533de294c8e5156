"""Device time and accuracy of an exact-size plan (fftup_plan_create_size) against its FFTUP_FLAG_ANY_SIZE neighbour, in one process.

    python tools/exactsize_time.py [--out-prefix profiles/exactsize]

Ordered us/frame (fftup_execute, medians of alternating batches), fp32, 8-bit input converted on upload:
  exact       1366x768 -> 1920x1080 with FFTUP_FLAG_ANY_SIZE, pixel centres aligned (Bluestein forward rows, Stockham everywhere
              else, one complex multiply per kept bin), and the same plan corner-aligned (no phase tables: what the multiply costs)
  neighbour   1366x768 -> 2732x1536 -u 2 with FFTUP_FLAG_ANY_SIZE (Bluestein rows both ways, polyphase column pass) -- the row of
              the README's table it stands beside; not like for like: twice the output pixels
Per plan: the frame time, the per-kernel times (fftup_profile_kernels), time per output pixel and what fftup_plan_describe says;
for the exact plans the relative L2 error of the amplitude-preserving pre-sharpen image and of the sharpened output against the fp64
oracle (tests/exactsize_oracle.py, oraclelib.sharpen with the effective factor; the frame is uniform noise, as in the neighbouring
timing tools: the sharpened output's maximum error is that of the filter's square-root slope on such frames,
tests/test_gpu_parity.py).  Prints one JSON object and writes <prefix>_1366x768_time.json.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = (1366, 768, 1920, 1080)


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def entry(plan, t, iters):
    k = plan.profile_kernels(iters)
    us = float(np.median(t)) * 1e3
    return {"description": plan.description, "in": "%dx%d" % (plan.width, plan.height), "out": "%dx%d" % (plan.out_width, plan.out_height),
            "frame_us": us, "frame_us_min": float(np.min(t)) * 1e3, "frame_us_max": float(np.max(t)) * 1e3,
            "ns_per_output_pixel": us * 1e3 / (plan.out_width * plan.out_height), "kernels": plan.kernel_names,
            "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6}


def accuracy(plan, rgb, align):
    import exactsize_oracle as E
    import oraclelib as O
    W, H, uW, uH = SIZE
    pre = plan.download_presharpen().astype(np.float64)
    out = plan.download_planar().astype(np.float64)
    x = O.load_lut(0)[np.transpose(rgb, (2, 0, 1))]
    R = E.resample_R(x, uW, uH, align)
    sh = O.sharpen(R, E.effective_factor(W, H, uW, uH), 0, 0.2)
    sc = uW * uH / (W * H)
    return {"pre_rel_l2": rel_l2(sc * pre, sc * R), "pre_max_err": float(np.abs(sc * pre - sc * R).max()),
            "out_rel_l2": rel_l2(out[:, :-1], sh[:, :-1]), "out_max_err": float(np.abs(out[:, :-1] - sh[:, :-1]).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    W, H, uW, uH = SIZE
    rgb = synth.frame(5, W, H)
    res = {"device": None}
    with v.Upscaler.to_size(W, H, uW, uH, 0, 0.2, 0, v.FLAG_ANY_SIZE, align=v.ALIGN_CENTRE) as pc, \
            v.Upscaler.to_size(W, H, uW, uH, 0, 0.2, 0, v.FLAG_ANY_SIZE, align=v.ALIGN_CORNER) as pk, \
            v.Upscaler(W, H, 2.0, 0, 0.2, 0, v.FLAG_ANY_SIZE) as pn:
        res["device"] = pc.device_name
        plans = (("exact_centres", pc), ("exact_corners", pk), ("anysize_u2", pn))
        times = {name: [] for name, _ in plans}
        for _, p in plans:
            p.upload_rgb8(rgb)
            p.execute(a.iters)
        for _ in range(a.batches):                          # (alternating: the plans see the same clocks)
            for name, p in plans:
                times[name].append(p.execute(a.iters))
        for name, p in plans:
            res[name] = entry(p, times[name], a.iters)
        res["exact_centres"]["accuracy"] = accuracy(pc, rgb, v.ALIGN_CENTRE)
        res["exact_corners"]["accuracy"] = accuracy(pk, rgb, v.ALIGN_CORNER)
    c, k, n = res["exact_centres"], res["exact_corners"], res["anysize_u2"]
    res["centres_over_corners"] = c["frame_us"] / k["frame_us"]
    res["exact_over_anysize_u2"] = c["frame_us"] / n["frame_us"]
    res["exact_over_anysize_u2_per_output_pixel"] = c["ns_per_output_pixel"] / n["ns_per_output_pixel"]
    print(json.dumps(res))
    if a.out_prefix:
        out = "%s_%dx%d_time.json" % (a.out_prefix, W, H)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
