"""Device time of a view plan (fftup_plan_create_view) against the exact-size plan on the pre-cropped frame, in one process.  A record,
not a gate.

    python tools/view_time.py [--out-prefix profiles/view]

Ordered us/frame (fftup_execute, medians of seven alternating batches of 20), fp32, 8-bit input converted on upload:
  view        a 1920x1080 frame viewed at 2x about its centre: output 1920x1080, origin (480, 270), span (960, 540) -- forward
              transforms of the WHOLE frame, chirp-z transforms (L = 3840 rows, 2160 columns) to the output
  to_size     the crop 960x540 of the same frame -> 1920x1080 with fftup_plan_create_size, corner-aligned: the same output lattice on
              a frame a quarter the size, made periodic at the crop's edges (what a caller without view plans does; the two images
              differ near the edges of the crop, by construction)
Per plan: the frame time, the per-kernel times (fftup_profile_kernels) and what fftup_plan_describe says; for the view plan the
relative L2 error against the fp64 oracle on a 64-row band of the output (tests/view_oracle.py: dense matrices) and the host time of
fftup_plan_set_view for a pan (same span: one table per axis) and for a zoom (all tables).  Prints one JSON object and writes
<prefix>_1920x1080_time.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
ORIGIN, SPAN = (480.0, 270.0), (960.0, 540.0)


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def entry(plan, t, iters):
    k = plan.profile_kernels(iters)
    us = float(np.median(t)) * 1e3
    return {"description": plan.description, "in": "%dx%d" % (plan.width, plan.height), "out": "%dx%d" % (plan.out_width, plan.out_height),
            "frame_us": us, "frame_us_min": float(np.min(t)) * 1e3, "frame_us_max": float(np.max(t)) * 1e3, "kernels": plan.kernel_names,
            "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6}


def accuracy(plan, rgb, rows=64):
    import oraclelib as O
    import view_oracle as V
    pre = plan.download_presharpen().astype(np.float64)[:, :rows]
    x = O.load_lut(0)[np.transpose(rgb, (2, 0, 1))]
    Vx = np.real(V.view_matrix(W, W, ORIGIN[0], SPAN[0]))
    Vy = np.real(V.view_matrix(H, H, ORIGIN[1], SPAN[1]))[:rows]
    y = Vy @ x @ Vx.T
    sc = W * H / (SPAN[0] * SPAN[1])
    return {"rows": rows, "pre_rel_l2": rel_l2(sc * pre, y), "pre_max_err": float(np.abs(sc * pre - y).max())}


def set_view_ms(plan, views, reps=5):
    t = []
    for _ in range(reps):
        for o, s in views:
            t0 = time.perf_counter()
            plan.set_view(o, s)
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    rgb = synth.frame(5, W, H)
    crop = np.ascontiguousarray(rgb[int(ORIGIN[1]):int(ORIGIN[1] + SPAN[1]), int(ORIGIN[0]):int(ORIGIN[0] + SPAN[0])])
    res = {"device": None}
    with v.Upscaler.view(W, H, W, H, ORIGIN, SPAN) as pv, v.Upscaler.to_size(int(SPAN[0]), int(SPAN[1]), W, H) as ps:
        res["device"] = pv.device_name
        plans = (("view", pv, rgb), ("to_size_on_crop", ps, crop))
        times = {name: [] for name, _, _ in plans}
        for _, p, f in plans:
            p.upload_rgb8(f)
            p.execute(a.iters)
        for _ in range(a.batches):                          # (alternating: the plans see the same clocks)
            for name, p, _ in plans:
                times[name].append(p.execute(a.iters))
        for name, p, _ in plans:
            res[name] = entry(p, times[name], a.iters)
        res["view"]["accuracy"] = accuracy(pv, rgb)
        res["view"]["set_view_pan_ms"] = set_view_ms(pv, [((481.25, 270.5), SPAN), (ORIGIN, SPAN)])
        res["view"]["set_view_zoom_ms"] = set_view_ms(pv, [(ORIGIN, (1000.0, 562.5)), (ORIGIN, SPAN)])
    res["view_over_to_size_on_crop"] = res["view"]["frame_us"] / res["to_size_on_crop"]["frame_us"]
    print(json.dumps(res))
    if a.out_prefix:
        out = "%s_%dx%d_time.json" % (a.out_prefix, W, H)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
