"""Device time of a mirror view plan (fftup_plan_create_view with FFTUP_FLAG_MIRROR) against the periodic view plan of the same sizes
and view, in one process.  A record, not a gate.

    python tools/mirror_time.py [--out-prefix profiles/mirror]

Ordered us/frame (fftup_execute, medians of seven alternating batches of 20), 8-bit input converted on upload, -p 0 and -p 2:
  1920x1080 -> 3840x2160   pixel centres aligned, the whole frame (origin -0.25, span = the frame); convolution lengths 7680 / 4320
                           (mirror) against 5760 / 3240 (periodic)
  1366x768  -> 1920x1080   the same with FFTUP_FLAG_ANY_SIZE (1366 = 2 * 683: Bluestein forward rows in both plans)
Per case and precision: the two frame times and their ratio, the per-kernel times (fftup_profile_kernels) and their ratios, what
fftup_plan_describe says, and for -p 0 the mirror plan's relative L2 error against the fp64 oracle (tests/mirror_oracle.py) on the
first 64 output rows of the frame that is timed.  Prints one JSON object per case and writes <prefix>_<in>_time.json.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def entry(plan, t, iters):
    k = plan.profile_kernels(iters)
    us = float(np.median(t)) * 1e3
    return {"description": plan.description, "frame_us": us, "frame_us_min": float(np.min(t)) * 1e3, "frame_us_max": float(np.max(t)) * 1e3,
            "kernels": plan.kernel_names, "kernel_us": [x * 1e3 for x in k], "alg_MB": plan.alg_bytes_per_frame / 1e6}


def accuracy(plan, rgb, uW, uH, origin, span, rows=64):
    import mirror_oracle as Mo
    import oraclelib as O
    H, W = rgb.shape[:2]
    pre = plan.download_presharpen().astype(np.float64)[:, :rows]
    x = O.load_lut(0)[np.transpose(rgb, (2, 0, 1))]
    y = Mo.mirror_matrix(H, uH, origin[1], span[1])[:rows] @ x @ Mo.mirror_matrix(W, uW, origin[0], span[0]).T
    sc = uW * uH / (span[0] * span[1])
    return {"rows": rows, "pre_rel_l2": float(np.linalg.norm((sc * pre - y).ravel()) / np.linalg.norm(y.ravel())),
            "pre_max_err": float(np.abs(sc * pre - y).max())}


def case(v, synth, W, H, uW, uH, flags, batches, iters):
    origin, span = ((W / uW - 1) / 2, (H / uH - 1) / 2), (float(W), float(H))
    rgb = synth.frame(5, W, H)
    res = {"device": None, "in": "%dx%d" % (W, H), "out": "%dx%d" % (uW, uH), "origin": origin, "span": span}
    for precision in (0, 2):
        with v.Upscaler.view(W, H, uW, uH, origin, span, precision, 0.2, 0, flags | v.FLAG_MIRROR) as pm, \
                v.Upscaler.view(W, H, uW, uH, origin, span, precision, 0.2, 0, flags) as pp:
            res["device"] = pm.device_name
            plans = (("mirror", pm), ("periodic", pp))
            times = {name: [] for name, _ in plans}
            for _, p in plans:
                p.upload_rgb8(rgb)
                p.execute(iters)
            for _ in range(batches):                        # (alternating: the plans see the same clocks)
                for name, p in plans:
                    times[name].append(p.execute(iters))
            r = {name: entry(p, times[name], iters) for name, p in plans}
            if precision == 0:
                r["mirror"]["accuracy"] = accuracy(pm, rgb, uW, uH, origin, span)
            r["mirror_over_periodic"] = r["mirror"]["frame_us"] / r["periodic"]["frame_us"]
            r["kernel_ratio"] = [a / b if b else None for a, b in zip(r["mirror"]["kernel_us"], r["periodic"]["kernel_us"])]
            res["p%d" % precision] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-prefix", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    for W, H, uW, uH, flags in ((1920, 1080, 3840, 2160, 0), (1366, 768, 1920, 1080, v.FLAG_ANY_SIZE)):
        res = case(v, synth, W, H, uW, uH, flags, a.batches, a.iters)
        print(json.dumps(res))
        if a.out_prefix:
            out = "%s_%dx%d_time.json" % (a.out_prefix, W, H)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
