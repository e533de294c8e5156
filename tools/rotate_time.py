"""Device time of fftup_rotate_frames (Rotator.rotate): a record, not a gate.

    python tools/rotate_time.py [--out profiles/rotate_time.json]

64 frames per call at 1920x1080 and at 3840x2160, 8-bit frames (in place: out[i] = in[i]) and float planes (out of place), angles
from -0.05 to 0.05 rad about the frame centre on a rotator with max_batch = 16.  us/frame by a host clock around work that ends in
ONE wait for the stream, medians of `--rounds` alternating rounds after one warm-up round, with min and max -- the variants of a
size take turns inside a round, so they see the same clocks.  For scale, the same rounds time a view frame of the same size (a
periodic view plan W x H -> W x H, 8-bit input read by the row kernel, dense planes out) through fftup_execute_device, 64 frames
per call.  And the three kernels one by one: tools/ub/rotate_kernels (built from tools/ub/rotate_kernels.hip, see its first lines)
puts a pair of events around each launch of a chunk of 16 frames on one stream; where the program has not been built the entry
says so.  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 64
KERNELS_EXE = os.path.join(ROOT, "tools", "ub", "rotate_kernels")


def spread(t):
    return {"us_per_frame": float(np.median(t)), "us_min_max": [float(np.min(t)), float(np.max(t))]}


def kernels(W, H, rounds):
    """the three kernels one by one, in a child process of its own"""
    if not os.path.exists(KERNELS_EXE):
        return {"error": "not measured: tools/ub/rotate_kernels is not built"}
    out = {}
    for kind, name in ((0, "rgb8"), (1, "planar_f32")):
        p = subprocess.run([KERNELS_EXE, str(W), str(H), "16", str(rounds), str(kind)], capture_output=True, text=True, timeout=120)
        out[name] = json.loads(p.stdout) if p.returncode == 0 else {"error": (p.stderr or p.stdout)[-300:]}
    return out


def measure(v, synth, W, H, rounds):
    res = {"size": "%dx%d" % (W, H)}
    rgb = synth.frame(5, W, H)
    planes = (np.transpose(rgb, (2, 0, 1)) / 255.0).astype(np.float32)
    angles = [float(a) for a in np.linspace(-0.05, 0.05, FRAMES)]
    out_bytes = 3 * W * H * 4
    n_buf = 4                                                # (frames cycle through a few buffers: 64 4K float frames would be 6 GB)
    with v.Stream() as st, v.Rotator(W, H, max_batch=16) as rot, \
            v.Upscaler.view(W, H, W, H, (0.25, 0.25), (float(W), float(H)), 0, 0.2, 0, v.FLAG_FUSE_U8_LOAD) as up, \
            v.DeviceBuffer(n_buf * rgb.nbytes) as d8, v.DeviceBuffer(planes.nbytes) as dpin, v.DeviceBuffer(n_buf * out_bytes) as dpout:
        for i in range(n_buf):
            d8.upload(rgb, offset=i * rgb.nbytes)
        dpin.upload(planes)
        im8 = [v.DeviceImage(d8.ptr + (i % n_buf) * rgb.nbytes, v.FMT_RGB8, 3 * W) for i in range(FRAMES)]
        pin = [v.DeviceImage(dpin.ptr, v.FMT_PLANAR, 4 * W, 4 * W * H)] * FRAMES
        pout = [v.DeviceImage(dpout.ptr + (i % n_buf) * out_bytes, v.FMT_PLANAR, 4 * W, 4 * W * H) for i in range(FRAMES)]
        vin = [v.DeviceImage(d8.ptr, v.FMT_RGB8, 3 * W)] * FRAMES
        variants = {
            "rotate_rgb8_in_place": lambda: rot.rotate(im8, im8, angles, st),
            "rotate_planar_f32": lambda: rot.rotate(pin, pout, angles, st),
            "view_frame": lambda: up.execute_device(vin, pout, st),
        }
        times = {k: [] for k in variants}
        for r in range(rounds + 1):                          # (alternating: the variants see the same clocks; round 0 warms up)
            for name, work in variants.items():
                dpout.download(16, stream=st)                # (the stream is idle)
                t0 = time.perf_counter()
                work()
                dpout.download(16, stream=st)                # ONE wait, behind everything the call enqueued
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e6 / FRAMES)
        for name, t in times.items():
            res[name] = spread(t)
        res["rotator"] = rot.info
        res["view_frame"]["description"] = up.description
    res["kernels"] = kernels(W, H, rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    if v.device_count() < 1:
        raise SystemExit("rotate_time.py needs a HIP device: nothing is measured without one")
    res = {"frames_per_call": FRAMES, "rounds": a.rounds, "device": v.device_name(0),
           "cases": [measure(v, synth, W, H, a.rounds) for (W, H) in ((1920, 1080), (3840, 2160))]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
