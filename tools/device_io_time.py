"""Batch time of fftup_execute_device on caller-owned device memory against fftup_execute_ring on ring slots, in one process.

    python tools/device_io_time.py [--out profiles/device_io_2048x1024_time.json]

2048x1024 -> 4096x2048, fp32, planar in and out, dense, 64 distinct frames:
  device   execute_device(n_frames=64) on a plan with ring = 1: 64 input and 64 output images in caller memory (DeviceBuffer), read
           and written in place by the frame's first and last kernel
  ring     execute_ring(64) on a plan with ring = 8: the same frames' first eight in the slots (the benchmark's headline path)
Both run the same three kernels per frame on the plan's FFTUP_STREAMS lanes.  The two alternate; seven batches each (after one of
warm-up), the median is the figure.  Both sides are timed on the host clock from the call to the end of the batch (execute_ring
returns there; the device batch is asynchronous, so it is followed by an empty blocking fftup_device_copy, which only waits); the
ring's own event time is kept beside it.  The ring = 1 plan is created with FFTUP_FLAG_OVERLAP_ITERATIONS, which lays the fused
kernel's strips out for overlapping frames as a ring does (strip_length, csrc/plan_rules.cpp); `device_sequential_layout` is the same call on a plan
without the flag.  A record, not a gate: `device_minus_ring_us_per_frame` against `ring_spread_us_per_frame` (max - min of the seven
ring batches) says whether the difference is above the noise.

The measurement runs in a child process under `timeout -k 10`, so that a hang ends it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N = 2048, 1024, 64


def measure(batches):
    import vkresample_amd as v
    lib = v._lib.load()
    esz = 4
    uW, uH = 2 * W, 2 * H
    in_bytes, out_bytes = 3 * W * H * esz, 3 * uW * uH * esz
    rng = np.random.Generator(np.random.PCG64(11))
    base = rng.random((3, H, W), dtype=np.float32)
    frames = [np.roll(base, (i, 3 * i), axis=(1, 2)) if i else base for i in range(N)]     # 64 distinct frames
    res = {}
    with v.Upscaler(W, H, 2.0, 0, ring=1, flags=v.FLAG_OVERLAP_ITERATIONS) as pd, v.Upscaler(W, H, 2.0, 0, ring=1) as ps, \
            v.Upscaler(W, H, 2.0, 0, ring=8) as pr, v.DeviceBuffer(N * in_bytes) as din, v.DeviceBuffer(N * out_bytes) as dout:
        res["device_name"] = pd.device_name
        res["plans"] = {"device": pd.description, "ring": pr.description}
        for i, f in enumerate(frames):
            din.upload(f, offset=i * in_bytes)
        for s in range(8):
            pr.upload_planar(frames[s], slot=s)
        ins = [v.DeviceImage(din.ptr + i * in_bytes, v.FMT_PLANAR, W * esz, W * H * esz) for i in range(N)]
        outs = [v.DeviceImage(dout.ptr + i * out_bytes, v.FMT_PLANAR, uW * esz, uW * uH * esz) for i in range(N)]

        def wait():
            assert lib.fftup_device_copy(dout.ptr, dout.ptr, 0, 2, None) == 0

        def t_device(plan):
            wait()
            t0 = time.perf_counter()
            plan.execute_device(ins, outs)
            wait()
            return (time.perf_counter() - t0) * 1e3

        def t_ring():
            t0 = time.perf_counter()
            ev = pr.execute_ring(N)
            return (time.perf_counter() - t0) * 1e3, ev

        t_device(pd), t_device(ps), t_ring()                 # warm-up
        td, ts, tr, te = [], [], [], []
        for _ in range(batches):                             # (alternating: both see the same clocks)
            td.append(t_device(pd))
            r, e = t_ring()
            tr.append(r)
            te.append(e)
            ts.append(t_device(ps))
        # same bits: frame 3 of the device batch against slot 3 of the ring (both plans cut the fused kernel's strips alike)
        pr.execute_ring(8)
        same = bool(np.array_equal(dout.download(out_bytes, 3 * out_bytes), pr.download_planar(3).reshape(-1).view(np.uint8)))

    def stats(t):
        return {"batch_ms": t, "median_ms": float(np.median(t)), "us_per_frame": float(np.median(t)) * 1e3 / N,
                "frames_per_s": N / (float(np.median(t)) * 1e-3)}
    res["device"], res["ring"], res["device_sequential_layout"] = stats(td), stats(tr), stats(ts)
    res["ring"]["event_batch_ms"] = te
    res["ring"]["event_us_per_frame"] = float(np.median(te)) * 1e3 / N
    res["device_over_ring"] = res["device"]["median_ms"] / res["ring"]["median_ms"]
    res["device_minus_ring_us_per_frame"] = res["device"]["us_per_frame"] - res["ring"]["us_per_frame"]
    res["ring_spread_us_per_frame"] = (max(tr) - min(tr)) * 1e3 / N
    res["frame3_equals_ring_slot3"] = same
    res["config"] = {"in": "%dx%d" % (W, H), "out": "%dx%d" % (uW, uH), "precision": 0, "format": "planar, dense", "n_frames": N,
                     "batches": batches, "streams": os.environ.get("FFTUP_STREAMS", "3 (default)")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.batches)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--batches", str(a.batches)],
                       stdout=subprocess.PIPE)
    if r.returncode != 0:
        sys.stderr.write("device_io_time: the measurement ended with status %d\n" % r.returncode)
        return r.returncode
    res = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
