"""Device time of fftup_align_shifts (Aligner.shifts_device): a record, not a gate.

    python tools/align_time.py [--out profiles/align_time.json]

64 pairs per call at 1920x1080 (window 1024 x 1024, d = 1) and at 3840x2160 (d = 2), 8-bit frames and float planes; a pair of HIP
events on one stream around the call, medians of `--rounds` rounds after one warm-up round, in the manner of
tools/view_frames_time.py.  For scale, the same run measures a view frame of the same size (a periodic view plan W x H -> W x H,
8-bit input read by the row kernel, dense planes out) through fftup_execute_device, 64 frames per call, the same event pair.
Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAIRS = 64


def rounds_us(ev, stream, work, wait, rounds):
    t = []
    for r in range(rounds + 1):                              # (round 0 warms up)
        wait()
        us = ev.time_us(stream.handle, work)
        if r:
            t.append(us / PAIRS)
    return {"us_per_item": float(np.median(t)), "us_min_max": [float(np.min(t)), float(np.max(t))]}


def measure(v, synth, Events, W, H, rounds):
    res = {"size": "%dx%d" % (W, H)}
    frames = [synth.frame(5, W, H), np.roll(synth.frame(5, W, H), (3, -2), axis=(0, 1))]
    with v.Stream() as st:
        ev = Events()
        for fmt in ("rgb8", "planar_f32"):
            host = frames if fmt == "rgb8" else [(np.transpose(f, (2, 0, 1)) / 255.0).astype(np.float32) for f in frames]
            bufs = [v.DeviceBuffer(h.nbytes) for h in host]
            for b, h in zip(bufs, host):
                b.upload(h)
            if fmt == "rgb8":
                ims = [v.DeviceImage(b.ptr, v.FMT_RGB8, 3 * W) for b in bufs]
            else:
                ims = [v.DeviceImage(b.ptr, v.FMT_PLANAR, 4 * W, 4 * W * H) for b in bufs]
            with v.Aligner(W, H) as al, v.DeviceBuffer(16 * PAIRS) as out:
                r = rounds_us(ev, st, lambda: al.shifts_device([ims[0]] * PAIRS, [ims[1]] * PAIRS, out.ptr, st),
                              lambda: out.download(16, stream=st), rounds)
                r["info"] = al.info
                r["shift"] = [float(x) for x in out.download(16, stream=st).view(np.float32)]
            res["align_" + fmt] = r
            for b in bufs:
                b.close()
        try:                                                 # the view frame of the same size, for scale
            out_bytes = 3 * W * H * 4
            with v.Upscaler.view(W, H, W, H, (0.25, 0.25), (float(W), float(H)), 0, 0.2, 0, v.FLAG_FUSE_U8_LOAD) as up, \
                    v.DeviceBuffer(frames[0].nbytes) as din, v.DeviceBuffer(3 * out_bytes) as dout:
                din.upload(frames[0])
                ins = [v.DeviceImage(din.ptr, v.FMT_RGB8, 3 * W)] * PAIRS
                outs = [v.DeviceImage(dout.ptr + (i % 3) * out_bytes, v.FMT_PLANAR, 4 * W, 4 * W * H) for i in range(PAIRS)]
                res["view_frame"] = rounds_us(ev, st, lambda: up.execute_device(ins, outs, st), lambda: dout.download(16, stream=st), rounds)
                res["view_frame"]["description"] = up.description
        except v.FftupError as e:
            res["view_frame"] = {"error": str(e)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    from view_frames_time import Events
    if v.device_count() < 1:
        raise SystemExit("align_time.py needs a HIP device: nothing is measured without one")
    res = {"pairs_per_call": PAIRS, "rounds": a.rounds, "device": v.device_name(0),
           "cases": [measure(v, synth, Events, W, H, a.rounds) for (W, H) in ((1920, 1080), (3840, 2160))]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
