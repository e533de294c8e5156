"""Device time of fftup_roll_angles (Roller.angles_device): a record, not a gate -- there is no earlier figure to compare it with.

    python tools/roll_time.py --device-label "AMD Instinct MI355X" [--out profiles/roll_time.json]

64 pairs per call at 1920x1080 (window 512 x 512, d = 2) and at 3840x2160 (d = 4), 8-bit frames and float planes; a pair of HIP
events on one stream around the call, medians of `--rounds` rounds after one warm-up round, in the manner of tools/align_time.py.
For scale, the same run measures fftup_align_shifts on the same frames and the chain roll -> rotate by -angle (angles read in device
memory) -> align of 16 frames.  Prints one JSON object and writes it to --out; the object says on what
device (`device`: --device-label, required, beside the runtime's own name for it) and when (`measured_at`)."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAIRS = 64
CHAIN = 16


def rounds_us(ev, stream, work, wait, rounds, items):
    t = []
    for r in range(rounds + 1):                              # (round 0 warms up)
        wait()
        us = ev.time_us(stream.handle, work)
        if r:
            t.append(us / items)
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
            with v.Roller(W, H) as ro, v.DeviceBuffer(16 * PAIRS) as out:
                r = rounds_us(ev, st, lambda: ro.angles_device([ims[0]] * PAIRS, [ims[1]] * PAIRS, out.ptr, st),
                              lambda: out.download(16, stream=st), rounds, PAIRS)
                r["info"] = ro.info
                r["angle"] = [float(x) for x in out.download(16, stream=st).view(np.float32)]
            res["roll_" + fmt] = r
            if fmt == "rgb8":
                with v.Aligner(W, H) as al, v.DeviceBuffer(16 * PAIRS) as out:
                    res["align_rgb8"] = rounds_us(ev, st, lambda: al.shifts_device([ims[0]] * PAIRS, [ims[1]] * PAIRS, out.ptr, st),
                                                  lambda: out.download(16, stream=st), rounds, PAIRS)
                try:
                    with v.Roller(W, H) as ro, v.Rotator(W, H, max_batch=CHAIN) as rot, v.Aligner(W, H) as al, v.DeviceBuffer(16 * CHAIN) as ang, \
                            v.DeviceBuffer(16 * CHAIN) as shf, v.DeviceBuffer(CHAIN * frames[0].nbytes) as lvl:
                        level = [v.DeviceImage(lvl.ptr + i * frames[0].nbytes, v.FMT_RGB8, 3 * W) for i in range(CHAIN)]

                        def chain():
                            ro.angles_device([ims[0]] * CHAIN, [ims[1]] * CHAIN, ang.ptr, st)
                            rot.frames_angles([ims[1]] * CHAIN, level, 0.0, ang.ptr, -1.0, st)
                            al.shifts_device([ims[0]] * CHAIN, level, shf.ptr, st)
                        res["chain_roll_rotate_align_rgb8"] = rounds_us(ev, st, chain, lambda: shf.download(16, stream=st), rounds, CHAIN)
                except v.FftupError as e:                    # (a rotator needs 2,3,5,7-smooth sizes)
                    res["chain_roll_rotate_align_rgb8"] = {"error": str(e)}
            for b in bufs:
                b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--device-label", required=True, help="the product the tool runs on, e.g. 'AMD Instinct MI355X': the word of whoever "
                    "runs it, stored beside the runtime's own name for the device (which may be no more than the architecture)")
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    from view_frames_time import Events
    if v.device_count() < 1:
        raise SystemExit("roll_time.py needs a HIP device: nothing is measured without one")
    res = {"pairs_per_call": PAIRS, "chain_frames_per_call": CHAIN, "rounds": a.rounds,
           "device": {"measured_on": a.device_label, "runtime_name": v.device_name(0)},
           "measured_at": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%d %H:%M:%S UTC"),
           "cases": [measure(v, synth, Events, W, H, a.rounds) for (W, H) in ((1920, 1080), (3840, 2160))]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
