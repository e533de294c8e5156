"""Device time of a clip whose view moves, fftup_execute_device_views, against the same plan at a fixed view and against the
fftup_plan_set_view loop it replaces, in one process.  A record, not a gate.

    python tools/view_frames_time.py [--out profiles/view_frames_time.json]

Two plans, -p 0, 8-bit input read by the row kernel, dense planes out (both in place: no staging kernel), 64 frames per call:
  1920x1080 -> 1920x1080   periodic view plan, the 2x zoom about the centre as the fixed view
  1366x768  -> 1920x1080   FFTUP_FLAG_MIRROR | FFTUP_FLAG_ANY_SIZE, the whole frame with centres aligned as the fixed view
Per plan, us/frame by a host clock around the call and a wait for its stream (medians of `--rounds` alternating rounds after one
warm-up round):
  (a) fixed    fftup_execute_device, the plan's own view
  (b) pan      fftup_execute_device_views, the span of (a), a moving origin: k_view_tables rebuilds `pre` alone
  (c) zoom     fftup_execute_device_views, origin and span move (views_between): all three tables per axis, every frame
  (d) set_view a loop of fftup_plan_set_view + fftup_execute_device of one frame: host tables, blocking copies
and the ratios (b)/(a), (c)/(a), (d)/(c).  k_view_tables on its own, two ways: (i) between a pair of timing events around the
kernel's launch -- a child process on libfftup_knobs.so with FFTUP_EXPERIMENT=view_tables_time=1, one lane, which reports each
launch on stderr (medians over the frames of a pan and of a zoom; the pair's own cost is in the figure); (ii) the plan again on
ONE lane (FFTUP_STREAMS=1: the frames of a call run one after the other) with a pair of HIP events on the caller's stream around
each call: the per-frame difference of (c) and (b) to (a) is what the kernel adds to a lane when nothing overlaps it.  Prints one
JSON object and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 64


class Events:
    """a pair of timing events of the HIP runtime the library is linked to"""

    def __init__(self):
        # (the copy libfftup.so has loaded: events of another copy would mean nothing to its streams)
        loaded = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]
        self.hip = C.CDLL(loaded[0])
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_us(self, stream, work):
        s = C.c_void_p(stream)
        assert self.hip.hipEventRecord(self.a, s) == 0
        work()
        assert self.hip.hipEventRecord(self.b, s) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3


def clip(v, W, H, uW, uH, flags, fixed, pan_to, zoom_from):
    """-> the plan's constructor arguments and the three view lists"""
    pan = v.views_between(fixed, (pan_to, fixed[1]), FRAMES)
    zoom = v.views_between((zoom_from[0], zoom_from[1]), fixed, FRAMES)
    return dict(W=W, H=H, uW=uW, uH=uH, flags=flags | v.FLAG_FUSE_U8_LOAD, fixed=fixed, pan=pan, zoom=zoom)


def measure(v, synth, c, rounds, lanes):
    os.environ["FFTUP_STREAMS"] = str(lanes)
    W, H, uW, uH = c["W"], c["H"], c["uW"], c["uH"]
    rgb = synth.frame(5, W, H)
    out_bytes = 3 * uW * uH * 4
    res = {}
    with v.Upscaler.view(W, H, uW, uH, c["fixed"][0], c["fixed"][1], 0, 0.2, 0, c["flags"]) as up, v.Stream() as st, \
            v.DeviceBuffer(rgb.nbytes) as din, v.DeviceBuffer(lanes * out_bytes) as dout:
        din.upload(rgb)
        ins = [v.DeviceImage(din.ptr, v.FMT_RGB8, 3 * W)] * FRAMES
        outs = [v.DeviceImage(dout.ptr + (i % lanes) * out_bytes, v.FMT_PLANAR, uW * 4, uW * uH * 4) for i in range(FRAMES)]   # (frame i runs on lane i % lanes)
        ev = Events() if lanes == 1 else None

        def wait():
            dout.download(16, stream=st)                    # (a blocking copy on the stream: everything before it has finished)

        def set_view_loop():
            for (o, s) in c["zoom"]:
                up.set_view(o, s)
                up.execute_device(ins[0], outs[0], st)
            up.set_view(*c["fixed"])

        variants = [("fixed", lambda: up.execute_device(ins, outs, st)), ("pan", lambda: up.execute_device_views(ins, outs, c["pan"], st)),
                    ("zoom", lambda: up.execute_device_views(ins, outs, c["zoom"], st))]
        if lanes > 1:
            variants.append(("set_view", set_view_loop))
        times = {name: [] for name, _ in variants}
        for r in range(rounds + 1):                          # (alternating: the variants see the same clocks; round 0 warms up)
            k = r % len(variants)
            for name, work in variants[k:] + variants[:k]:   # (... and every variant follows every other one in turn)
                variants[0][1]()                             # an untimed call first: the set_view loop leaves the GPU half idle
                wait()
                if ev:
                    t = ev.time_us(st.handle, work)
                else:
                    t0 = time.perf_counter()
                    work()
                    wait()
                    t = (time.perf_counter() - t0) * 1e6
                if r:
                    times[name].append(t / FRAMES)
        res["description"], res["device"] = up.description, up.device_name
        for name, t in times.items():
            res[name + "_us"] = float(np.median(t))
            res[name + "_us_min_max"] = [float(np.min(t)), float(np.max(t))]
    return res


def kernel_child(v, synth, c):
    """(the child of kernel_alone) a zoom and a pan of 32 frames on one lane; the library reports every k_view_tables on stderr"""
    W, H, uW, uH = c["W"], c["H"], c["uW"], c["uH"]
    rgb = synth.frame(5, W, H)
    n = 32
    with v.Upscaler.view(W, H, uW, uH, c["fixed"][0], c["fixed"][1], 0, 0.2, 0, c["flags"]) as up, \
            v.DeviceBuffer(rgb.nbytes) as din, v.DeviceBuffer(3 * uW * uH * 4) as dout:
        din.upload(rgb)
        ins = [v.DeviceImage(din.ptr, v.FMT_RGB8, 3 * W)] * n
        outs = [v.DeviceImage(dout.ptr, v.FMT_PLANAR, uW * 4, uW * uH * 4)] * n
        for views in (c["zoom"][:n], c["pan"][:n]):
            up.execute_device_views(ins, outs, views)
            dout.download(16)


def kernel_alone(index):
    """-> {"pre_only_us", "all_us"}: medians of the event pairs around k_view_tables (the first frames of each kind left out)"""
    from vkresample_amd import _lib
    env = dict(os.environ, FFTUP_LIBRARY=_lib.KNOBS_LIB_PATH, FFTUP_EXPERIMENT="view_tables_time=1", FFTUP_STREAMS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", str(index)], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("the k_view_tables child failed:\n" + r.stderr)
    got = {(0, 0): [], (1, 1): []}
    for us, x, y in re.findall(r"k_view_tables ([0-9.]+) us \(chirp tables rebuilt: x (\d), y (\d)\)", r.stderr):
        if (int(x), int(y)) in got:
            got[(int(x), int(y))].append(float(us))
    return {"pre_only_us": float(np.median(got[(0, 0)][4:])), "all_us": float(np.median(got[(1, 1)][4:])),
            "launches": [len(got[(0, 0)]), len(got[(1, 1)])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    if v.device_count() < 1:
        raise SystemExit("view_frames_time.py needs a HIP device: nothing is measured without one")
    cases = [clip(v, 1920, 1080, 1920, 1080, 0, ((480.0, 270.0), (960.0, 540.0)), (900.0, 500.0), ((0.0, 0.0), (1920.0, 1080.0))),
             clip(v, 1366, 768, 1920, 1080, v.FLAG_MIRROR | v.FLAG_ANY_SIZE, ((-0.144, -0.144), (1366.0, 768.0)), (40.0, 20.0), ((340.0, 190.0), (683.0, 384.0)))]
    if a.kernel_child is not None:
        kernel_child(v, synth, cases[a.kernel_child])
        return
    res = {"frames_per_call": FRAMES, "rounds": a.rounds, "cases": []}
    for index, c in enumerate(cases):
        lanes3 = measure(v, synth, c, a.rounds, 3)
        lane1 = measure(v, synth, c, a.rounds, 1)
        r = {"in": "%dx%d" % (c["W"], c["H"]), "out": "%dx%d" % (c["uW"], c["uH"]), "mirror": bool(c["flags"] & v.FLAG_MIRROR),
             "three_lanes_host_clock": lanes3, "one_lane_event_pair": lane1, "view_tables_event_pair": kernel_alone(index),
             "pan_over_fixed": lanes3["pan_us"] / lanes3["fixed_us"], "zoom_over_fixed": lanes3["zoom_us"] / lanes3["fixed_us"],
             "set_view_over_zoom": lanes3["set_view_us"] / lanes3["zoom_us"],
             "view_tables_pre_only_us": lane1["pan_us"] - lane1["fixed_us"], "view_tables_all_us": lane1["zoom_us"] - lane1["fixed_us"]}
        res["cases"].append(r)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
