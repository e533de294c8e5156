"""Host time of a stabilised clip with and without the host copy of the shifts, in one process.  A record, not a gate.

    python tools/stabilise_time.py [--out profiles/stabilise_time.json]

64 frames, 1920x1080 -> 1920x1080, -p 0, 8-bit input read by the row kernel in place, dense planes out (in place), a view a little
inside the frame; the frames alternate between a synthetic frame and a copy of it rolled by (5, 3) pixels.  us/frame by a host clock
around work that ends in ONE wait for the stream (medians of `--rounds` alternating rounds after one warm-up round):
  (a) host    fftup_align_shifts -> blocking copy of the shifts -> views moved on the host -> fftup_execute_device_views
  (b) device  fftup_align_shifts -> fftup_shift_path (ABSOLUTE, sigma 8) -> fftup_execute_device_views_shifted
  (c) direct  fftup_align_shifts -> fftup_execute_device_views_shifted
k_shift_path alone, n = 64 and n = 4096 at sigma 8, between a pair of HIP events on the stream (median of 32 launches; the pair's
own cost is in the figure).  And k_view_tables of a pan with and without a shift pointer: a child process on libfftup_knobs.so with
FFTUP_EXPERIMENT=view_tables_time=1, one lane, which reports each launch on stderr (tools/view_frames_time.py has the method).
Prints one JSON object and writes it to --out.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FRAMES, LANES = 64, 3
W, H = 1920, 1080
VIEW = ((96.0, 54.0), (1728.0, 972.0))


def spread(t):
    return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}


def chains(v, synth, rounds):
    os.environ["FFTUP_STREAMS"] = str(LANES)
    rgb = synth.frame(5, W, H)
    both = np.stack([rgb, np.roll(rgb, (3, 5), (0, 1))])
    out_bytes = 3 * W * H * 4
    with v.Upscaler.view(W, H, W, H, VIEW[0], VIEW[1], 0, 0.2, 0, v.FLAG_FUSE_U8_LOAD) as up, v.Aligner(W, H) as al, v.Stream() as st, \
            v.DeviceBuffer(both.nbytes) as din, v.DeviceBuffer(LANES * out_bytes) as dout, v.DeviceBuffer(16 * FRAMES) as dshift, \
            v.DeviceBuffer(16 * FRAMES) as doffset:
        din.upload(both)
        ref = v.DeviceImage(din.ptr, v.FMT_RGB8, 3 * W)
        ins = [v.DeviceImage(din.ptr + (i % 2) * rgb.nbytes, v.FMT_RGB8, 3 * W) for i in range(FRAMES)]
        outs = [v.DeviceImage(dout.ptr + (i % LANES) * out_bytes, v.FMT_PLANAR, W * 4, W * H * 4) for i in range(FRAMES)]
        views = [VIEW] * FRAMES

        def wait():
            dout.download(16, stream=st)                    # (a blocking copy on the stream: everything before it has finished)

        def host():
            al.shifts_device(ref, ins, dshift.ptr, st)
            est = dshift.download(stream=st).view(np.float32).reshape(FRAMES, 4)
            up.execute_device_views(ins, outs, v.stabilised_views(VIEW, est), st)

        def device():
            al.shifts_device(ref, ins, dshift.ptr, st)
            v.shift_path(dshift.ptr, doffset.ptr, FRAMES, v.PATH_ABSOLUTE, 8.0, 0.0, st)
            up.execute_device_views_shifted(ins, outs, views, doffset.ptr, st)

        def direct():
            al.shifts_device(ref, ins, dshift.ptr, st)
            up.execute_device_views_shifted(ins, outs, views, dshift.ptr, st)

        variants = [("host", host), ("device", device), ("direct", direct)]
        times = {name: [] for name, _ in variants}
        for r in range(rounds + 1):                          # (alternating: the variants see the same clocks; round 0 warms up)
            k = r % len(variants)
            for name, work in variants[k:] + variants[:k]:
                wait()
                t0 = time.perf_counter()
                work()
                wait()
                if r:
                    times[name].append((time.perf_counter() - t0) * 1e6 / FRAMES)
        est = dshift.download().view(np.float32).reshape(FRAMES, 4)
        res = {"description": up.description, "device": up.device_name, "estimated_shift_of_the_rolled_frame": [float(est[1, 0]), float(est[1, 1])]}
        for name, t in times.items():
            res[name + "_per_frame"] = spread(t)
        res["device_over_host"] = res["device_per_frame"]["median_us"] / res["host_per_frame"]["median_us"]
        res["direct_over_host"] = res["direct_per_frame"]["median_us"] / res["host_per_frame"]["median_us"]
    return res


def path_kernel(v):
    from view_frames_time import Events
    res = {}
    with v.Stream() as st, v.DeviceBuffer(16 * 4096) as din, v.DeviceBuffer(16 * 4096) as dout:
        rng = np.random.default_rng(1)
        rows = rng.uniform(-8, 8, (4096, 4)).astype(np.float32)
        rows[:, 2:] = 1.0
        din.upload(rows)
        ev = Events()
        for n in (64, 4096):
            def work():
                v.shift_path(din.ptr, dout.ptr, n, v.PATH_CONSECUTIVE, 8.0, 0.0, st)
            t = [ev.time_us(st.handle, work) for _ in range(36)][4:]
            res["n_%d_sigma_8" % n] = spread(t)
    return res


def pan_child(v, synth):
    """(the child of view_tables) a zoom, then a pan of 32 frames plain and the same pan with a shift pointer, on one lane"""
    rgb = synth.frame(5, W, H)
    n = 32
    zoom = v.views_between(((0.0, 0.0), (float(W), float(H))), VIEW, n)
    pan = v.views_between(VIEW, ((140.0, 80.0), VIEW[1]), n)
    with v.Upscaler.view(W, H, W, H, VIEW[0], VIEW[1], 0, 0.2, 0, v.FLAG_FUSE_U8_LOAD) as up, \
            v.DeviceBuffer(rgb.nbytes) as din, v.DeviceBuffer(3 * W * H * 4) as dout, v.DeviceBuffer(16 * n) as dshift:
        din.upload(rgb)
        dshift.upload(np.tile(np.array([1.25, -0.75, 1.0, 1.0], np.float32), (n, 1)))
        ins = [v.DeviceImage(din.ptr, v.FMT_RGB8, 3 * W)] * n
        outs = [v.DeviceImage(dout.ptr, v.FMT_PLANAR, W * 4, W * H * 4)] * n
        up.execute_device_views(ins, outs, zoom)
        dout.download(16)
        for _ in range(2):                                   # (plain, shifted, plain, shifted)
            up.execute_device_views(ins, outs, pan)
            dout.download(16)
            up.execute_device_views_shifted(ins, outs, pan, dshift.ptr)
            dout.download(16)


def view_tables():
    from vkresample_amd import _lib
    env = dict(os.environ, FFTUP_LIBRARY=_lib.KNOBS_LIB_PATH, FFTUP_EXPERIMENT="view_tables_time=1", FFTUP_STREAMS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pan-child"], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("the k_view_tables child failed:\n" + r.stderr)
    pre = [float(us) for us, x, y in re.findall(r"k_view_tables ([0-9.]+) us \(chirp tables rebuilt: x (\d), y (\d)\)", r.stderr) if (x, y) == ("0", "0")]
    # the zoom ends on the pan's span, so the pans rebuild `pre` alone: the last 4 x 32 such launches are theirs
    if len(pre) < 4 * 32:
        raise SystemExit("the k_view_tables child reported %d pan launches, not %d:\n%s" % (len(pre), 4 * 32, r.stderr[-2000:]))
    pre = pre[-4 * 32:]
    calls = [pre[32 * k:32 * k + 32] for k in range(4)]
    plain, shifted = calls[0][4:] + calls[2][4:], calls[1][4:] + calls[3][4:]
    return {"pan_plain": spread(plain), "pan_shifted": spread(shifted), "launches": [len(plain), len(shifted)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pan-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    import vkresample_amd as v
    from vkresample_amd import synth
    if v.device_count() < 1:
        raise SystemExit("stabilise_time.py needs a HIP device: nothing is measured without one")
    if a.pan_child:
        pan_child(v, synth)
        return
    res = {"frames_per_call": FRAMES, "rounds": a.rounds, "size": "%dx%d" % (W, H), "lanes": LANES,
           "chains_host_clock": chains(v, synth, a.rounds), "shift_path_event_pair": path_kernel(v), "view_tables_event_pair": view_tables()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
