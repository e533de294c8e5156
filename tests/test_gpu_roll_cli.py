"""GPU: `vkresample -stabilise -roll` -- per frame the roll against frame 000001 is estimated, the frame turned back by it (the angle
read in device memory), the level frame's shift estimated and the shifted view rendered.  The files are, byte for byte, what the same
chain gives through the Python classes; the printed angles are the library's; -roll without -stabilise is refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import paritylib as P
import roll_cases as RC
import roll_oracle as RL
from devimage import RGB8, Image

pytestmark = pytest.mark.gpu


def test_cli_stabilise_roll_renders_the_bytes_of_the_python_chain(tmp_path):
    import vkresample_amd as v
    case = RL.GPU_CASES[1]
    W, H = case[:2]
    ref, moved, true = RC.scene(case)
    frames = [ref] + list(moved[1:4])
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for k, f in enumerate(frames):
        P.png_write(str(src / ("%06d.png" % (k + 1))), f)
    r = subprocess.run([P.CLI, "-stabilise", "-roll", "-ifolder", str(src), "-ofolder", str(dst), "-numfiles", "4", "-size", "%dx%d" % (W, H), "-s", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^frame (\d{6}): shift (-?\d+\.\d{3}) (-?\d+\.\d{3}) peak (-?\d+\.\d{3}) roll (-?\d+\.\d{5}) rollpeak (-?\d+\.\d{3})$", r.stdout, re.M)
    assert [l[0] for l in lines] == ["%06d" % (k + 1) for k in range(4)], r.stdout
    ims = [Image(RGB8, W, H, 1, frame=f) for f in frames]
    level = [Image(RGB8, W, H, 1) for _ in frames]
    outs = [Image(RGB8, W, H, 1) for _ in frames]
    view = ((0.0, 0.0), (float(W), float(H)))
    try:
        d, lv = [im.image for im in ims], [im.image for im in level]
        with v.Roller(W, H) as ro, v.Rotator(W, H) as rot, v.Aligner(W, H) as al, v.DeviceBuffer(16 * 4) as ang, v.DeviceBuffer(16 * 4) as shf, \
                v.Upscaler.view(W, H, W, H, view[0], view[1], sharpen=0.0) as up:
            ro.angles_device(d[0], d, ang.ptr)
            rot.frames_angles(d, lv, 0.0, ang.ptr, -1.0)
            al.shifts_device(lv[0], lv, shf.ptr)
            up.execute_device_views_shifted(lv, [o.image for o in outs], [view] * 4, shf.ptr)
            want = [o.read()[0] for o in outs]
            angles = ang.download().view(np.float32).reshape(4, 4).copy()
            shifts = shf.download().view(np.float32).reshape(4, 4).copy()
    finally:
        for im in ims + level + outs:
            im.close()
    for l, a, s, t in zip(lines, angles, shifts, [0.0] + list(true[1:4])):
        assert abs(float(l[4]) - a[0]) <= 0.000005 + 2.0 ** -23 and abs(float(l[1]) - s[0]) <= 0.0005 + 2.0 ** -23 * max(abs(s[0]), 1), (l, a, s)
        assert abs(a[0] - t) <= RL.ACCURACY_BAR[(W, H)], (a, t)
    assert sorted(os.listdir(dst)) == ["%06d.png" % (k + 1) for k in range(4)]
    for k in range(4):
        assert np.array_equal(P.png_read(str(dst / ("%06d.png" % (k + 1)))), want[k].reshape(H, W, 3)), k
    assert not np.array_equal(want[3].reshape(H, W, 3), frames[3])


def test_cli_roll_needs_stabilise(tmp_path):
    r = subprocess.run([P.CLI, "-roll", "-i", str(tmp_path / "none.png"), "-o", str(tmp_path / "o.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-roll undoes camera roll under -stabilise" in r.stdout
    assert not os.path.exists(tmp_path / "o.png")
