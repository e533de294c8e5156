"""The device-free planner driver (tests/plan_rules_driver.cpp) for the CPU suite: built from the library's own object files (plan_rules,
the kernel facts of fftup_launch, the chooser of jit) and run over a list of requests with the device facts recorded in
tests/golden/plan_geometry.json (an MI355X).  Shared by tests/test_host_plan_rules.py and tests/test_host_family_sweep.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def golden_rows(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def build(d, name="plan_rules_driver", knobs=False):
    """the executable of the driver tests/`name`.cpp in the directory `d`, linked with the library's objects; knobs: with the
    objects of libfftup_knobs.so (jit_knobs.o in place of jit.o: FFTUP_EXPERIMENT is read)"""
    exe = os.path.join(str(d), name + ("_knobs" if knobs else ""))
    obj = os.path.join(ROOT, "build", "obj")
    objs = sorted(os.path.join(obj, f) for f in os.listdir(obj) if f.endswith(".o") and f != ("jit.o" if knobs else "jit_knobs.o"))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                           "-x", "hip", os.path.join(ROOT, "tests", name + ".cpp"), "-x", "none"] + objs + ["-o", exe])
    return exe


def request_line(entry, width, height, upscale=1.0, precision=0, flags=0, ring=0, out=(0, 0), align=0, view=(0.0, 0.0, 0.0, 0.0), sharpen=None):
    """one request in the driver's input format (floats in hex); sharpen None: the driver's 0.2"""
    return " ".join([entry, str(width), str(height), float(upscale).hex(), str(precision), str(flags), str(ring),
                     str(out[0]), str(out[1]), str(align)] + [float(x).hex() for x in view] + ([] if sharpen is None else [float(sharpen).hex()]))


def run(exe, d, requests):
    """one output line per request line: every PlanGeometry field, or "error CODE TEXT"; an empty cache directory under `d`, so
    that no wisdom file changes a factorization"""
    dev = golden_rows("plan_geometry.json")["device"]
    lines = ["device %d %d %s" % (dev["lds_bytes"], dev["compute_units"], dev["arch"])] + list(requests)
    env = {k: v for k, v in os.environ.items() if k not in ("FFTUP_EXPERIMENT", "FFTUP_JIT", "FFTUP_STREAMS")}
    env["FFTUP_CACHE_DIR"] = os.path.join(str(d), "empty_cache")
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert len(out) == len(requests)
    return out


def fields(line):
    """the name=value pairs of one geometry line"""
    return dict(kv.split("=", 1) for kv in line.split())
