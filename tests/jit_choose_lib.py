"""The plan-time chooser's driver (tests/jit_choose_driver.cpp) for the CPU suite: the request lists behind the fixtures
tests/golden/jit_choices.txt.gz and jit_candidates.txt.gz, the fixtures' file format, and one call that runs a driver over requests.
Shared by tests/test_host_jit_choose.py and tests/golden/make_jit_choose_golden.py (which wrote the fixtures)."""
import gzip
import os
import subprocess

import plan_driver

GOLDEN = plan_driver.GOLDEN
# every (D, DD) the planner can produce: the factor is D / (2 DD)
FACTORS = [(3, 1), (4, 1), (5, 1), (6, 1), (8, 1), (10, 1), (14, 1), (16, 1), (5, 2), (7, 2), (9, 4), (15, 4), (8, 3), (10, 3), (16, 5), (14, 5), (16, 7)]
# the row lengths of kBuiltinWisdom (csrc/jit_choose.cpp); test_host_jit_choose.py holds the list to the table
BUILTIN_WISDOM_UW = [768, 1080, 1200, 1280, 1344, 1440, 1500, 1536, 1600, 1728, 1800, 1920, 2240, 2688, 2880, 3200, 3600, 3840, 4000, 4480,
                     4608, 4800, 5040, 5120, 5376, 5760, 6000, 6144, 8000]


def smooth():
    """all even 2,3,5,7-smooth sizes in 64..8192"""
    return sorted({2 ** a * 3 ** b * 5 ** c * 7 ** d for a in range(1, 14) for b in range(6) for c in range(6) for d in range(5)
                   if 64 <= 2 ** a * 3 ** b * 5 ** c * 7 ** d <= 8192})


def choice_requests():
    """jit_choices.txt.gz: every width, three heights each (the stride rule of test_jit_chooser_invariants_over_all_sizes and two
    further offsets), every factor, binary16 storage for D = 4, and the structural default where a built-in wisdom entry may apply"""
    s = smooth()
    out = []
    for i, W in enumerate(s):
        for off in (3, 71, 149):
            H = s[(i * 7 + off) % len(s)]
            for (D, DD) in FACTORS:
                for half in ((0, 1) if D == 4 else (0,)):
                    out.append("choose %d %d %d %d %d 1 -" % (W, H, D, DD, half))
                    if (D * W) % (2 * DD) == 0 and D * W // (2 * DD) in BUILTIN_WISDOM_UW:
                        out.append("choose %d %d %d %d %d 0 -" % (W, H, D, DD, half))
    return out


def candidate_requests():
    """jit_candidates.txt.gz: the tuner's five candidates for every row length and first-radix constraint"""
    return (["cands %d %d 1 5" % (n, D) for n in smooth() for D in (3, 4, 5, 6, 8, 10)]
            + ["cands %d %d %d 5" % (n, D, DD) for n in smooth() for D in (5, 7, 9, 15) for DD in (2, 4)])


def write_text(path, text):
    """a fixture of thousands of recorded lines, gzip'ed (no name, no time in the header: the same text gives the same bytes)"""
    with open(path, "wb") as raw, gzip.GzipFile("", "wb", 9, raw, 0) as f:
        f.write(text.encode())


def read_lines(path):
    with gzip.open(path, "rt") as f:
        return f.read().splitlines()


def run(exe, requests, cache_dir, experiment=None):
    """one answer line per request; FFTUP_CACHE_DIR = `cache_dir` (its wisdom.txt, if any, is consulted), FFTUP_EXPERIMENT =
    `experiment` (read by the build with the test knobs only)"""
    env = {k: v for k, v in os.environ.items() if k not in ("FFTUP_EXPERIMENT", "FFTUP_JIT", "FFTUP_STREAMS")}
    env["FFTUP_CACHE_DIR"] = str(cache_dir)
    if experiment is not None:
        env["FFTUP_EXPERIMENT"] = experiment
    p = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert len(out) == len(requests)
    return out


# jit_choices.txt.gz: a choose answer is four parts joined by " | " (row, column, fused kernel, stand-alone C2R), and every part is shared
# by many requests (the row part depends on W alone, the column part on H and the factor, ...), so the file holds every distinct part
# once ("part TEXT", numbered in order from 0), then "row W H D DD half use_wisdom = i j k l" for every request that succeeds (all of
# them have the empty device key), then "none COUNT" for those that do not.
def write_choices(path, requests, answers):
    parts, rows, none = {}, [], 0
    for rq, a in zip(requests, answers):
        if a == "none":
            none += 1
            continue
        assert rq.startswith("choose ") and rq.endswith(" -")
        rows.append("row %s = %s" % (rq[7:-2], " ".join(str(parts.setdefault(p, len(parts))) for p in a.split(" | "))))
    write_text(path, "".join("part %s\n" % p for p in parts) + "\n".join(rows) + "\nnone %d\n" % none)


def read_choices(path):
    """({request: expected answer}, number of requests without one)"""
    parts, rows, none = [], {}, None
    for line in read_lines(path):
        kind, rest = line.split(" ", 1)
        if kind == "part":
            parts.append(rest)
        elif kind == "row":
            rq, idx = rest.split(" = ")
            rows["choose %s -" % rq] = " | ".join(parts[int(i)] for i in idx.split())
        else:
            assert kind == "none"
            none = int(rest)
    return rows, none
