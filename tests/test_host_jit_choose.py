"""CPU suite: the plan-time chooser (csrc/jit_choose.hpp) answers what it answered before it became a unit of its own.

tests/jit_choose_driver.cpp, linked with the library's object files, prints every field of the Choice for a request; the fixtures under
tests/golden/ (written by make_jit_choose_golden.py from the chooser as csrc/jit.cpp held it) record the answers:
    jit_choices.txt.gz     all even 2,3,5,7-smooth widths up to 8192, three heights each, every factor D / (2 DD) the planner produces,
                           binary16 storage at u2, with and without the built-in wisdom table; and how many requests have no answer
    jit_candidates.txt.gz  the plan-time tuner's candidate list for every row length and first-radix constraint
    jit_wisdom_rows.json   entries of a wisdom.txt: valid, equal to the pick, of another key, and every way of being invalid
    jit_pin_rows.json      FFTUP_EXPERIMENT pins and switches, through the objects of libfftup_knobs.so; the rows with a "rule" entry
                           are written by hand: a pin that needs more than 16 points per thread is ignored like any other invalid pin
A row that cannot be reproduced says the chooser changed: the fixtures are the reference, not the code."""
import os
import re
import shutil
import subprocess

import pytest

import jit_choose_lib as J
import plan_driver

ROOT = plan_driver.ROOT


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """(the driver, the driver with the test knobs, an empty cache directory)"""
    d = tmp_path_factory.mktemp("jit_choose")
    return plan_driver.build(d, "jit_choose_driver"), plan_driver.build(d, "jit_choose_driver", knobs=True), d / "empty_cache"


def compare(requests, expected, got):
    bad = [(rq, e, g) for rq, e, g in zip(requests, expected, got) if e != g]
    for (rq, e, g) in bad[:20]:
        print("request : %s\nexpected: %s\nreceived: %s" % (rq, e, g))
    assert not bad, "%d of %d answers differ (the first ones are printed)" % (len(bad), len(requests))


def test_choices_over_all_sizes_and_factors(drivers):
    rows, none = J.read_choices(os.path.join(J.GOLDEN, "jit_choices.txt.gz"))
    requests = J.choice_requests()
    assert set(rows) <= set(requests) and len(rows) + none == len(requests)
    compare(requests, [rows.get(rq, "none") for rq in requests], J.run(drivers[0], requests, drivers[2]))


def test_tuner_candidates(drivers):
    rows = [line.split(" = ") for line in J.read_lines(os.path.join(J.GOLDEN, "jit_candidates.txt.gz"))]
    assert [rq for rq, _ in rows] == J.candidate_requests()
    compare([rq for rq, _ in rows], [e for _, e in rows], J.run(drivers[0], [rq for rq, _ in rows], drivers[2]))


def test_wisdom_file_entries(drivers, tmp_path):
    rows = plan_driver.golden_rows("jit_wisdom_rows.json")["rows"]
    got = []
    for i, r in enumerate(rows):
        cache = tmp_path / ("cache%d" % i)
        cache.mkdir()
        (cache / "wisdom.txt").write_text(r["wisdom"])
        got += J.run(drivers[0], [r["request"]], cache)
    compare(["%s: %s with wisdom.txt %r" % (r["name"], r["request"], r["wisdom"]) for r in rows], [r["expect"] for r in rows], got)


def test_experiment_pins(drivers):
    rows = plan_driver.golden_rows("jit_pin_rows.json")["rows"]
    got = [J.run(drivers[1], [r["request"]], drivers[2], r["experiment"])[0] for r in rows]
    compare(["%s: %s with FFTUP_EXPERIMENT=%s" % (r["name"], r["request"], r["experiment"]) for r in rows], [r["expect"] for r in rows], got)
    # ... and the build without the knobs answers every one of them as if nothing were pinned
    plain = J.run(drivers[0], [r["request"] for r in rows], drivers[2])
    assert [J.run(drivers[0], [r["request"]], drivers[2], r["experiment"])[0] for r in rows] == plain


def test_the_sweep_asks_without_wisdom_wherever_the_builtin_table_has_an_entry():
    src = open(os.path.join(ROOT, "vkresample_amd", "csrc", "jit_choose.cpp")).read()
    table = src[src.index("kBuiltinWisdom[] = {"):]
    table = table[:table.index("};")]
    assert sorted({int(m.group(1)) for m in re.finditer(r"\{(\d+), \d+, \"", table)}) == J.BUILTIN_WISDOM_UW


def test_chooser_object_calls_no_runtime():
    """the chooser is arithmetic and a text file: its object references neither the HIP runtime nor hipRTC"""
    nm = shutil.which("nm") or os.path.join(os.path.dirname(plan_driver.HIPCC), "..", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-u", os.path.join(ROOT, "build", "obj", "jit_choose.o")], capture_output=True, text=True, check=True).stdout
    assert out.strip() and not [s for s in out.split() if s.startswith(("hip", "hiprtc", "__hip"))], out
