"""CPU: everything tests/test_gpu_align_edges.py takes for granted, proven on the fp64 oracle (tests/align_oracle.py) and the
device-free geometry rules alone -- the table of tests/align_edge_cases.py: every pair's coarse gap, the far row's coarse cell, the
oracle against the truth, the literals of the bars recomputed, the cap on the pairs that leave the tight shift bar, the forty-five
pairs, the no-signal results, and the geometry of every row from the library's own rules (tests/align_rules_driver.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import align_edge_cases as EC
import align_oracle as AO
import plan_driver as PD


@pytest.fixture(scope="module")
def estimates():
    """{(row, format): (fp64 estimates, complex64 estimates)} of every row's pairs: computed once, shared, left unchanged"""
    out = {}
    for r in EC.ROWS:
        g = EC.geometry(r)
        ref, moved, _ = EC.row_clip(r)
        for fmt, conv in EC.FORMATS.items():
            a = conv(ref)
            out[(r[0], fmt)] = ([AO.estimate(a, conv(c), g) for c in moved], [AO.estimate(a, conv(c), g, single=True) for c in moved])
    return out


def test_every_pair_has_a_clear_coarse_peak(estimates):
    """oracle gap > 1e-3 for every pair of every row in the three formats; per row the smallest is the figure beside its seed"""
    for r in EC.ROWS:
        gaps = [o["gap"] for fmt in EC.FORMATS for o in estimates[(r[0], fmt)][0]]
        print("MEASURED %s seed %d: smallest oracle gap %.3g over %d pairs" % (r[0], r[8], min(gaps), len(gaps)))
        assert min(gaps) > 1e-3, (r[0], gaps)


def test_far_row_peaks_far_from_the_origin(estimates):
    """the coarse cell at least n / 5 from 0 on both axes (signed), and the true shift recovered within 0.06 px"""
    r = EC.row("far")
    g = EC.geometry(r)
    true = EC.row_clip(r)[2]
    for fmt in EC.FORMATS:
        for o, (tx, ty) in zip(estimates[("far", fmt)][0], true):
            px, py = o["coarse"]
            sx, sy = (px if px < g["nx"] - px else px - g["nx"]), (py if py < g["ny"] - py else py - g["ny"])
            assert abs(sx) >= g["nx"] / 5 and abs(sy) >= g["ny"] / 5, (fmt, o)
            assert abs(sx - tx) <= 1 and abs(sy - ty) <= 1, (fmt, o)
            assert abs(o["dx"] - tx) <= 0.06 and abs(o["dy"] - ty) <= 0.06, (fmt, o, tx, ty)


def test_oracle_recovers_the_small_shifts(estimates):
    """rows whose shifts are at most 4 decimated pixels: the oracle within 0.5 decimated pixels of the truth (band01 and d8 have
    too few bins for that; they only have to match the oracle)"""
    for r in EC.ROWS:
        if r[0] in EC.NOT_HELD_TO_THE_TRUTH or max(max(abs(x), abs(y)) for (x, y) in r[7]) > 4:
            continue
        d, true = r[4], EC.row_clip(r)[2]
        worst = 0.0
        for fmt in EC.FORMATS:
            for o, (tx, ty) in zip(estimates[(r[0], fmt)][0], true):
                worst = max(worst, abs(o["dx"] - tx) / d, abs(o["dy"] - ty) / d)
        print("MEASURED %s: oracle within %.3f decimated px of the truth" % (r[0], worst))
        assert worst <= 0.5, r[0]
    assert sorted(r[0] for r in EC.ROWS if max(max(abs(x), abs(y)) for (x, y) in r[7]) > 4) == ["far"]


def test_bars_are_the_oracles_own_single_precision_scatter(estimates):
    """EDGE_PEAK_C64 and every row's shift_c64, recomputed: the largest complex64-vs-complex128 difference.  The complex64 run is a
    sample of rounding noise, and its sums change their order with the matrix-product kernel and the thread count numpy finds on
    the machine (band1: 1.9e-6 with eight threads, 3.0e-6 with three; band099: 3.0e-6 and 1.6e-6 with one; min16: 4.0e-6 on one
    processor's kernels, 3.5e-6 on another's -- up to 1.83 times apart over six such settings), so a literal cannot be met digit
    for digit everywhere: each has to lie within a factor of three of the figure recomputed here, either way -- inside the factor
    4 that the bars put on top of it."""
    peak = 0.0
    for r in EC.ROWS:
        figs = [EC.figures(*estimates[(r[0], fmt)], r[4]) for fmt in EC.FORMATS]
        dp, ds = max(f[0] for f in figs), max(f[1] for f in figs)
        print("MEASURED %s: peak c64/c128 %.3g, shift c64/c128 %.3g decimated px (literal %.3g), tight bar %.3g px, hard bar %.3g px"
              % (r[0], dp, ds, r[9], EC.tight_bar(r), r[4] / r[6]))
        peak = max(peak, dp)
        assert r[9] / 3 <= ds <= 3 * r[9], (r[0], ds)
        assert EC.tight_bar(r) < r[4] / r[6]                       # (the tight bar is the tighter one)
    print("MEASURED all rows: peak c64/c128 %.3g (literal %.3g)" % (peak, EC.EDGE_PEAK_C64))
    assert EC.EDGE_PEAK_C64 / 3 <= peak <= 3 * EC.EDGE_PEAK_C64 and EC.EDGE_PEAK_BAR == 4 * EC.EDGE_PEAK_C64


def test_tight_shift_cap(estimates):
    """at least 5 of every 7 pairs per row and format qualify for the tight bar (a row with fewer pairs may lose one), at
    least 90 % of all"""
    q_all = n_all = 0
    for r in EC.ROWS:
        for fmt in EC.FORMATS:
            q = [EC.qualifies(o) for o in estimates[(r[0], fmt)][0]]
            need = -(-5 * len(q) // 7) if len(q) >= 7 else len(q) - 1
            assert sum(q) >= need, (r[0], fmt, q)
            q_all, n_all = q_all + sum(q), n_all + len(q)
            for o in estimates[(r[0], fmt)][0]:
                assert abs(o["dx_"]) <= 0.5 and abs(o["dy_"]) <= 0.5 and o["K"] > 0
    print("MEASURED tight shift bar: %d of %d pairs qualify" % (q_all, n_all))
    assert q_all >= 0.9 * n_all


def test_forty_five_pairs():
    """the order puts every frame but the last in both positions, and each chosen pair has an oracle gap > 1e-3 in the three formats
    (measured: at least 4.5e-3)"""
    assert len(EC.LONG_PAIRS) == 45 == len(set(EC.LONG_PAIRS)) and all(a != b for a, b in EC.LONG_PAIRS)
    refs, curs = {a for a, _ in EC.LONG_PAIRS}, {b for _, b in EC.LONG_PAIRS}
    assert 0 in refs and 0 in curs and len(refs & curs) >= 7
    assert EC.LONG_MAX_BATCH == 40 and 45 - EC.LONG_MAX_BATCH == 5              # launches of 16, 16, 8; then a chunk of 5
    W, H, window, d = EC.LONG_CASE
    g = AO.geometry(W, H, window, d)
    worst = 1.0
    for fmt, conv in EC.FORMATS.items():
        fr = [conv(f) for f in EC.long_frames()]
        for a, b in EC.LONG_PAIRS:
            worst = min(worst, AO.estimate(fr[a], fr[b], g)["gap"])
    print("MEASURED forty-five pairs: smallest oracle gap %.3g" % worst)
    assert worst > 1e-3


@pytest.mark.parametrize("name", EC.NO_SIGNAL_ROWS)
def test_no_signal_on_the_oracle(name):
    """black-black, black-frame and frame-black: the oracle's result is (-d, -d, 0, 0), the tie rule alone -- P[0,0] is exactly 0,
    although the packed transform of step 2 leaves a rounding residue of the other frame in the black frame's bins (the fp64
    oracle too: 1e-17 of it, which a floor of 1e-9 |P[0,0]| = 0 alone would let through as unit phasors)"""
    W, H, window, d, band, kappa, ref, cur, black = EC.no_signal_case(name)
    g = AO.geometry(W, H, window, d, band, kappa)
    for conv in EC.FORMATS.values():
        r, c, b = conv(ref), conv(cur), conv(black)
        assert not AO.windowed(b, g).any() and AO.windowed(r, g).any()
        for pair in ((b, b), (b, r), (r, b)):
            for single in (False, True):
                o = AO.estimate(pair[0], pair[1], g, single=single)
                assert (o["dx"], o["dy"], o["peak"], o["peak_coarse"]) == EC.dead_result(d), o
                assert o["coarse"] == (0, 0) and o["fine"] == (0, 0) and o["gap"] == 0.0
        live = AO.estimate(r, c, g)
        assert live["gap"] > 1e-3 and abs(live["dx"]) > 0.5 * d and live["peak"] > 0.5, live


def test_geometry_of_every_row_from_the_librarys_rules(tmp_path):
    """align_geometry (csrc/plan_rules.cpp) through the device-free driver of tests/test_host_align.py equals AO.geometry; and the
    branches the rows are there for: Kx = n_x at band 1, band_kx = n_x / 2 - 1 at 0.99, K of a few dozen bins at 0.1"""
    exe = PD.build(tmp_path, "align_rules_driver")
    lines = ["%d %d 0 %d %d %d %s %d 3" % (r[1], r[2], r[3][0], r[3][1], r[4], float(r[5]).hex(), r[6]) for r in EC.ROWS]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert len(out) == len(EC.ROWS)
    for r, got in zip(EC.ROWS, out):
        g = EC.geometry(r)
        assert got == "ok %d %d %d %d %d %d %d %d" % (g["d"], g["nx"], g["ny"], g["crop_x"], g["crop_y"], g["kappa"], g["band_kx"], g["band_ky"]), (r[0], got, g)
        assert (g["nx"], g["ny"], g["d"], g["kappa"]) == (r[3][0], r[3][1], r[4], r[6])
    G = {r[0]: EC.geometry(r) for r in EC.ROWS}
    assert (G["band1"]["band_kx"], G["band1"]["band_ky"]) == (32, 16) and (G["band099"]["band_kx"], G["band099"]["band_ky"]) == (31, 15)
    assert (G["band01"]["band_kx"], G["band01"]["band_ky"]) == (3, 1) and (G["band025"]["band_kx"], G["band025"]["band_ky"]) == (16, 8)
    assert G["tall"]["ny"] > G["tall"]["nx"] and G["min16"]["nx"] == 16 and G["x1024"]["nx"] == 1024 and G["y1024"]["ny"] == 1024
