"""fftup_shift_path (include/fftup.h, "a smoothed camera path") restated in fp64 numpy: serial loops, one line per rule of the header.
The yardstick of csrc/shift_path.hpp (tests/path/shift_path_driver.cpp on the CPU, k_shift_path on the GPU).  Test infrastructure only.

Bars.  out is rounded to fp32 once: |out - oracle| <= 2^-23 max(|oracle|, 1), one fp32 rounding step at the magnitude of the value
(or of 1).  The fp64 sums behind it -- at most 4096 fp32 values of a few pixels, at most 1537 weights -- carry errors below 1e-8
whatever their order, far under that step; p and s themselves are held at 1e-9 absolute."""
import math

import numpy as np

ABSOLUTE, CONSECUTIVE, MAX_FRAMES = 0, 1, 4096
P_S_BAR = 1e-9


def out_bar(oracle):
    return 2.0 ** -23 * np.maximum(np.abs(oracle), 1.0)


def path(shifts, mode, sigma=0.0, min_peak=0.0):
    """shifts: (n, 4) float32 rows dx, dy, peak, peak_coarse -> (p, s, out): (n, 2) float64 each (out BEFORE its rounding to fp32)"""
    sh = np.asarray(shifts, np.float32).reshape(-1, 4)
    n = len(sh)
    sigma, min_peak = float(np.float32(sigma)), np.float32(min_peak)
    p = np.zeros((n, 2))
    last = np.zeros(2)
    for i in range(n):
        dx, dy, peak = sh[i, 0], sh[i, 1], sh[i, 2]
        measured = bool(peak >= min_peak) and math.isfinite(dx) and math.isfinite(dy)          # (a NaN peak: False)
        if mode == CONSECUTIVE:
            if i > 0 and measured:
                last = last + np.array([dx, dy], np.float64)
        elif measured:
            last = np.array([dx, dy], np.float64)
        p[i] = last
    s = np.zeros((n, 2))
    if sigma > 0.0:
        r = int(math.ceil(3.0 * sigma))
        j = np.arange(-r, r + 1)
        g = np.exp(-(j * j) / (2.0 * sigma * sigma))
        for i in range(n):
            s[i] = (g[:, None] * p[np.clip(i + j, 0, n - 1)]).sum(axis=0) / g.sum()
    return p, s, p - s


def offsets(shifts, mode, sigma=0.0, min_peak=0.0):
    """what fftup_shift_path writes: (n, 4) float32 -- dx, dy = (float)(p - s), peak and peak_coarse copied"""
    sh = np.asarray(shifts, np.float32).reshape(-1, 4)
    out = sh.copy()
    out[:, :2] = path(sh, mode, sigma, min_peak)[2].astype(np.float32)
    return out


# ---- the grid the driver and the kernel are held on: (n, sigma)
GRID = ([(n, s) for n in (1, 2, 7, 63, 64, 65) for s in (0.0, 0.4, 1.5, 8.0)] + [(n, 64.0) for n in (1023, 1024, 1025, 4096)] + [(7, 256.0)])
MODES = (ABSOLUTE, CONSECUTIVE)
MIN_PEAKS = (0.0, 0.5)


def grid_shifts(n, seed):
    """seeded shifts in +-8 px with peaks in [0.2, 1], and planted trouble: a NaN dx, an infinite dx, an infinite dy, a NaN peak"""
    rng = np.random.default_rng(seed)
    sh = np.empty((n, 4), np.float32)
    sh[:, :2] = rng.uniform(-8.0, 8.0, (n, 2))
    sh[:, 2] = rng.uniform(0.2, 1.0, n)
    sh[:, 3] = rng.uniform(0.2, 1.0, n)
    if n >= 7:
        k = rng.choice(np.arange(1, n), 4, replace=False)
        sh[k[0], 0] = np.nan
        sh[k[1], 0] = np.inf
        sh[k[2], 1] = -np.inf
        sh[k[3], 2] = np.nan
    return sh


_cache = {}


def grid_case(n, sigma, mode, min_peak):
    """(shifts, (p, s, out)) of a grid point, computed once and left unchanged"""
    key = (n, sigma, mode, min_peak)
    if key not in _cache:
        sh = grid_shifts(n, 1000 + n)
        res = path(sh, mode, sigma, min_peak)
        for a in (sh,) + res:
            a.flags.writeable = False
        _cache[key] = (sh, res)
    return _cache[key]
