"""The edges of the view plans' geometry (csrc/plan_rules.cpp: check_view, view_col_tk; csrc/view_tables.hpp: kmax_of, conv_length;
csrc/mirror_tables.hpp): the literal table of shapes and views that tests/test_gpu_view_edges.py runs k_row_r2c_odd, k_col_view,
k_row_view_c2r and their mirror siblings at, the views of its per-frame calls, the probes that tell a plan one bin off from a right
one, and the oracle of a row.  Test infrastructure only: no test lives here and nothing needs a device;
tests/test_view_edge_oracle.py recomputes every literal below (kmax and L from the oracles' rules, TK and the accept / reject pair
through the device-free planner) and proves on the fp64 oracles alone what the GPU tests rest on.

Edges and the rows that reach them.
    column tiles of 4, 2, 1        tk4, tk2, tk1 (periodic), tk4_m, tk2_m, tk1_m (mirror): W = 8, so 5 spectrum columns -- the last
                                   tile is partial at TK 4 (1 of 4) and TK 2 (1 of 2); tk4_trunc: step 2.5 along x, 2 columns, fewer
                                   than one tile; tk2_bz: a Bluestein forward length (2625) above L_y (1960) decides TK
    the largest column convolution ymax, ymax_m: L_y = 9604 (two buffers of 9637 points, padded, are the 160 KB); REJECTED: L_y = 9720
    step 1/64, step 8              step64, step8 and their _m siblings; k0, k0_y, k0_m: step 8 on so short an axis that kmax = 0
    the floor in kmax              kflip_lo / kflip_hi (N M / (2 span) an integer, and the next double), nyq_kept / nyq_dropped
                                   (span = M and the next double on even N), their _m siblings; mirror_cap / mirror_cap_hi (the cap
                                   N, the zero bin, and N - 1 uncapped: the same map), mcap_lo / mcap_hi (N - 1 and N - 2 cosines)
    far origins                    far, far_m (1e9 pixels), farther, farther_m (2^49 pixels), far_refl_m (span > 2N from an origin left of -N:
                                   reflected copies)
    the smallest lengths           min2, min3, min2_m

Step bounds: every such row keeps its other axis near step 1.  With both axes at 1/64, sc = uW uH / (span_x span_y) = 4096 and the
binary16 R = y / sc of a -p 2 plan falls into subnormals -- a property of the storage type, not an edge of a kernel.

kmax = 0 (k0, k0_m: one spectrum column; k0_y: one spectrum row): the output is constant along that axis, the mean of the input
line.  The rows' other axis is a quarter-pixel shift at step 1, not the identity: with the identity and a step of exactly 8,
R = y / sc = 8 mean is the plain sum of eight input values, and on binary16 input (-p 2) one such sum in eight is an exact tie
between two binary16 numbers (24 of k0's 216 values), which the fp64 oracle and the fp32 kernels break by their own last bits --
the fraction bars mean nothing there.  mean_view is the row's view with that shift taken out, for the -p 0 test that holds the
plan to the input's means without an oracle in between.

Bars: those of tests/paritylib.py, unchanged, for every row.
"""
import functools

import numpy as np

import mirror_oracle as Mo
import view_oracle as V

MIRROR, ANY, U8 = 4096, 1024, 2          # FFTUP_FLAG_MIRROR, FFTUP_FLAG_ANY_SIZE, FFTUP_FLAG_FUSE_U8_LOAD (the row also runs on 8-bit input)


def _up(x):
    return float(np.nextafter(x, np.inf))


FAR = (1e9 + 0.37, -1e9 - 0.61)
# 2^49 pixels: a double still holds eighths of a pixel there.  An 80-bit long double carries 2 f origin / N for 1e9 pixels to 1e-10
# of a turn with or without a reduction of the origin; here it would be left with 1e-4 of a turn, so only these rows need the fmod
FARTHER = (2.0 ** 49 + 0.375, -2.0 ** 49 - 0.625)

# (name, W, H, uW, uH, origin, span, flags, kmax_x, kmax_y, L_x, L_y, TK)
#   mirror rows: kmax by csrc/mirror_tables.hpp (min(N, floor(N M / max(span, M))): what the plan reports), L >= 2N + M
ROWS = (
    # ---- column tiles
    ("tk4", 8, 640, 8, 720, (0.3, 0.7), (8.0, 640.0), 0, 4, 320, 16, 1372, 4),
    ("tk4_trunc", 8, 640, 8, 720, (0.3, 0.7), (20.0, 640.0), 0, 1, 320, 16, 1372, 4),
    ("tk2", 8, 1280, 8, 1280, (0.3, 0.7), (8.0, 1280.0), U8, 4, 640, 16, 2560, 2),
    ("tk1", 8, 2048, 8, 3072, (0.3, 0.7), (8.0, 2048.0), 0, 4, 1024, 16, 5120, 1),
    ("tk2_bz", 8, 1306, 8, 640, (0.3, 0.7), (8.0, 1306.0), ANY, 4, 320, 16, 1960, 2),
    ("tk4_m", 8, 400, 8, 480, (0.3, 0.7), (8.0, 400.0), MIRROR | U8, 8, 400, 24, 1280, 4),
    ("tk2_m", 8, 800, 8, 960, (0.3, 0.7), (8.0, 800.0), MIRROR, 8, 800, 24, 2560, 2),
    ("tk1_m", 8, 1600, 8, 1920, (0.3, 0.7), (8.0, 1600.0), MIRROR, 8, 1600, 24, 5120, 1),
    # ---- the largest column convolution (ymax: a half-pixel shift in y, the oracle through FFTs)
    ("ymax", 8, 4802, 8, 4802, (0.0, 0.5), (8.0, 4802.0), 0, 4, 2401, 16, 9604, 1),
    ("ymax_m", 8, 3200, 8, 3204, (0.3, 0.7), (8.0, 3200.0), MIRROR, 8, 3200, 24, 9604, 1),
    # ---- the closed step bounds
    ("step64", 48, 40, 40, 36, (10.3, 0.25), (0.625, 40.0), 0, 24, 18, 90, 80, 8),
    ("step8", 48, 40, 40, 36, (0.4, -3.25), (48.0, 288.0), 0, 20, 2, 90, 80, 8),
    ("step64_m", 48, 40, 40, 36, (10.3, 0.25), (0.625, 40.0), MIRROR, 48, 36, 140, 120, 8),
    ("step8_m", 48, 40, 40, 36, (0.4, -3.25), (48.0, 288.0), MIRROR, 40, 5, 140, 120, 8),
    ("k0", 8, 12, 6, 12, (0.3, 0.25), (48.0, 12.0), 0, 0, 6, 14, 24, 8),
    ("k0_y", 12, 8, 12, 6, (0.25, 0.3), (12.0, 48.0), 0, 6, 0, 24, 14, 8),
    ("k0_m", 4, 12, 6, 12, (0.3, 0.25), (48.0, 12.0), MIRROR, 0, 12, 14, 36, 8),
    # ---- the floor in kmax
    ("kflip_lo", 48, 40, 40, 36, (5.5, 2.25), (60.0, 45.0), U8, 16, 16, 90, 80, 8),
    ("kflip_hi", 48, 40, 40, 36, (5.5, 2.25), (_up(60.0), _up(45.0)), 0, 15, 15, 90, 80, 8),
    ("nyq_kept", 48, 40, 40, 36, (5.25, 2.25), (40.0, 36.0), 0, 24, 20, 90, 80, 8),
    ("nyq_dropped", 48, 40, 40, 36, (5.25, 2.25), (_up(40.0), _up(36.0)), 0, 23, 19, 90, 80, 8),
    ("kflip_lo_m", 48, 40, 40, 36, (5.5, 2.25), (60.0, 45.0), MIRROR, 32, 32, 140, 120, 8),
    ("kflip_hi_m", 48, 40, 40, 36, (5.5, 2.25), (_up(60.0), _up(45.0)), MIRROR, 31, 31, 140, 120, 8),
    ("mirror_cap", 48, 40, 40, 36, (5.5, 2.25), (40.0, 36.0), MIRROR, 48, 40, 140, 120, 8),
    ("mirror_cap_hi", 48, 40, 40, 36, (5.5, 2.25), (_up(40.0), _up(36.0)), MIRROR, 47, 39, 140, 120, 8),
    ("mcap_lo", 48, 40, 47, 39, (5.5, 2.25), (48.0, 40.0), MIRROR, 47, 39, 144, 120, 8),
    ("mcap_hi", 48, 40, 47, 39, (5.5, 2.25), (_up(48.0), _up(40.0)), MIRROR, 46, 38, 144, 120, 8),
    # ---- far origins
    ("far", 48, 40, 40, 36, FAR, (17.9, 12.2), 0, 24, 20, 90, 80, 8),
    ("far_m", 48, 40, 40, 36, FAR, (17.9, 12.2), MIRROR | U8, 48, 40, 140, 120, 8),
    ("far_refl_m", 48, 40, 40, 36, (-60.5, -47.25), (100.0, 90.0), MIRROR, 19, 16, 140, 120, 8),
    ("farther", 48, 40, 40, 36, FARTHER, (17.9, 12.2), 0, 24, 20, 90, 80, 8),
    ("farther_m", 48, 40, 40, 36, FARTHER, (17.9, 12.2), MIRROR, 48, 40, 140, 120, 8),
    # ---- the smallest lengths
    ("min2", 2, 2, 2, 2, (0.25, 0.5), (2.0, 2.0), 0, 1, 1, 4, 4, 8),
    ("min3", 3, 2, 2, 3, (0.25, 0.5), (3.0, 2.0), 0, 1, 1, 4, 5, 8),
    ("min2_m", 2, 2, 2, 2, (0.25, 0.5), (2.0, 2.0), MIRROR, 2, 2, 6, 6, 8),
)
NAMES = [r[0] for r in ROWS]

# next to ymax and ymax_m: the smallest column convolution the rules refuse, FFTUP_E_UNSUPPORTED_SIZE (two buffers of
# lpad_size(9720) = 10328 points are 165 248 bytes); (name, W, H, uW, uH, span, flags, the L_y it would need)
REJECTED = (
    ("ymax_over", 8, 4802, 8, 4803, (8.0, 4802.0), 0, 9720),
    ("ymax_m_over", 8, 3200, 8, 3205, (8.0, 3200.0), MIRROR, 9720),
)
LDS_POINTS = 9637                  # the largest L TK with 16 lpad_size(L TK) = 16 (L TK + L TK // 16 + 1) <= 160 KB: two fp32 complex buffers
TK_OF = {"tk4": 4, "tk4_trunc": 4, "tk2": 2, "tk1": 1, "tk2_bz": 2, "tk4_m": 4, "tk2_m": 2, "tk1_m": 1, "ymax": 1, "ymax_m": 1}
# the Bluestein forward length of tk2_bz's columns: the smallest 2,3,5,7-smooth length >= 2 * 1306 - 1.  It is above L_y = 1960 and
# above 9637 / 4: it, not L_y, moves the row from tiles of 4 to tiles of 2
TK2_BZ_FORWARD = 2625

# rows whose y axis is too long for a dense matrix in a test: the oracle of ymax is view_oracle.shift_planes (FFTs), every other
# row's is the two factors of the dense statement applied one after the other
SHIFT_ROWS = ("ymax",)
DENSE_LIMIT = 800                  # tests/test_view_edge_oracle.py forms dense matrices and runs the O(K M) chirp sums up to here


def row(name):
    return ROWS[NAMES.index(name)]


def mirror(r):
    return bool(r[7] & MIRROR)


def plan_flags(r, uint8=False):
    """the flags of the row's plan: FFTUP_FLAG_FUSE_U8_LOAD only on the run that uploads 8-bit pixels"""
    return (r[7] & ~U8) | (U8 if uint8 else 0)


def runs_u8(r):
    return bool(r[7] & U8)


def out_values(r):
    return 3 * r[3] * r[4]


def axes(r):
    """((N, M, origin, span) of x, the same of y)"""
    return (r[1], r[3], r[5][0], r[6][0]), (r[2], r[4], r[5][1], r[6][1])


def reduced(origin, N, is_mirror):
    """the origin modulo the period (N, or 2N of the reflected frame): fmod is exact in fp64"""
    return float(np.fmod(origin, 2.0 * N if is_mirror else float(N)))


def recomputed(r):
    """(kmax_x, kmax_y, L_x, L_y) by the oracles' rules"""
    (W, uW, _, sx), (H, uH, _, sy) = axes(r)
    if mirror(r):
        return Mo.table_kmax(W, uW, sx), Mo.table_kmax(H, uH, sy), Mo.conv_length(W, uW), Mo.conv_length(H, uH)
    return V.kmax(W, uW, sx), V.kmax(H, uH, sy), V.conv_length(W, uW), V.conv_length(H, uH)


def description_words(r):
    """what fftup_plan_describe must say of the row: both axes with kmax and L, and the tile width"""
    (W, uW, ox, sx), (H, uH, oy, sy) = axes(r)
    return ("rows %d->%d origin %.17g span %.17g (kmax %d, L=%d), columns %d->%d origin %.17g span %.17g (kmax %d, L=%d)"
            % (W, uW, ox, sx, r[8], r[10], H, uH, oy, sy, r[9], r[11]), "column tiles of %d)" % r[12])


def scale(r):
    """sc: the amplitude-preserving image is sc * R"""
    return r[3] * r[4] / (r[6][0] * r[6][1])


# ------------------------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def factors(N, M, origin, span, is_mirror):
    """the two factors of the dense statement of one axis, at the origin reduced modulo the period; computed once per
    (N, M, origin, span), shared by the tests, read-only.  y = Re(A (B x)): periodic A = E / N, B = F; mirror A = E, B = D"""
    o = reduced(origin, N, is_mirror)
    if is_mirror:
        A, B = Mo.mirror_factors(N, M, o, span)
    else:
        A, B = V.view_factors(N, M, o, span)
        A = A / N
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def axis_apply(x, axis, N, M, origin, span, is_mirror):
    """the view of one axis of x (fp64), along `axis`"""
    A, B = factors(N, M, float(origin), float(span), is_mirror)
    x = np.moveaxis(np.asarray(x, np.float64), axis, 0)
    y = np.real(np.tensordot(A, np.tensordot(B, x, axes=1), axes=1))
    return np.moveaxis(y, 0, axis)


def oracle_y(r, x):
    """planes [C][H][W] (fp64) -> the amplitude-preserving image [C][uH][uW] of the row's view"""
    (W, uW, ox, sx), (H, uH, oy, sy) = axes(r)
    if r[0] in SHIFT_ROWS:
        assert not mirror(r) and (W, H) == (uW, uH) and (sx, sy) == (W, H)
        return V.shift_planes(x, (ox, oy))
    return axis_apply(axis_apply(x, 1, H, uH, oy, sy, mirror(r)), 2, W, uW, ox, sx, mirror(r))


# ------------------------------------------------------------------------------------------------------------------- the probes
# pairs of rows whose kmax differs by one on both axes, and the input that tells them apart: a cosine at the frequency the _lo row
# keeps last.  Periodic: 0.5 + A cos(2 pi k n / N + 0.4), k = kmax of the _lo row (N / 2 for the nyq pair); mirror: the DCT-II basis
# vector 0.5 + A cos(pi k (2n + 1) / 2N), k the last cosine of the _lo row (N - 1 for mcap).  mirror_cap / mirror_cap_hi are no
# such pair: bin N of a reflected frame is identically zero, both keep the N - 1 cosines there are and have to give the same image.
PROBE_PAIRS = (("kflip_lo", "kflip_hi"), ("nyq_kept", "nyq_dropped"), ("kflip_lo_m", "kflip_hi_m"), ("mcap_lo", "mcap_hi"))
PROBE_AMPLITUDE = 0.3
# rows probed with the last cosine they keep without a neighbour in the table: the probe has to come back whole
PROBE_ALONE = ("mirror_cap", "mirror_cap_hi")


def last_kept(r, axis):
    """the frequency of the probe along `axis` (0: x, 1: y): the last bin (periodic) or cosine (mirror) the row keeps"""
    N, M, _, span = axes(r)[axis]
    return Mo.kmax(N, M, span) if mirror(r) else V.kmax(N, M, span)


def probe(r, axis, k):
    """planes [3][H][W] (fp32 values, as uploaded) that vary along `axis` alone"""
    N = axes(r)[axis][0]
    n = np.arange(N)
    line = 0.5 + PROBE_AMPLITUDE * (np.cos(np.pi * k * (2 * n + 1) / (2 * N)) if mirror(r) else np.cos(2 * np.pi * k * n / N + 0.4))
    planes = np.broadcast_to(line[None, :] if axis == 0 else line[:, None], (3, r[2], r[1]))
    return np.ascontiguousarray(planes.astype(np.float32))


# -------------------------------------------------------------------------------------------------------------- per-frame views
# ONE fftup_execute_device_views call per plan: the edge views of the plan's shape, in the table's words.  Frame i runs on lane
# i % FFTUP_STREAMS.  With three lanes the kflip pair are consecutive frames of lane 2 and its last (2 -> 5; mirror 5 -> 8), the nyq
# (mirror_cap) pair frames 3 -> 6, consecutive on lane 0 and its last; lane 1 ends on the farthest origin.  With one lane each pair is adjacent and
# the call ends on the _hi row of the kflip pair.  The tables of a lane's last frame are read back (last_on_lane).
FRAME_SHAPE = (48, 40, 40, 36)
FRAME_VIEWS = {False: ("step64", "step8", "kflip_lo", "nyq_kept", "far", "kflip_hi", "nyq_dropped", "farther"),
               True: ("step64_m", "step8_m", "far_refl_m", "mirror_cap", "far_m", "kflip_lo_m", "mirror_cap_hi", "farther_m", "kflip_hi_m")}
FRAME_VIEWS_ONE_LANE = {False: ("step64", "step8", "far", "farther", "nyq_kept", "nyq_dropped", "kflip_lo", "kflip_hi"),
                        True: ("step64_m", "step8_m", "far_refl_m", "far_m", "farther_m", "mirror_cap", "mirror_cap_hi", "kflip_lo_m", "kflip_hi_m")}


def frame_views(is_mirror, lanes):
    names = (FRAME_VIEWS if lanes == 3 else FRAME_VIEWS_ONE_LANE)[is_mirror]
    assert all(row(n)[1:5] == FRAME_SHAPE and mirror(row(n)) == is_mirror for n in names)
    return names


def last_on_lane(names, lanes):
    """{lane: index of the last frame that ran on it}"""
    return {k % lanes: k for k in range(len(names))}


def view_of(r):
    return (r[5], r[6])


# ------------------------------------------------------------------------------------------------------------------- kmax = 0
# (row, the axis of the planes [C][H][W] along which kmax = 0)
K0_ROWS = (("k0", 2), ("k0_m", 2), ("k0_y", 1))


def mean_view(r, axis):
    """the row with the origin of its other axis set to 0 -- there the view is the identity (step 1 from pixel 0), so every output
    line along `axis` is the mean of the input line at the same place"""
    origin = (r[5][0], 0.0) if axis == 2 else (0.0, r[5][1])
    return r[:5] + (origin,) + r[6:]
