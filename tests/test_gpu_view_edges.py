"""GPU: the view and mirror kernels (csrc/kernels_view.hpp, kernels_mirror.hpp, kernels_view_tables.hpp) at the edges of their
geometry -- the rows of tests/view_edge_cases.py: column tiles of 4, 2 and 1 with a partial last tile, the largest column
convolution, the closed step bounds 1/64 and 8, kmax = 0, the floor in kmax on either side of an integer quotient, origins 1e9
pixels away and the smallest lengths -- against the fp64 oracles (tests/view_oracle.py, tests/mirror_oracle.py) at the bars of
tests/paritylib.py, unchanged.  tests/test_view_edge_oracle.py proves on the CPU every literal of the table and everything the
oracle is taken for here.

Every run asserts from the plan's description the kmax, L and tile width of its row: a planner that moves a row off its edge fails
the test instead of passing it in the comfortable middle.  A natural frame has next to no energy in the last bin a view keeps, so
the parity bars alone would not see a plan that is one bin off: the rows around a floor are run on the cosine of that bin as well.

Measured on an MI355X (profiles/view_edges_measured.txt), the largest figure of any row beside its bar.  -p 0: pre_l2 2.8e-7 (2e-6),
pre_max 6.4e-7 (1e-5), out_l2 5.6e-7 (5e-6), out_max 1.5e-6 (2e-5) -- the tall rows (L_y up to 9604) no worse than the short ones; the
probes 1.9e-7 and 4.4e-7; kmax = 0: the mean within 1.8e-7, a line's spread 2.1e-7.  -p 2: R never beyond one ulp, differing R 0.046 %
(1 %), out_l2 6.7e-5 (3.5e-4), out_max 2.0e-3 (8e-3), differing output 0.19 % (2 %).  Per-frame views: the bytes of fresh plans;
device tables within 0.46 of an fp32 step.

-p 2 on an output of a few dozen values: the two fraction bars mean nothing there (tests/test_gpu_family_sweep.py); the rows
smaller than the smallest view case that runs -p 2 today run -p 0 in the parametrized test and -p 2 in one pooled test."""
import functools

import numpy as np
import pytest

import mirror_oracle as Mo
import paritylib as P
import test_gpu_view as VW
import view_edge_cases as EC
import view_oracle as V
from devimage import PLANAR
from test_gpu_view_frames import _against_fresh, _fresh, _table_bars, _views_run

pytestmark = pytest.mark.gpu

TINY = min(3 * c[2] * c[3] for c in VW.VIEWS + VW.THIN)


def _names(r):
    W, H = r[1], r[2]
    if EC.mirror(r):
        return ["row_r2c_mirror" + ("" if P.smooth(W) else "_bz"), "col_view_mirror" + ("" if P.smooth(H) else "_bz"), "row_view_c2r_mirror", "sharpen"]
    return ["row_r2c_odd" + ("" if P.smooth(W) else "_bz"), "col_view" + ("" if P.smooth(H) else "_bz"), "row_view_c2r", "sharpen"]


def _describes(r, desc):
    for words in EC.description_words(r):
        assert words in desc, (r[0], words, desc)
    assert ("mirror" in desc) == EC.mirror(r)


@functools.lru_cache(maxsize=None)
def _inputs(W, H, precision, uint8, seed):
    """(rgb, planes, x) of paritylib.inputs, made once per shape and shared; read-only"""
    got = P.inputs(W, H, precision, uint8, seed)
    for a in got:
        if a is not None:
            a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def _oracle(name, precision, uint8):
    """the oracle's image of the row's frame: the tall ones are the module's only multi-second cost"""
    r = EC.row(name)
    y = EC.oracle_y(r, _inputs(r[1], r[2], precision, uint8, 900 + r[1] + r[2])[2])
    y.setflags(write=False)
    return y


def _run(r, precision, uint8=False, rgb=None, planes=None):
    import vkresample_amd as v
    with v.Upscaler.view(r[1], r[2], r[3], r[4], r[5], r[6], precision, P.SHARPEN, 0, EC.plan_flags(r, uint8)) as up:
        pre, out = P.run_uploaded(up, rgb, planes)
        names, desc = up.kernel_names, up.description
        assert (up.out_width, up.out_height) == (r[3], r[4])
        assert not up.tuned and not up.u8_store and up.num_kernels == 4
    assert names == _names(r), (r[0], names)
    _describes(r, desc)
    return pre, out


def _check(r, precision, uint8, pooled=None):
    rgb, planes, _ = _inputs(r[1], r[2], precision, uint8, 900 + r[1] + r[2])
    pre, out = _run(r, precision, uint8, rgb, planes)
    y = _oracle(r[0], precision, uint8)
    assert pre.shape == y.shape == (3, r[4], r[3])
    P.assert_parity("view edge %s p%d u8%d" % (r[0], precision, uint8), precision, pre, out, y, EC.scale(r), V.effective_factor(r[3], r[4], r[6]), pooled=pooled)
    return pre


def _tiny(r):
    return EC.out_values(r) < TINY


PARITY = [pytest.param(r[0], p, u8, id="%s-p%d%s" % (r[0], p, "-u8" if u8 else ""))
          for r in EC.ROWS for p in (0, 2) for u8 in ((False, True) if EC.runs_u8(r) or _tiny(r) else (False,)) if not (p == 2 and _tiny(r))]


@pytest.mark.parametrize("name,precision,uint8", PARITY)
def test_edge_parity(name, precision, uint8):
    _check(EC.row(name), precision, uint8)


def test_tiny_rows_at_p2_pooled():
    """k0, k0_y, k0_m, min2, min3, min2_m at -p 2, planar and 8-bit input: the per-case bars inside assert_parity, the two fraction
    bars on all of them together"""
    rows = [r for r in EC.ROWS if _tiny(r)]
    assert sorted(r[0] for r in rows) == ["k0", "k0_m", "k0_y", "min2", "min2_m", "min3"]
    acc = []
    for r in rows:
        for uint8 in (False, True):
            _check(r, 2, uint8, pooled=acc)
    P.pooled_fraction_bars("view edge tiny rows pooled p2 (%d runs)" % len(acc), acc)


@pytest.mark.parametrize("name,W,H,uW,uH,span,flags,Ly", EC.REJECTED, ids=[c[0] for c in EC.REJECTED])
def test_one_smooth_length_past_the_largest_column_is_refused(name, W, H, uW, uH, span, flags, Ly):
    import vkresample_amd as v
    for precision in (0, 2):
        with pytest.raises(v.FftupError) as e:
            v.Upscaler.view(W, H, uW, uH, (0.0, 0.0), span, precision, flags=flags)
        assert e.value.code == 2 and "columns" in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------------ the floor in kmax, kmax = 0
@pytest.mark.parametrize("name", [n for pair in EC.PROBE_PAIRS for n in pair] + list(EC.PROBE_ALONE))
def test_the_last_bin_is_kept_or_dropped(name):
    """the cosine at the last frequency the pair's _lo row keeps, along x and along y, through the row's plan: sc * pre within the
    fp32 bars of the oracle, which differs between the two rows of a pair by 0.16 and more (tests/test_view_edge_oracle.py)"""
    r = EC.row(name)
    lo = next((EC.row(a) for a, b in EC.PROBE_PAIRS if name in (a, b)), r)
    sc = EC.scale(r)
    for axis in (0, 1):
        k = EC.last_kept(lo, axis)
        planes = EC.probe(r, axis, k)
        pre, _ = _run(r, 0, planes=planes)
        want = EC.oracle_y(r, planes.astype(np.float64))
        P.measured("view edge probe %s axis %d k=%d" % (name, axis, k), l2=P.rel_l2(sc * pre, want), max_err=np.abs(sc * pre - want).max(),
                   swing=want.max() - want.min())
        assert P.rel_l2(sc * pre, want) <= P.FP32_PRE_L2
        assert np.abs(sc * pre - want).max() <= P.FP32_PRE_MAX


@pytest.mark.parametrize("name,axis", EC.K0_ROWS)
def test_kmax_zero_is_the_mean(name, axis):
    """one spectrum column (k0, k0_m) or one spectrum row (k0_y): every output row (column) of sc * pre is constant, and with the
    quarter-pixel shift of the other axis taken out (view_edge_cases.mean_view) it is the mean of its input row (column) -- no
    oracle between the kernel and the statement"""
    r = EC.row(name)
    _, planes, x = _inputs(r[1], r[2], 0, False, 900 + r[1] + r[2])
    spread = np.ptp(EC.scale(r) * _run(r, 0, planes=planes)[0], axis=axis).max()
    m = EC.mean_view(r, axis)
    got = EC.scale(m) * _run(m, 0, planes=planes)[0]
    want = np.broadcast_to(x.mean(axis=axis, keepdims=True), got.shape)
    P.measured("view edge %s mean" % name, max_err=np.abs(got - want).max(), spread=max(spread, np.ptp(got, axis=axis).max()))
    assert np.abs(got - want).max() <= P.FP32_PRE_MAX
    assert spread <= P.FP32_PRE_MAX


# ------------------------------------------------------------------------------------------------------------- per-frame views
def _frames(is_mirror, precision):
    W, H = EC.FRAME_SHAPE[:2]
    n = len(EC.FRAME_VIEWS[is_mirror])
    return [_inputs(W, H, precision, False, 700 + k)[1:] for k in range(n)]


@pytest.mark.parametrize("lanes", [3, 1])
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("is_mirror", [False, True], ids=["periodic", "mirror"])
def test_edge_views_in_one_call(is_mirror, precision, lanes, monkeypatch):
    """ONE fftup_execute_device_views call on one plan whose frames are the shape's edge views (k_view_tables gets its kmax from
    frame_view, not from the host tables): every frame against the oracle and against a fresh plan; the tables of each lane's last
    frame, read back, have the row's kmax and lie within one fp32 rounding step of the long double tables"""
    import vkresample_amd as v
    monkeypatch.setenv("FFTUP_STREAMS", str(lanes))
    names = EC.frame_views(is_mirror, lanes)
    rows = [EC.row(n) for n in names]
    W, H, uW, uH = EC.FRAME_SHAPE
    flags = v.FLAG_MIRROR if is_mirror else 0
    frames = _frames(is_mirror, precision)
    with v.Upscaler.view(W, H, uW, uH, (0.0, 0.0), (float(W), float(H)), precision, 0.2, 0, flags) as up:
        outs, pre = _views_run(up, [f[0] for f in frames], PLANAR, [EC.view_of(r) for r in rows])
        tables = {}
        if precision == 0:
            for lane, k in EC.last_on_lane(names, lanes).items():
                tables[k] = [up.download_view_tables(lane, axis) for axis in (0, 1)]
    for k, r in enumerate(rows):
        tag = "edge views %s p%d lanes %d frame %d %s" % ("mirror" if is_mirror else "periodic", precision, lanes, k, r[0])
        P.assert_parity(tag, precision, pre if k == len(rows) - 1 else None, outs[k], EC.oracle_y(r, frames[k][1]), EC.scale(r),
                        V.effective_factor(uW, uH, r[6]))
        _against_fresh(tag, precision, outs[k], _fresh(EC.FRAME_SHAPE, EC.view_of(r), precision, flags, frames[k][0], PLANAR))
    assert precision != 0 or len(tables) == lanes
    for k, got in tables.items():
        r = rows[k]
        for axis, (N, M, origin, span) in enumerate(EC.axes(r)):
            assert got[axis][0] == r[8 + axis], (r[0], axis, got[axis][0])
            _table_bars("edge tables %s lanes %d %s %s" % ("mirror" if is_mirror else "periodic", lanes, r[0], "xy"[axis]), got[axis],
                        (Mo.chirp_tables if is_mirror else V.chirp_tables)(N, M, origin, span))


@pytest.mark.parametrize("is_mirror", [False, True], ids=["periodic", "mirror"])
def test_set_view_walks_the_edges_with_the_bytes_of_fresh_plans(is_mirror):
    """fftup_plan_set_view through the same edge views on one plan: planes, 8-bit output, description and byte counts of a plan
    created with the view"""
    import vkresample_amd as v
    W, H, uW, uH = EC.FRAME_SHAPE
    flags = v.FLAG_MIRROR if is_mirror else 0
    rgb = P.frame(W, H, seed=9)
    rows = [EC.row(n) for n in EC.FRAME_VIEWS[is_mirror]]
    for precision in (0, 2):
        fresh = []
        for r in rows:
            with v.Upscaler.view(W, H, uW, uH, r[5], r[6], precision, flags=flags) as up:
                up.upload_rgb8(rgb)
                up.execute(1)
                fresh.append((up.download_planar().tobytes(), up.download_rgb8().tobytes(), up.description, up.kernel_min_bytes))
                _describes(r, up.description)
        assert len({f[0] for f in fresh}) >= len(rows) - 1                # (mirror_cap and mirror_cap_hi may round to the same tables)
        with v.Upscaler.view(W, H, uW, uH, (0.0, 0.0), (float(W), float(H)), precision, flags=flags) as up:
            up.upload_rgb8(rgb)
            for r, want in zip(rows, fresh):
                up.set_view(r[5], r[6])
                up.execute(1)
                assert up.download_planar().tobytes() == want[0], (precision, r[0])
                assert up.download_rgb8().tobytes() == want[1], (precision, r[0])
                assert (up.description, up.kernel_min_bytes) == want[2:], (precision, r[0])
