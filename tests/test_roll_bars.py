"""CPU: where the fp32 bars of tests/test_gpu_roll.py come from (tests/roll_cases.py): the roll oracle run in complex64 against the
oracle run in complex128 over exactly the GPU tests' pairs and formats.  Each bar is four times the largest difference, computed
here and in the GPU test by the same function -- no figure is typed in.  This file checks what makes such bars meaningful: that
the two runs land in the same coarse cell everywhere, that the differences are rounding-sized, and that the accuracy of the
method stands far above them."""
import numpy as np

import roll_cases as K
import roll_oracle as R


def test_bars_are_four_times_the_measured_differences():
    worst, same_cell = K.measured_c64()
    bars = K.bars()
    for k in ("angle", "peak", "peak_coarse"):
        print("MEASURED roll complex64 oracle: largest |difference| in %s %.3g -> bar %.3g" % (k, worst[k], bars[k]))
        assert bars[k] == 4.0 * worst[k]
    assert same_cell
    # rounding-sized: the angle within a few fp32 steps of its largest value (0.35 rad: 3e-8 a step), the peaks of ones alike;
    # and nowhere near the method's own error (roll_oracle.ACCURACY_BAR), so a parity failure is never excused by the scene
    assert 0.0 < worst["angle"] <= 1e-6 and 0.0 < worst["peak"] <= 1e-6 and 0.0 < worst["peak_coarse"] <= 1e-6, worst
    assert bars["angle"] <= 1e-2 * min(R.ACCURACY_BAR.values())


def test_seven_pairs_per_case_and_every_format():
    assert len(R.GPU_CASES) == 4 and sorted(K.FORMATS) == ["planar_f16", "planar_f32", "rgb8"]
    for case in R.GPU_CASES:
        ref, moved, true = K.scene(case)
        assert len(moved) == 7 and list(true) == R.ANGLES and ref.dtype == np.uint8 and ref.shape == (case[1], case[0], 3)
        for fmt in K.FORMATS:
            assert len(K.oracle(case, fmt)) == 7


def test_gaps_of_the_oracle():
    """the parity test compares coarse cells where the oracle's best and second-best differ by 1e-3 of the peak or more, and accepts
    the neighbouring cell below that; with these scenes every pair is above it (the smallest: printed)"""
    for case, cid in zip(R.GPU_CASES, K.CASE_IDS):
        for fmt in K.FORMATS:
            gaps = [o["gap"] / o["peak_coarse"] for o in K.oracle(case, fmt)]
            print("MEASURED roll oracle %s %s: smallest gap %.3g of the peak" % (cid, fmt, min(gaps)))
            assert min(gaps) >= K.GAP_FOR_SAME_CELL
