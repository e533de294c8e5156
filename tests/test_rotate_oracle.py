"""CPU: the oracle of the rotation by three shears (tests/rotate_oracle.py, the definition of include/fftup.h in fp64) held to known
answers, so that the GPU tests compare the kernels with something that is itself pinned:
  (a) a rotated off-centre anisotropic Gaussian is the analytically rotated Gaussian within 1e-8 (measured: at most 4.0e-9), and
      the opposite sign is off by 0.5 or more -- which pins the direction;
  (b) theta = 0 is the identity within 1e-14;
  (c) on odd x odd frames rotate(theta) then rotate(-theta) returns 8-bit noise within 1e-13 relative L2 (measured: at most 7e-16):
      every shear is a unitary phase ramp there;
  (d) on 64 x 32 the same round trip does NOT return the input (more than 1e-3; measured 6e-2 and more): the Nyquist rule of even
      lengths is real but not unitary -- nobody "fixes" it silently;
  (e) a rotation about another centre than the frame's is the definition, checked directly."""
import numpy as np
import pytest

import rotate_oracle as R


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


@pytest.mark.parametrize("theta", [0.1, -0.4, 0.9])
@pytest.mark.parametrize("size", [(96, 80), (64, 48)])
def test_rotated_gaussian_is_the_analytic_rotation(size, theta):
    W, H = size
    c = R.centre_of(W, H)
    got = R.rotate(R.gaussian(W, H, c), theta)
    err = float(np.abs(got - R.gaussian(W, H, c, angle=theta)).max())
    wrong = float(np.abs(got - R.gaussian(W, H, c, angle=-theta)).max())
    print("MEASURED gaussian %dx%d theta %+.1f: max|err| %.3g, against the opposite sign %.3g" % (W, H, theta, err, wrong))
    assert err <= 1e-8
    assert wrong >= 0.5


@pytest.mark.parametrize("size", R.CASES[:4])
def test_zero_angle_is_the_identity(size):
    W, H = size
    x = R.planes_of(R.noise_u8(W, H, 1))
    assert float(np.abs(R.rotate(x, 0.0) - x).max()) <= 1e-14


@pytest.mark.parametrize("theta", [0.02, -0.3, 0.7, 1.5])
@pytest.mark.parametrize("size", [(45, 21), (75, 45)])
def test_round_trip_on_odd_sizes(size, theta):
    W, H = size
    x = R.planes_of(R.noise_u8(W, H, 2))
    back = R.rotate(R.rotate(x, theta), -theta)
    err = rel_l2(back, x)
    print("MEASURED round trip %dx%d theta %+.2f: rel L2 %.3g" % (W, H, theta, err))
    assert err <= 1e-13


@pytest.mark.parametrize("theta", [0.02, -0.3, 0.7, 1.5])
def test_round_trip_on_even_sizes_loses_the_nyquist_bins(theta):
    x = R.planes_of(R.noise_u8(64, 32, 3))
    err = rel_l2(R.rotate(R.rotate(x, theta), -theta), x)
    print("MEASURED round trip 64x32 theta %+.2f: rel L2 %.3g" % (theta, err))
    assert err > 1e-3


def _dft_shift(line, delta):
    """one line moved by delta, written out bin by bin from the header's formula"""
    n = len(line)
    X = np.array([sum(line[m] * np.exp(-2j * np.pi * k * m / n) for m in range(n)) for k in range(n)])
    Y = np.zeros(n, dtype=np.complex128)
    for k in range(n):
        f = k if 2 * k < n else k - n
        Y[k] = X[k] * (np.cos(np.pi * delta) if 2 * k == n else np.exp(-2j * np.pi * f * delta / n))
    return np.real(np.array([sum(Y[k] * np.exp(2j * np.pi * k * m / n) for k in range(n)) for m in range(n)]) / n)


def test_rotation_about_another_centre_is_the_definition():
    W, H, theta, cx, cy = 12, 10, 0.35, 3.25, 6.5
    x = R.planes_of(R.noise_u8(W, H, 4))[0]
    a, b = -np.tan(theta / 2), np.sin(theta)
    t = np.stack([_dft_shift(x[y], a * (y - cy)) for y in range(H)])
    t = np.stack([_dft_shift(t[:, c], b * (c - cx)) for c in range(W)], axis=1)
    t = np.stack([_dft_shift(t[y], a * (y - cy)) for y in range(H)])
    assert float(np.abs(R.rotate(x, theta, (cx, cy)) - t).max()) <= 1e-12
    assert float(np.abs(R.rotate(x, theta) - t).max()) > 1e-2            # (the frame's own centre gives another image)
    # ... and the Gaussian again, turned about a centre off the frame's: the meaning of the centre
    W, H, c = 96, 80, (40.0, 44.5)
    got = R.rotate(R.gaussian(W, H, c), -0.4, c)
    assert float(np.abs(got - R.gaussian(W, H, c, angle=-0.4)).max()) <= 1e-8
