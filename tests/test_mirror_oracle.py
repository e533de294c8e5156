"""CPU: the mathematics of FFTUP_FLAG_MIRROR (include/fftup.h) as tests/mirror_oracle.py states it, in fp64 to 1e-12 -- the cosine
form against the periodic view formula of the 2N-periodic even extension, constants, the DCT modes at centre alignment, the
border of a ramp, and the reordering that lets the kernels transform N points instead of 2N."""
import numpy as np
import pytest

import dct_oracle as D
import downscale_oracle as DS
import mirror_oracle as Mo
import view_oracle as V

SHAPES = [(12, 30, 1.3, 5.5), (9, 14, -2.25, 9), (16, 10, 0, 16), (15, 7, 3, 12), (10, 25, -4, 19), (8, 8, 0, 8)]


@pytest.mark.parametrize("N,M,origin,span", SHAPES)
def test_cosine_form_is_the_view_of_the_even_extension(N, M, origin, span):
    A, B = Mo.mirror_matrix(N, M, origin, span), Mo.mirror_matrix_ext(N, M, origin, span)
    assert np.abs(B.imag).max() <= 1e-12
    assert np.abs(A - B.real).max() <= 1e-12
    # ... and applied to a frame: view_matrix(2N, ...) on the extended samples
    x = np.random.default_rng(N + M).random(N)
    assert np.abs(A @ x - (V.view_matrix(2 * N, M, origin, span) @ Mo.extend(x)).real).max() <= 1e-12
    # the bin the cap at N - 1 drops is identically zero
    assert abs(np.fft.fft(Mo.extend(x))[N]) <= 1e-12
    assert Mo.kmax(N, M, span) == min(N - 1, V.kmax(2 * N, M, span))


@pytest.mark.parametrize("N,M,origin,span", SHAPES)
def test_constants_stay_constant(N, M, origin, span):
    assert np.abs(Mo.mirror_matrix(N, M, origin, span).sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("N,M", [(12, 30), (16, 24), (14, 14), (20, 10), (18, 12)])
def test_centre_alignment_is_the_dct_mode(N, M):
    A = Mo.mirror_matrix(N, M, Mo.centre_origin(N, M), N)
    want = D.resample_matrix(N, M) if M >= N else DS.dct_down_matrix(N, M)
    assert np.abs(A - want).max() <= 1e-12


def test_ramp_border_overshoot():
    """32 -> 64, centre-aligned: the periodic interpolant rings at the jump between the last and the first sample, the mirror one
    has no jump to ring at"""
    N, M = 32, 64
    x = np.linspace(0, 1, N)
    o = Mo.centre_origin(N, M)
    per = V.view_1d(x, M, o, N).real
    mir = Mo.mirror_matrix(N, M, o, N) @ x
    assert per.min() < -0.1 and per.max() > 1.1
    assert mir.min() > -0.01 and mir.max() < 1.01
    assert abs(per.max() - 1.115) < 1e-3 and abs(mir.max() - 1.0044) < 1e-4


@pytest.mark.parametrize("N", [12, 9])
def test_reordering_identities(N):
    rng = np.random.default_rng(N)
    x = rng.random(N)
    z = rng.random(N) + 1j * rng.random(N)
    v = Mo.reorder(np.arange(N))
    assert sorted(v) == list(range(N)) and list(v[:(N + 1) // 2]) == list(range(0, N, 2)) and list(v[::-1][:N // 2]) == list(range(1, N, 2))
    assert np.abs(Mo.dct2_reordered_real(x) - Mo.dct2(x)).max() <= 1e-12
    assert np.abs(Mo.dct2_reordered_complex(z) - Mo.dct2(z)).max() <= 1e-12
    assert np.abs(Mo.dct2_reordered_complex(x) - Mo.dct2(x)).max() <= 1e-12
    # the factor the kernels carry: the spectrum of the extension is X~[f] = 2 exp(i pi f / 2N) C[|f|], and 0 at |f| = N
    Xe = np.fft.fft(Mo.extend(x))
    f = np.arange(N)
    assert np.abs(Xe[:N] - 2 * np.exp(1j * np.pi * f / (2 * N)) * Mo.dct2(x)).max() <= 1e-12
    assert np.abs(Xe[2 * N - f[1:]] - 2 * np.exp(-1j * np.pi * f[1:] / (2 * N)) * Mo.dct2(x)[1:]).max() <= 1e-12


def test_planes_are_the_separable_map():
    x = np.random.default_rng(3).random((3, 9, 12))
    y = Mo.mirror_planes(x, 30, 14, (1.3, -2.25), (5.5, 9.0))
    want = np.einsum("ab,cbd,ed->cae", Mo.mirror_matrix(9, 14, -2.25, 9.0), x, Mo.mirror_matrix(12, 30, 1.3, 5.5))
    assert np.abs(y - want).max() <= 1e-12
    assert np.abs(Mo.mirror_R(x, 30, 14, (1.3, -2.25), (5.5, 9.0)) - y * 5.5 * 9.0 / (30 * 14)).max() <= 1e-15
