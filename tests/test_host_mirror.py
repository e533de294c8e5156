"""CPU: FFTUP_FLAG_MIRROR (include/fftup.h) without a device -- the flag is in the header, the binding and the CLI's help; the rules
of such a plan are arithmetic decided before any device access (through the device-free planner, tests/plan_driver.py, and through
the library itself); the geometry comes back with the convolution lengths of the doubled periods; the host tables
(csrc/mirror_tables.hpp) agree with a longdouble restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

import mirror_oracle as Mo
import plan_driver
from family_sweep_cases import smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRROR, ANY, DCT = 4096, 1024, 256


def _conv(N, M):
    L = 2 * N + M
    while not smooth(L):
        L += 1
    return L


def test_flag_in_header_binding_and_help():
    import vkresample_amd as v
    src = open(os.path.join(ROOT, "include", "fftup.h")).read()
    assert re.search(r"FFTUP_FLAG_MIRROR\s*=\s*4096u", src) and v.FLAG_MIRROR == MIRROR
    # the mathematics, as the issue fixes it
    for line in ("C[k]  = sum_n x[n] cos(pi k (2n+1) / 2N)", "kmax  = min(N - 1, floor((double)(N M) / max(span, (double)M)))",
                 "y[m]  = C[0]/N + (2/N) sum_{k=1..kmax} C[k] cos(pi k (2 t_m + 1) / 2N)", "x~[n] = x[2N-1-n] for N <= n < 2N"):
        assert line in src, line
    assert re.search(r"\bFFTUP_ABI_VERSION\s*=\s*2\b", src)
    main = open(os.path.join(ROOT, "vkresample_amd", "csrc", "cli", "vkresample_main.cpp")).read()
    assert '"-mirror"' in main and "-mirror needs a view" in main and "\t-mirror:" in main


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("mirror_plan")
    exe = plan_driver.build(d)
    return lambda lines: plan_driver.run(exe, d, lines)


def _view(W, H, uW, uH, origin, span, flags, precision=0):
    return plan_driver.request_line("view", W, H, 1.0, precision, flags, 0, (uW, uH), 0, tuple(origin) + tuple(span))


ACCEPTED = [(1920, 1080, 3840, 2160, (-0.25, -0.25), (1920.0, 1080.0), MIRROR),
            (2048, 16, 4096, 16, (0.0, 0.0), (2048.0, 16.0), MIRROR),
            (46, 22, 70, 30, (0.37, -0.5), (46.0, 22.0), MIRROR | ANY),
            (1366, 768, 1920, 1080, (-0.144, -0.144), (1366.0, 768.0), MIRROR | ANY),
            (48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), MIRROR), (45, 21, 64, 30, (-3.25, 2.5), (61.5, 33.3), MIRROR),
            (16, 256, 32, 512, (0.0, 0.0), (16.0, 256.0), MIRROR)]


def test_accepted_sizes_and_their_geometry(planner):
    lds_max = plan_driver.golden_rows("plan_geometry.json")["device"]["lds_bytes"]
    lines = []
    for case in ACCEPTED:
        for p in (0, 2):
            lines += [_view(*case, precision=p), _view(*case[:6], case[6] & ~MIRROR, precision=p)]
    out = planner(lines)
    for i, case in enumerate(c for c in ACCEPTED for _ in (0, 2)):
        W, H, uW, uH, origin, span, flags = case
        assert not out[2 * i].startswith("error"), (case, out[2 * i])
        g, per = plan_driver.fields(out[2 * i]), plan_driver.fields(out[2 * i + 1])
        Lx, Ly = _conv(W, uW), _conv(H, uH)
        assert g["viewL"] == "%d,%d" % (Lx, Ly) and g["view"] == "1" and g["family"] == per["family"], (case, g)
        assert Lx <= 8192 and Lx >= 2 * W + uW and Ly >= 2 * H + uH
        # the forward transforms keep the input's lengths; the buffers those of the worst case
        assert g["planW"].startswith("%d:" % W) and g["planH"].startswith("%d:" % H) and g["ncols"] == str(W // 2 + 1)
        assert g["bzL"] == per["bzL"] and (g["bz"] == "1") == (not (smooth(W) and smooth(H)))
        tk = int(g["TK"])
        assert tk in (1, 2, 4, 8) and int(g["ldsCol"]) <= lds_max and int(g["ldsRowI"]) <= lds_max
        assert int(g["ldsRowI"]) >= 16 * Lx and int(g["ldsCol"]) >= 16 * Ly * tk
        assert int(g["thrUW"]) == min(1024, max(64, -(-(Lx // 8) // 64) * 64))
        # the periodic plan of the same request: shorter convolutions, nothing else about the request differs
        assert per["viewL"] != g["viewL"] and [per[k] for k in ("W", "H", "uW", "uH", "half", "upsq")] == [g[k] for k in ("W", "H", "uW", "uH", "half", "upsq")]
    assert plan_driver.fields(out[0])["viewL"] == "7680,4320" and plan_driver.fields(out[4])["viewL"].startswith("8192,")


REFUSED = [
    # (request, code, a word of the message)
    (_view(2049, 16, 4096, 16, (0, 0), (2049, 16), MIRROR | ANY), 2, "convolution"),                 # 2 * 2049 + 4096 > 8192
    (_view(2048, 16, 4097, 16, (0, 0), (2048, 16), MIRROR), 2, "convolution"),
    (_view(46, 22, 70, 30, (0.37, -0.5), (46, 22), MIRROR), 2, "FFTUP_FLAG_ANY_SIZE"),
    (_view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), MIRROR, precision=1), 3, "-p 0 and -p 2"),
    (_view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), MIRROR | DCT), 2, "FFTUP_FLAG_DCT"),
    (plan_driver.request_line("create", 64, 48, 2.0, 0, MIRROR), 1, "fftup_plan_create_view only"),
    (plan_driver.request_line("create", 64, 48, 2.0, 1, MIRROR | DCT), 1, "fftup_plan_create_view only"),
    (plan_driver.request_line("size", 50, 32, 1.0, 0, MIRROR, 0, (32, 50), 1), 1, "fftup_plan_create_view only"),
    (_view(64, 4096, 64, 4096, (0, 0), (64, 4096), MIRROR), 2, "columns"),                           # L_y = 12288: two buffers do not fit
    (_view(64, 3072, 64, 4096, (0, 0), (64, 3072), MIRROR), 2, "columns"),                           # 10240 points: 163 840 bytes + padding
    (_view(48, 40, 40, 36, (0, 0), (400.0, 12.2), MIRROR), 1, "span_x"),                            # the step rule is the view plans'
    (_view(8400, 8, 64, 8, (0, 0), (512, 8), MIRROR), 2, "8192"),
]


def test_refusals_with_code_and_message(planner):
    out = planner([r[0] for r in REFUSED])
    for (req, code, word), line in zip(REFUSED, out):
        assert line.startswith("error %d " % code) and word in line, (req, line)


def test_the_library_decides_the_same_before_any_device_access():
    """through the C ABI: the refusals come back with or without a GPU; an accepted request gets as far as the device"""
    import vkresample_amd as v
    bad = [(lambda: v.Upscaler(64, 48, 2.0, 0, 0.2, 0, MIRROR), 1, "fftup_plan_create_view only"),
           (lambda: v.Upscaler.to_size(50, 32, 32, 50, flags=MIRROR), 1, "fftup_plan_create_view only"),
           (lambda: v.Upscaler.view(2049, 16, 4096, 16, (0, 0), (2049, 16), flags=MIRROR | ANY), 2, "convolution"),
           (lambda: v.Upscaler.view(46, 22, 70, 30, (0.37, -0.5), (46, 22), flags=MIRROR), 2, "FFTUP_FLAG_ANY_SIZE"),
           (lambda: v.Upscaler.view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), 1, flags=MIRROR), 3, "-p 0 and -p 2"),
           (lambda: v.Upscaler.view(48, 40, 40, 36, (10.3, 7.75), (17.9, 12.2), flags=MIRROR | DCT), 2, "FFTUP_FLAG_DCT"),
           (lambda: v.Upscaler.view(64, 4096, 64, 4096, (0, 0), (64, 4096), flags=MIRROR), 2, "columns")]
    for make, code, word in bad:
        with pytest.raises(v.FftupError) as e:
            make()
        assert e.value.code == code and word in str(e.value), str(e.value)
    for W, H, uW, uH, origin, span, flags in ACCEPTED:
        try:
            with v.Upscaler.view(W, H, uW, uH, origin, span, flags=flags) as up:
                assert all("_mirror" in n for n in up.kernel_names[:3]) and "mirror" in up.description
        except v.FftupError as e:
            assert e.code == 4 and v.device_count() == 0, str(e)


@pytest.fixture(scope="module")
def tables_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mirror") / "mirror_tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "vkresample_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mirror", "mirror_tables_driver.cpp"), "-o", exe])
    return exe


def _longdouble_tables(N, M, origin, span):
    """pre [K], post [M], c [d = -(K-1) .. M-1] of the axis with period 2N aimed at origin + 1/2, stated here on their own:
    pre[j] = g exp(i pi (f (2 origin + 1) + s j^2) / 2N), post[m] = (s / 2N) exp(i pi (s m^2 - 2 kmax m s) / 2N), c[d] = exp(-i pi s d^2 / 2N)"""
    ld = np.longdouble
    pi = ld("3.141592653589793238462643383279502884")
    k = min(N, int(np.floor(float(N * M) / max(float(span), float(M)))))
    K = 2 * k + 1
    n2, s = ld(2 * N), ld(span) / ld(M)
    o = np.fmod(ld(origin) + ld(0.5), n2)

    def e(x):
        r = np.fmod(x, ld(2))
        return np.cos(pi * r) + 1j * np.sin(pi * r)

    j = np.arange(K).astype(ld)
    f = j - k
    g = np.where(np.abs(np.arange(K) - k) == N, ld(0.5), ld(1))
    pre = g * e(np.fmod(2 * f * o / n2, ld(2)) + np.fmod(s * j * j / n2, ld(2)))
    m = np.arange(M).astype(ld)
    post = (s / n2) * e(np.fmod(s * m * m / n2, ld(2)) - np.fmod(2 * k * m * s / n2, ld(2)))
    d = np.arange(-(K - 1), M).astype(ld)
    return k, pre, post, e(-np.fmod(s * d * d / n2, ld(2)))


@pytest.mark.parametrize("N,M,origin,span", [(48, 40, 10.3, 17.9), (45, 64, -3.25, 61.5), (46, 70, 0.37, 46.0), (50, 25, 0.5, 50.0),
                                             (2048, 4096, -0.25, 2048.0), (1920, 3840, 480.0 + 1e6 * 3840, 960.0), (1080, 1080, -0.25, 8640.0)])
def test_host_tables_against_longdouble_numpy(tables_driver, N, M, origin, span):
    out = subprocess.run([tables_driver, str(N), str(M), repr(origin), repr(span)], capture_output=True, text=True, check=True).stdout.split("\n")
    kmax, L, ncols = (int(t) for t in out[0].split())
    vals = np.array([[float(t) for t in line.split()] for line in out[1:] if line])
    K = 2 * kmax + 1
    assert vals.shape == (K + M + L, 2)
    cplx = vals[:, 0] + 1j * vals[:, 1]
    pre, post, bhat = cplx[:K], cplx[K:K + M], cplx[K + M:]
    k, opre, opost, oc = _longdouble_tables(N, M, origin, span)
    # kmax may be N (the zero bin, weight 1/2); the cosines the frame needs stop at N - 1
    assert kmax == k and min(kmax, N - 1) == Mo.kmax(N, M, span)
    assert ncols == (kmax + 1 if kmax < N // 2 else N // 2 + 1)
    assert L == _conv(N, M) and L >= K + M - 1
    eps = 2.0 ** -24
    assert np.abs(pre - opre.astype(np.complex128)).max() <= 1.01 * eps
    assert np.abs(post - opost.astype(np.complex128)).max() <= 1.01 * eps * float(span) / M / (2 * N)
    cw = np.zeros(L, np.complex128)
    cw[np.arange(-(K - 1), M) % L] = oc.astype(np.complex128)
    ref = np.fft.ifft(cw)
    assert np.abs(bhat - ref).max() <= 1.01 * eps * max(np.abs(ref).max(), 1e-30) + 1e-12
    # and the tables ARE the map: y[m] = post[m] sum_j (2 C[|j - kmax|]) pre[j] c[m - j] is the oracle's row (fp64, small sizes)
    if N <= 64:
        x = np.random.default_rng(N).random(N)
        Cc = np.append(Mo.dct2(x), 0.0)
        Z = 2 * Cc[np.abs(np.arange(K) - kmax)] * opre.astype(np.complex128)
        c = oc.astype(np.complex128)
        y = np.array([np.sum(Z * c[(m - np.arange(K)) + (K - 1)]) for m in range(M)]) * opost.astype(np.complex128) * (M / float(span))
        assert np.abs(y - Mo.mirror_matrix(N, M, origin, span) @ x).max() <= 1e-12
