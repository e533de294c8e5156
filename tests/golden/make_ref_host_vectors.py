#!/usr/bin/env python3
"""Generates tests/golden/ref_host_conversions.npz: the reference's own host conversions (oracle/_ref/libref_host.so, built by
oracle/Makefile where the reference tree is present: half.hpp and the casts of VkResample.cpp:1644 / 1676 / 1715) evaluated on
fixed inputs, so that the oracle can be pinned against them anywhere (tests/test_oracle.py)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_host.so"))
    ref.ref_pack_half.restype = C.c_double
    ref.ref_pack_half.argtypes = [C.c_ubyte]
    ref.ref_pack_float.restype = C.c_double
    ref.ref_pack_float.argtypes = [C.c_ubyte]
    ref.ref_unpack_float.restype = C.c_ubyte
    ref.ref_unpack_float.argtypes = [C.c_float]
    ref.ref_half_round.restype = C.c_double
    ref.ref_half_round.argtypes = [C.c_double]
    rng = np.random.default_rng(1)
    # round to binary16: a dense sweep incl. ties, subnormals and the overflow edge (half.hpp converts from float)
    hr_x = np.concatenate([rng.uniform(-2, 2, 20000), rng.uniform(-1e-4, 1e-4, 5000),
                           (np.arange(0, 4096) + 0.5) * 2.0 ** -11, [0.0, 6.0e-8, 2.0 ** -25, 65504.0, 65519.0]])
    hr_x = hr_x.astype(np.float32).astype(np.float64)
    # the 8-bit store: in range, and out of range (UB in the reference; what x86-64 gcc does with it)
    st_x = np.concatenate([np.arange(256) / 255.0, rng.uniform(0, 1, 4000)]).astype(np.float32)
    wrap_x = np.array([-1.6 / 255, -0.3, 256.3 / 255, 1.5]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "ref_host_conversions.npz"),
                        pack_float=np.array([ref.ref_pack_float(v) for v in range(256)]),
                        pack_half=np.array([ref.ref_pack_half(v) for v in range(256)]),
                        hr_x=hr_x, hr_y=np.array([ref.ref_half_round(float(x)) for x in hr_x]),
                        st_x=st_x, st_y=np.array([ref.ref_unpack_float(float(x)) for x in st_x], np.uint8),
                        wrap_x=wrap_x, wrap_y=np.array([ref.ref_unpack_float(float(x)) for x in wrap_x], np.uint8))
    print("ref_host_conversions.npz:", len(hr_x), "half roundings,", len(st_x), "+", len(wrap_x), "stores")


if __name__ == "__main__":
    main()
