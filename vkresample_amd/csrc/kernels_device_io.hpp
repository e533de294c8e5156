// kernels_device_io.hpp -- the kernels fftup_execute_device needs beside the frame's own: a strided row copy (gather into the
// lane's staging planes, scatter out of the lane's scratch image) and the 8-bit pack with a destination row stride.  They are off
// the fast path, which is the frame kernels reading and writing the caller's memory in place.  Not handed to the plan-time
// compiler; needs kernels_generic.hpp (cvt_f_u8, cvt4_f_u8, cvt4_h_u8) in front of it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

namespace fftup {

// ---------------------------------------------------------------- strided row copy
// `planes` x `rows` rows of row_bytes bytes, source and destination each with a row and a plane stride in bytes.  A row is cut
// where the DESTINATION is 16-byte aligned: thread 0 of a row takes the bytes in front of the first boundary, thread t >= 1 the
// t-th 16-byte piece behind it, the last one what is left.  A whole piece is one 16-byte store; it is one 16-byte load too when the
// source is aligned there, and loads of G bytes otherwise.  Heads and tails move in units of G bytes.  G: a power of two that
// divides both addresses, every stride and row_bytes (the element size, or 1 for byte rows and for pointers that are not element
// aligned).  Nothing outside the rows' row_bytes bytes is read or written.  grid (ceil((row_bytes / 16 + 2) / 256), rows, planes).
struct CopyRowsParams {
    const uint8_t* src;
    uint8_t* dst;
    long src_row, src_plane, dst_row, dst_plane;
    long row_bytes;
};
template <int G> struct CopyUnit;
template <> struct CopyUnit<1> { typedef uint8_t type; };
template <> struct CopyUnit<2> { typedef uint16_t type; };
template <> struct CopyUnit<4> { typedef uint32_t type; };
template <> struct CopyUnit<8> { typedef uint64_t type; };

template <int G>
__global__ void __launch_bounds__(256) k_copy_rows(CopyRowsParams p)
{
    typedef typename CopyUnit<G>::type U;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const uint8_t* s = p.src + (long)blockIdx.z * p.src_plane + (long)blockIdx.y * p.src_row;
    uint8_t* d = p.dst + (long)blockIdx.z * p.dst_plane + (long)blockIdx.y * p.dst_row;
    long head = (long)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > p.row_bytes) head = p.row_bytes;
    const long b0 = t == 0 ? 0 : head + 16 * (t - 1);
    long b1 = t == 0 ? head : b0 + 16;
    if (b1 > p.row_bytes) b1 = p.row_bytes;
    if (b0 >= b1) return;
    if (b1 - b0 == 16) {
        union { uint4 v; U e[16 / G]; } r;
        if (((uintptr_t)(s + b0) & 15) == 0) r.v = *(const uint4*)(s + b0);
        else {
#pragma unroll
            for (int i = 0; i < 16 / G; i++) r.e[i] = ((const U*)(s + b0))[i];
        }
        *(uint4*)(d + b0) = r.v;
        return;
    }
    for (long b = b0; b < b1; b += G) *(U*)(d + b) = *(const U*)(s + b);
}

// ---------------------------------------------------------------- 8-bit pack with a destination row stride
// k_pack_u8 / k_pack_u8_f64 (VkResample.cpp:1708-1748) writing rows of row_stride_bytes: the same conversions (cvt4_f_u8,
// cvt4_h_u8, cvt_f_u8: the same bytes), the planes dense [3][uH][uW].  One thread = four consecutive pixels: 16-byte (8-byte)
// plane loads where the row length keeps the quads aligned, twelve bytes out as three dwords where the destination row is 4-byte
// aligned, byte stores otherwise.  Only the 3 uW bytes of a row are written.  grid (ceil(uW / 1024), uH), block 256.
template <bool HALF>
__global__ void __launch_bounds__(256) k_pack_u8_strided(const void* planes, uint8_t* rgb, long row_stride_bytes, int uW, int uH, int wrap)
{
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y = blockIdx.y;
    if (x >= uW) return;
    const long plane = (long)uW * uH, at = (long)y * uW + x;
    uint8_t* dst = rgb + (long)y * row_stride_bytes + 3l * x;
    if (x + 4 <= uW && (uW & 3) == 0) {                     // whole quad, aligned in the planes
        uint8_t b[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if constexpr (HALF) {
                const uint2 r = *(const uint2*)((const __half*)planes + c * plane + at);
                cvt4_h_u8(__builtin_bit_cast(cvt_h2, r.x), __builtin_bit_cast(cvt_h2, r.y), wrap, b[c]);
            } else {
                const float4 r = *(const float4*)((const float*)planes + c * plane + at);
                cvt4_f_u8(r.x, r.y, r.z, r.w, wrap, b[c]);
            }
        }
        if (((uintptr_t)dst & 3) == 0) {
            unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int k = 3 * i + c;
                    o[k >> 2] |= (unsigned)b[c][i] << (8 * (k & 3));
                }
            unsigned* d = (unsigned*)dst;
            d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < 3; c++) dst[3 * i + c] = b[c][i];
        }
        return;
    }
    for (int i = 0; i < 4 && x + i < uW; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float v;
            if constexpr (HALF) v = __half2float(((const __half*)planes)[c * plane + at + i]);
            else v = ((const float*)planes)[c * plane + at + i];
            dst[3 * i + c] = cvt_f_u8(v, wrap);
        }
}

// -p 1: one thread = one pixel, as k_pack_u8_f64
__global__ void __launch_bounds__(256) k_pack_u8_f64_strided(const double* planes, uint8_t* rgb, long row_stride_bytes, int uW, int uH, int wrap)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= uW) return;
    const long plane = (long)uW * uH;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double d = 255.0 * planes[c * plane + (long)y * uW + x];
        uint8_t o;
        if (wrap) o = (d > -2147483648.0 && d < 2147483648.0) ? (uint8_t)(((int)d) & 0xFF) : 0;
        else o = !(d > 0.0) ? 0 : (d >= 255.0 ? 255 : (uint8_t)d);
        rgb[(long)y * row_stride_bytes + 3l * x + c] = o;
    }
}

}  // namespace fftup
