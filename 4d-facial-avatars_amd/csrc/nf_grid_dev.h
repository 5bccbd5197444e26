// Device helpers the kernels over a dense grid share (nf_isosurface.hip, nf_sparse_grid.hip): the workgroup scan in thread order and
// the split of a linear point index into (i, j, k).
#pragma once
#include "nf_common.h"

// inclusive sum over the workgroup's threads in thread order (wave64 shuffles, then the wave totals); *total = the workgroup's sum
template <int WAVES>
__device__ __forceinline__ uint32_t nf_iso_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    __syncthreads();                                            // s_wave may still be read from the previous call
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    *total = all;
    return v + before;
}

struct NfIsoPoint { int i, j, k; };

// (i, j, k) of point p.  The plans keep the number of points below 2^31, so the two divisions are 32-bit ones (a 64-bit division
// is some hundred instructions, and every thread of k_iso_count takes two); everything that addresses memory stays 64-bit.
__device__ __forceinline__ NfIsoPoint nf_iso_point(int64_t p, int nx, int ny) {
    const uint32_t q = (uint32_t)p, row = q / (uint32_t)nx, k = row / (uint32_t)ny;
    NfIsoPoint g;
    g.i = (int)(q - row * (uint32_t)nx);
    g.k = (int)k;
    g.j = (int)(row - k * (uint32_t)ny);
    return g;
}
