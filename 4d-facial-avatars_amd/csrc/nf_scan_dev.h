// What every scan-and-compact unit shares (nf_isosurface.hip, nf_sparse_grid.hip, nf_mesh_components.hip, nf_mesh_smooth.hip; DESIGN.md
// "Scan-and-compact scaffolding"): one thread per element and 256 elements per workgroup, whose sum is one block sum; one workgroup
// of 1024 threads that turns the block sums into their exclusive prefixes, PER_THREAD of them per thread and round; a workspace that
// starts with a header of 256 bytes and is carved into parts of whole 256 bytes.
#pragma once
#include "nf_common.h"

namespace nfc {
constexpr int THREADS = 256;               // elements per workgroup (4 waves), one block sum each (1024 was measured too: DESIGN.md)
constexpr int WAVES = THREADS / NF_WAVE;
constexpr int SCAN_THREADS = 1024;         // the one workgroup of a unit's scan kernel (k_iso_scan, k_sg_scan, k_mc_scan, k_ms_scan1)
constexpr int SCAN_WAVES = SCAN_THREADS / NF_WAVE;
constexpr int HEADER = 256;                // bytes at the workspace's start: the unit's totals, as int64
}  // namespace nfc

// ---- host: the workspace and the grid of a launch
static inline size_t nf_ws_up(size_t b) { return (b + 255) / 256 * 256; }

// the parts of a workspace, one after the other behind the header: take(bytes) = the part's offset
struct NfWorkspace {
    size_t at = nfc::HEADER;
    size_t take(size_t bytes) {
        const size_t off = at;
        at += nf_ws_up(bytes);
        return off;
    }
};

// workgroups of THREADS for n elements
static inline int64_t nf_blocks(int64_t n) { return (n + nfc::THREADS - 1) / nfc::THREADS; }

// ---- device
// inclusive sum over the workgroup's threads in thread order (wave64 shuffles, then the wave totals); *total = the workgroup's sum
template <int WAVES>
__device__ __forceinline__ uint32_t nf_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
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

// the workgroup's sum alone, for the kernels that count and keep no prefix (the same scan: its shuffles and its two barriers)
template <int WAVES>
__device__ __forceinline__ uint32_t nf_block_total(uint32_t v, uint32_t* s_wave) {
    uint32_t total;
    nf_block_scan<WAVES>(v, s_wave, &total);
    return total;
}

// One workgroup of SCAN_THREADS: the block sums a[0 .. n_blocks) -> their exclusive prefixes in place, in rounds of SCAN_THREADS *
// PER_THREAD sums with the total so far carried from round to round; returns the total (the same in every thread).  s_wave holds
// SCAN_WAVES words.
template <int PER_THREAD>
__device__ __forceinline__ uint32_t nf_scan_block_sums(uint32_t* __restrict__ a, int64_t n_blocks, uint32_t* s_wave) {
    uint32_t carry = 0;
    for (int64_t base = 0; base < n_blocks; base += (int64_t)nfc::SCAN_THREADS * PER_THREAD) {
        const int64_t at = base + (int64_t)threadIdx.x * PER_THREAD;
        uint32_t v[PER_THREAD], sum = 0;                            // unrolled: registers, constant indices only
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            v[q] = at + q < n_blocks ? a[at + q] : 0u;
            sum += v[q];
        }
        uint32_t total;
        uint32_t run = carry + nf_block_scan<nfc::SCAN_WAVES>(sum, s_wave, &total) - sum;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            if (at + q < n_blocks) a[at + q] = run;
            run += v[q];
        }
        carry += total;
    }
    return carry;
}
