// Device helpers shared by the render translation units (nf_render.hip, nf_render_bwd_full.hip): the ray -> wavefront mapping,
// the wavefront scans and the per-sample quantities of the volume integrator.
#pragma once
#include "nf_common.h"

// nf_render.hip states these two itself, beside NF_MAX_BINS and NF_MAX_SORT: tests/test_host.py reads all the size limits that
// nerf/ops.py mirrors from that file's own #defines.  Every other unit takes them from here, and the assert keeps the two equal.
#ifndef NF_MAX_CHUNKS
#define NF_RAYS_PER_BLOCK 4                   // 4 waves = 256 threads per block, one ray each
#define NF_MAX_CHUNKS 16                      // <= 1024 samples per ray
#endif
static_assert(NF_RAYS_PER_BLOCK == 4 && NF_MAX_CHUNKS == 16, "the render units must agree on the ray mapping and the chunk limit");

__device__ __forceinline__ int nf_lane() { return threadIdx.x & 63; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_rscan_add(float v) {      // inclusive, from the last lane down: the sum over lanes >= this one
    const int l = nf_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_down(v, o, 64); if (l + o < 64) v += t; }
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v) {       // inclusive
    const int l = nf_lane();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(v, o, 64); if (l >= o) v *= t; }
    return v;
}

// ---------------------------------------------------------------------------------------------
// Per-sample quantities of volume_render_radiance_field (reference volume_rendering_utils.py:19-55)
// ---------------------------------------------------------------------------------------------
struct NfSample {
    float c[3];     // colour entering the sum (sigmoid(raw) or the background for the last sample)
    float alpha;    // 1 - exp(-sigma*dist)
    float dist;
    float pre;      // raw_sigma + noise (ReLU argument)
    bool  is_bg;
};

__device__ __forceinline__ float nf_sigmoid(float x) { return nf_div(1.0f, nf_add(1.0f, expf(-x))); }

// mode bits: 1 = scale the sample spacing by |rd| (V:26), 2 = add 1e-6 to the last density (V:52-53), 4 = report the depth
// map sum(w z) instead of the disparity.  NeRFace = 3; tiny_nerf's render_volume_density (tiny_nerf.py:68-107) = 4.
#define NF_VR_NERFACE 3
#define NF_VR_TINY 4

__device__ __forceinline__ NfSample nf_load_sample(const float4* __restrict__ raw_row, const float* __restrict__ z_row,
                                                   const float* __restrict__ noise_row, const float* __restrict__ bg_ray,
                                                   float rd_norm, int s, int S, int mode = NF_VR_NERFACE) {
    NfSample o;
    const float4 r = raw_row[s];
    const bool last = (s == S - 1);
    o.is_bg = last && bg_ray != nullptr;
    if (o.is_bg) { o.c[0] = bg_ray[0]; o.c[1] = bg_ray[1]; o.c[2] = bg_ray[2]; }
    else { o.c[0] = nf_sigmoid(r.x); o.c[1] = nf_sigmoid(r.y); o.c[2] = nf_sigmoid(r.z); }
    const float d = last ? 1e10f : nf_sub(z_row[s + 1], z_row[s]);
    o.dist = (mode & 1) ? nf_mul(d, rd_norm) : d;
    o.pre = noise_row ? nf_add(r.w, noise_row[s]) : r.w;
    float sigma = o.pre < 0.0f ? 0.0f : o.pre;                     // torch.relu: a NaN density stays NaN (fmaxf would turn it into 0)
    if (last && (mode & 2)) sigma = nf_add(sigma, 1e-6f);         // V:52-53
    o.alpha = nf_sub(1.0f, expf(-nf_mul(sigma, o.dist)));
    return o;
}

__device__ __forceinline__ float nf_rd_norm(const float* __restrict__ rd_ray) {
    const float x = rd_ray[0], y = rd_ray[1], zc = rd_ray[2];
    return sqrtf(nf_add(nf_add(nf_mul(x, x), nf_mul(y, y)), nf_mul(zc, zc)));
}
