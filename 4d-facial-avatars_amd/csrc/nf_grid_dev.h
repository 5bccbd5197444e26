// What the kernels over a dense grid share (nf_isosurface.hip, nf_sparse_grid.hip): the grids they serve, the box and the coordinate
// of a grid index, and the split of a linear point index into (i, j, k).  The workgroup scan and the workspace: nf_scan_dev.h.
#pragma once
#include "nf_scan_dev.h"

// the number of points of a grid ops.isosurface serves: every axis >= 2, 7 * points and 12 * cells below 2^31 (V <= 7 points and
// F <= 12 cells are bounded BEFORE any launch, so every count and every prefix fits 31 bits); 0 for any other grid
static inline int64_t nf_grid_points(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    if ((int64_t)nx * ny > 0x7fffffff) return 0;                // the product is checked stepwise: no 64-bit overflow
    const int64_t n = (int64_t)nx * ny * nz;
    const int64_t cells = (int64_t)(nx - 1) * (ny - 1) * (nz - 1);
    return 7 * n > 0x7fffffff || 12 * cells > 0x7fffffff ? 0 : n;
}

struct NfGridBox { float lo[3], h[3]; };

// false: !(lo < hi) on an axis (NaN bounds too).  h as nerf.mesh.grid_axes computes it: (hi - lo) / float32(n - 1), in float32.
static inline bool nf_grid_box(const float* lo, const float* hi, int nx, int ny, int nz, NfGridBox* box) {
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        if (!(lo[a] < hi[a])) return false;
        box->lo[a] = lo[a];
        box->h[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
    }
    return true;
}

// the coordinate of index i: multiply, then add, no fused multiply-add -- the bits of grid_axes
__device__ __forceinline__ float nf_grid_coord(float lo, float h, int i) { return nf_add(lo, nf_mul((float)i, h)); }

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
