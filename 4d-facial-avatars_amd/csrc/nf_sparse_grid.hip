// Sparse evaluation of a dense float32 grid v[nz][ny][nx] (x fastest) around the surface v == level: which points a network has to be
// asked for, and +-inf ("not evaluated, side known") everywhere else, so that ops.isosurface gives the dense grid's mesh.  (The
// normative text is DESIGN.md "Sparse density grid"; tests/sparse_grid_ref.py restates it in NumPy.)
//
//   bricks of B cells: axis a has m = ceil((n - 1) / B) bricks, brick b covers the point indices [B b, min(B (b + 1), n - 1)]; bricks
//   share their faces.  The coarse lattice is the product of the indices {0, B, 2B, ...} u {n - 1}: the brick corners, m + 1 per axis.
//   seed brick:   NOT (all 8 corners > level + margin) and NOT (all 8 corners < level - margin); the two thresholds are float32 sums
//   active brick: within `dilate` bricks (Chebyshev) of a seed
//   evaluated:    the lattice points and every point of every active brick, each once; every other point lies only in bricks that
//                 are no seeds and gets +inf where their corners are inside (v > level), -inf where they are outside
//
// The caller evaluates the lattice (nf_sparse_grid_lattice gives its coordinates and indices), scatters the values into the grid,
// classifies, marks, evaluates the marked points and scatters again:
//   nf_sparse_grid_lattice:  k_sg_lattice   one thread per lattice point: linear index and coordinates
//   nf_sparse_grid_classify: k_sg_classify  one thread per brick: 8 corner values of the grid -> seed flag and side (1 B each)
//                            k_sg_dilate    one thread per brick: any seed in the (2 dilate + 1)^3 neighbourhood -> active flag
//   nf_sparse_grid_mark:     k_sg_count     one thread per point: to evaluate and not on the lattice? -> per-workgroup sums
//                            k_sg_scan      one workgroup: the sums -> exclusive prefixes (nf_scan_dev.h); the total
//   nf_sparse_grid_emit:     k_sg_emit      the same decision -> wave64 / workgroup scan -> slot in ascending linear index: index and
//                                           coordinates; +-inf into the points that are not evaluated
//   nf_sparse_grid_scatter:  k_sg_scatter   grid[index[t]] = values[t]
// 256 threads per workgroup; the only atomics are one integer add per workgroup for the two brick counts, so two calls give the same
// bits.  The point kernels read no per-point memory at all (the brick flags of a 512^3 grid at B = 8 are 256 KiB and stay in the
// cache): k_sg_emit writes 4 B per point that is skipped and 16 B per point that is listed.
#include "nf_grid_dev.h"

namespace nfg {
constexpr int SCAN_PER_THREAD = 16;        // k_sg_scan: block sums per thread and round.  The header: seed bricks, active bricks, points
                                           // to evaluate beside the lattice
}  // namespace nfg

// ---- plan
struct NfSgDims {
    int n[3], m[3], B;                     // points and bricks per axis; the brick size, cut to the longest axis (one brick there as well)
};

struct NfSgPlan {
    NfSgDims d;
    int64_t n_points, n_blocks, n_bricks, n_lattice;
    size_t off_seed, off_side, off_active, off_block, bytes;
};

// false: a brick below 2 cells, or a grid ops.isosurface does not serve (nf_grid_points)
static inline bool nf_sg_plan(int nx, int ny, int nz, int brick, NfSgPlan* p) {
    p->n_points = nf_grid_points(nx, ny, nz);
    if (brick < 2 || !p->n_points) return false;
    const int n[3] = {nx, ny, nz};
    const int longest = (nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz)) - 1;
    p->d.B = brick < longest ? brick : longest;                 // a larger brick is one brick per axis either way; B * (m + 1) < 2^29
    p->n_bricks = 1, p->n_lattice = 1;
    for (int a = 0; a < 3; ++a) {
        p->d.n[a] = n[a];
        p->d.m[a] = (n[a] - 1 + p->d.B - 1) / p->d.B;
        p->n_bricks *= p->d.m[a];
        p->n_lattice *= p->d.m[a] + 1;
    }
    p->n_blocks = nf_blocks(p->n_points);
    NfWorkspace ws;
    p->off_seed = ws.take((size_t)p->n_bricks);
    p->off_side = ws.take((size_t)p->n_bricks);
    p->off_active = ws.take((size_t)p->n_bricks);
    p->off_block = ws.take((size_t)p->n_blocks * 4);
    p->bytes = ws.at;
    return true;
}

extern "C" size_t nf_sparse_grid_workspace_bytes(int nx, int ny, int nz, int brick) {
    NfSgPlan p;
    return nf_sg_plan(nx, ny, nz, brick, &p) ? p.bytes : 0;
}

// ---- device helpers (the box and nf_grid_coord: nf_grid_dev.h)
// first point index of brick b along an axis of n points (b == m: the last index)
__device__ __forceinline__ int nf_sg_corner(int b, int B, int n) { return min(b * B, n - 1); }

struct NfSgAxis { int lo, hi; bool lattice; };                   // the bricks [lo, hi] that contain an index; is it a lattice index?

__device__ __forceinline__ NfSgAxis nf_sg_axis(int i, int n, int m, int B) {
    const uint32_t q = (uint32_t)i / (uint32_t)B, r = (uint32_t)i - q * (uint32_t)B;
    NfSgAxis a;
    a.hi = min((int)q, m - 1);                                  // i == n - 1 == B m belongs to the last brick only
    a.lo = r == 0u && q > 0u ? min((int)q - 1, m - 1) : a.hi;   // a shared face: the brick below as well
    a.lattice = r == 0u || i == n - 1;
    return a;
}

enum { NF_SG_KEEP = 0, NF_SG_EVAL = 1, NF_SG_INSIDE = 2, NF_SG_OUTSIDE = 3 };

// what becomes of point (i, j, k): KEEP (a lattice point: evaluated before, its value stands in the grid), EVAL (in an active brick),
// or the side of its bricks, which are no seeds and agree (they share at least one corner)
__device__ __forceinline__ int nf_sg_decide(const NfIsoPoint g, const NfSgDims d, const uint8_t* __restrict__ active, const uint8_t* __restrict__ side) {
    const NfSgAxis x = nf_sg_axis(g.i, d.n[0], d.m[0], d.B), y = nf_sg_axis(g.j, d.n[1], d.m[1], d.B), z = nf_sg_axis(g.k, d.n[2], d.m[2], d.B);
    if (x.lattice && y.lattice && z.lattice) return NF_SG_KEEP;
    uint32_t any = 0;
    for (int bz = z.lo; bz <= z.hi; ++bz)
        for (int by = y.lo; by <= y.hi; ++by)
            for (int bx = x.lo; bx <= x.hi; ++bx) any |= active[((int64_t)bz * d.m[1] + by) * d.m[0] + bx];
    if (any) return NF_SG_EVAL;
    return side[((int64_t)z.hi * d.m[1] + y.hi) * d.m[0] + x.hi] ? NF_SG_INSIDE : NF_SG_OUTSIDE;
}

// ---- kernels
__global__ void __launch_bounds__(nfc::THREADS) k_sg_lattice(NfSgDims d, NfGridBox box, int64_t n_lattice, int* __restrict__ index_out,
                                                             float* __restrict__ coords_out) {
    const int64_t t = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (t >= n_lattice) return;
    const NfIsoPoint c = nf_iso_point(t, d.m[0] + 1, d.m[1] + 1);
    const int i = nf_sg_corner(c.i, d.B, d.n[0]), j = nf_sg_corner(c.j, d.B, d.n[1]), k = nf_sg_corner(c.k, d.B, d.n[2]);
    index_out[t] = (int)(((int64_t)k * d.n[1] + j) * d.n[0] + i);
    coords_out[t * 3 + 0] = nf_grid_coord(box.lo[0], box.h[0], i);
    coords_out[t * 3 + 1] = nf_grid_coord(box.lo[1], box.h[1], j);
    coords_out[t * 3 + 2] = nf_grid_coord(box.lo[2], box.h[2], k);
}

// the workgroup's number of set flags -> one integer add
__device__ __forceinline__ void nf_sg_count_flags(uint32_t flag, uint32_t* s_wave, unsigned long long* counter) {
    const uint32_t total = nf_block_total<nfc::WAVES>(flag, s_wave);
    if (threadIdx.x == 0 && total) atomicAdd(counter, (unsigned long long)total);
}

__global__ void __launch_bounds__(nfc::THREADS) k_sg_classify(const float* __restrict__ grid, NfSgDims d, float above, float below, int64_t n_bricks,
                                                              uint8_t* __restrict__ seed_out, uint8_t* __restrict__ side_out,
                                                              unsigned long long* __restrict__ header) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t q = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t seed = 0;
    if (q < n_bricks) {
        const NfIsoPoint b = nf_iso_point(q, d.m[0], d.m[1]);
        const int i[2] = {nf_sg_corner(b.i, d.B, d.n[0]), nf_sg_corner(b.i + 1, d.B, d.n[0])};
        const int j[2] = {nf_sg_corner(b.j, d.B, d.n[1]), nf_sg_corner(b.j + 1, d.B, d.n[1])};
        const int k[2] = {nf_sg_corner(b.k, d.B, d.n[2]), nf_sg_corner(b.k + 1, d.B, d.n[2])};
        bool all_in = true, all_out = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = grid[((int64_t)k[c >> 2] * d.n[1] + j[(c >> 1) & 1]) * d.n[0] + i[c & 1]];
            all_in = all_in && v > above;                        // NaN fails both
            all_out = all_out && v < below;
        }
        seed = all_in || all_out ? 0u : 1u;
        seed_out[q] = (uint8_t)seed;
        side_out[q] = all_in ? (uint8_t)1 : (uint8_t)0;
    }
    nf_sg_count_flags(seed, s_wave, header + 0);
}

__global__ void __launch_bounds__(nfc::THREADS) k_sg_dilate(const uint8_t* __restrict__ seed, NfSgDims d, int dilate, int64_t n_bricks,
                                                            uint8_t* __restrict__ active_out, unsigned long long* __restrict__ header) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t q = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t active = 0;
    if (q < n_bricks) {
        const NfIsoPoint b = nf_iso_point(q, d.m[0], d.m[1]);
        active = seed[q];
        const int x0 = max(b.i - dilate, 0), x1 = min(b.i + dilate, d.m[0] - 1), y0 = max(b.j - dilate, 0), y1 = min(b.j + dilate, d.m[1] - 1),
                  z0 = max(b.k - dilate, 0), z1 = min(b.k + dilate, d.m[2] - 1);
        for (int bz = z0; bz <= z1 && !active; ++bz)
            for (int by = y0; by <= y1 && !active; ++by)
                for (int bx = x0; bx <= x1; ++bx) active |= seed[((int64_t)bz * d.m[1] + by) * d.m[0] + bx];
        active_out[q] = (uint8_t)active;
    }
    nf_sg_count_flags(active, s_wave, header + 1);
}

__global__ void __launch_bounds__(nfc::THREADS) k_sg_count(NfSgDims d, int64_t n_points, const uint8_t* __restrict__ active,
                                                           const uint8_t* __restrict__ side, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t p = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t flag = p < n_points && nf_sg_decide(nf_iso_point(p, d.n[0], d.n[1]), d, active, side) == NF_SG_EVAL ? 1u : 0u;
    const uint32_t total = nf_block_total<nfc::WAVES>(flag, s_wave);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one workgroup: the block sums -> exclusive prefixes in place; the total to the header; the header's three counts to counts_out
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_sg_scan(uint32_t* __restrict__ a, int64_t n_blocks, long long* __restrict__ header,
                                                               long long* __restrict__ counts_out) {
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    const uint32_t carry = nf_scan_block_sums<nfg::SCAN_PER_THREAD>(a, n_blocks, s_wave);
    if (threadIdx.x == 0) {
        header[2] = (long long)carry;
        counts_out[0] = header[0];
        counts_out[1] = header[1];
        counts_out[2] = (long long)carry;
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_sg_emit(float* __restrict__ grid, NfSgDims d, NfGridBox box, int64_t n_points,
                                                          const uint8_t* __restrict__ active, const uint8_t* __restrict__ side,
                                                          const uint32_t* __restrict__ block_base, int* __restrict__ index_out,
                                                          float* __restrict__ coords_out, int64_t capacity) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t p = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    NfIsoPoint g = {0, 0, 0};
    int what = NF_SG_KEEP;
    if (p < n_points) {
        g = nf_iso_point(p, d.n[0], d.n[1]);
        what = nf_sg_decide(g, d, active, side);
    }
    const uint32_t flag = what == NF_SG_EVAL ? 1u : 0u;
    uint32_t total;
    const int64_t slot = (int64_t)block_base[blockIdx.x] + nf_block_scan<nfc::WAVES>(flag, s_wave, &total) - flag;
    if (what == NF_SG_EVAL) {
        if (slot < capacity) {
            index_out[slot] = (int)p;
            coords_out[slot * 3 + 0] = nf_grid_coord(box.lo[0], box.h[0], g.i);
            coords_out[slot * 3 + 1] = nf_grid_coord(box.lo[1], box.h[1], g.j);
            coords_out[slot * 3 + 2] = nf_grid_coord(box.lo[2], box.h[2], g.k);
        }
    } else if (what != NF_SG_KEEP) {
        grid[p] = what == NF_SG_INSIDE ? __builtin_inff() : -__builtin_inff();
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_sg_scatter(const float* __restrict__ values, const int* __restrict__ index, int64_t count,
                                                             float* __restrict__ grid, int64_t n_points) {
    const int64_t t = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (t >= count) return;
    const int64_t p = index[t];
    if (p >= 0 && p < n_points) grid[p] = values[t];             // an index that is none of the grid's writes nothing
}

// ---- entry points
extern "C" int nf_sparse_grid_lattice(int nx, int ny, int nz, int brick, const float* lo, const float* hi, int* index, float* coords,
                                      int64_t capacity, nf_stream_t stream) {
    NfSgPlan p;
    NfGridBox box;
    if (!lo || !hi || !index || !coords || !nf_sg_plan(nx, ny, nz, brick, &p) || capacity < p.n_lattice || !nf_grid_box(lo, hi, nx, ny, nz, &box))
        return NF_EINVAL;
    hipLaunchKernelGGL(k_sg_lattice, dim3((unsigned)nf_blocks(p.n_lattice)), dim3(nfc::THREADS), 0, nf_s(stream), p.d, box, p.n_lattice, index, coords);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_sparse_grid_classify(const float* grid, int nx, int ny, int nz, int brick, float level, float margin, int dilate,
                                       void* workspace, size_t workspace_bytes, nf_stream_t stream) {
    NfSgPlan p;
    if (!grid || !workspace || !nf_sg_plan(nx, ny, nz, brick, &p) || workspace_bytes < p.bytes || !(margin >= 0.0f) || dilate < 0) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    unsigned long long* header = reinterpret_cast<unsigned long long*>(ws);
    uint8_t* seed = reinterpret_cast<uint8_t*>(ws + p.off_seed);
    const hipError_t e = hipMemsetAsync(ws, 0, nfc::HEADER, nf_s(stream));
    if (e != hipSuccess) return (int)e;
    const int reach = p.d.m[0] > p.d.m[1] ? (p.d.m[0] > p.d.m[2] ? p.d.m[0] : p.d.m[2]) : (p.d.m[1] > p.d.m[2] ? p.d.m[1] : p.d.m[2]);
    if (dilate > reach) dilate = reach;                          // covers the grid already, and brick index + dilate stays an int
    const unsigned blocks = (unsigned)nf_blocks(p.n_bricks);
    hipLaunchKernelGGL(k_sg_classify, dim3(blocks), dim3(nfc::THREADS), 0, nf_s(stream), grid, p.d, level + margin, level - margin, p.n_bricks, seed,
                       reinterpret_cast<uint8_t*>(ws + p.off_side), header);
    hipLaunchKernelGGL(k_sg_dilate, dim3(blocks), dim3(nfc::THREADS), 0, nf_s(stream), seed, p.d, dilate, p.n_bricks,
                       reinterpret_cast<uint8_t*>(ws + p.off_active), header);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_sparse_grid_mark(int nx, int ny, int nz, int brick, void* workspace, size_t workspace_bytes, int64_t* counts_dev,
                                   nf_stream_t stream) {
    NfSgPlan p;
    if (!workspace || !counts_dev || !nf_sg_plan(nx, ny, nz, brick, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    uint32_t* block = reinterpret_cast<uint32_t*>(ws + p.off_block);
    hipLaunchKernelGGL(k_sg_count, dim3((unsigned)p.n_blocks), dim3(nfc::THREADS), 0, nf_s(stream), p.d, p.n_points,
                       reinterpret_cast<const uint8_t*>(ws + p.off_active), reinterpret_cast<const uint8_t*>(ws + p.off_side), block);
    hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(nfc::SCAN_THREADS), 0, nf_s(stream), block, p.n_blocks, reinterpret_cast<long long*>(ws),
                       reinterpret_cast<long long*>(counts_dev));
    NF_RETURN_LAUNCH();
}

extern "C" int nf_sparse_grid_emit(float* grid, int nx, int ny, int nz, int brick, const float* lo, const float* hi, void* workspace,
                                   size_t workspace_bytes, int* index, float* coords, int64_t capacity, nf_stream_t stream) {
    NfSgPlan p;
    NfGridBox box;
    if (!grid || !lo || !hi || !workspace || !nf_sg_plan(nx, ny, nz, brick, &p) || workspace_bytes < p.bytes || capacity < 0 ||
        (capacity > 0 && (!index || !coords)) || !nf_grid_box(lo, hi, nx, ny, nz, &box))
        return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(k_sg_emit, dim3((unsigned)p.n_blocks), dim3(nfc::THREADS), 0, nf_s(stream), grid, p.d, box, p.n_points,
                       reinterpret_cast<const uint8_t*>(ws + p.off_active), reinterpret_cast<const uint8_t*>(ws + p.off_side),
                       reinterpret_cast<const uint32_t*>(ws + p.off_block), index, coords, capacity);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_sparse_grid_scatter(const float* values, const int* index, int64_t count, float* grid, int nx, int ny, int nz,
                                      nf_stream_t stream) {
    if (count == 0) return 0;
    const int64_t n_points = nf_grid_points(nx, ny, nz);
    if (!values || !index || !grid || !n_points || count < 0 || count > n_points) return NF_EINVAL;
    hipLaunchKernelGGL(k_sg_scatter, dim3((unsigned)nf_blocks(count)), dim3(nfc::THREADS), 0, nf_s(stream), values, index, count, grid, n_points);
    NF_RETURN_LAUNCH();
}
