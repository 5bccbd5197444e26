// Isosurface of a dense float32 grid v[nz][ny][nx] (x fastest) at `level` inside the box [lo, hi]: an indexed, welded, consistently
// oriented triangle mesh by marching tetrahedra on the Kuhn (Freudenthal) triangulation -- every cell is cut into the six
// tetrahedra 0 -> e(p0) -> e(p0) + e(p1) -> 7 of the axis permutations p, which is translation invariant and matches across cell
// faces, so the surface is watertight by construction.  (The normative text is DESIGN.md "Isosurface"; tests/isosurface_ref.py
// restates it in NumPy.)
//
//   grid point (i, j, k) at lo + (i, j, k) * h, h = (hi - lo) / (n - 1) per axis; inside iff v > level (NaN and == level: outside)
//   grid point g owns the seven edges e = 1..7 to g + (e & 1, (e >> 1) & 1, e >> 2); an edge that crosses yields ONE vertex at
//   p_a + t (p_b - p_a), t = (level - v_a) / (v_b - v_a), 0.5 unless 0 <= t <= 1; vertex ids count the crossing edges in the order
//   (k, j, i, e); faces are ordered by (cell, tetrahedron, triangle).
//
// Every tetrahedron edge runs from a cell corner to a corner that contains its bits, so its owner is the lower corner's grid point
// and e the difference: a triangle's vertex id is vbase[owner] + (number of crossing edges of the owner below e).  That needs the
// exclusive count `vbase` of every point and its 7-bit crossing mask, which is what the workspace holds.
//
// Four launches, one thread per grid point (a cell is the point at its corner 0), 256 points per workgroup, no atomics:
//   nf_isosurface_count: k_iso_count  corner values -> inside bits (1 B) and crossing mask (1 B) per point; per-workgroup sums of
//                                     vertices and triangles
//                        k_iso_scan   one workgroup: both arrays of sums -> exclusive prefixes (nf_scan_dev.h); V and F
//   nf_isosurface_emit:  k_iso_verts  crossing mask -> wave64 / workgroup scan -> vbase[point]; positions (and normals) of the
//                                     point's own edges
//                        k_iso_faces  inside bits -> triangles per cell -> scan -> face base; indices from vbase / mask of the owners
// The order of every sum is fixed, so two calls give the same bits.  Memory-bound: 4 B per point read (the seven far corners come
// from the cache), 2 + 4 B written, 1 + 1 B read again, plus the output.
#include "nf_grid_dev.h"

namespace nfi {
constexpr int SCAN_PER_THREAD = 16;        // k_iso_scan: block sums per thread and round.  The header: V, F

// ---- the case table, derived at compile time (host and device see the same constant expression)
constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};   // lexicographic

constexpr int tet_corner(int tet, int n) {
    return n == 0 ? 0 : n == 1 ? (1 << PERM[tet][0]) : n == 2 ? ((1 << PERM[tet][0]) | (1 << PERM[tet][1])) : 7;
}

struct Table {
    uint32_t entry[6 * 16];                // [tet][inside mask]: six 4-bit vertex codes (lo | hi << 2, an edge of tet vertices lo < hi),
                                           // triangles in bits 24..25, flip bit 26 (the stored order already has the flip applied)
    bool quads_agree, oriented;
};

// twice the midpoint of the edge (m, n) of tetrahedron `tet` on the unit cell, per axis
constexpr int mid2(int tet, int m, int n, int axis) { return ((tet_corner(tet, m) >> axis) & 1) + ((tet_corner(tet, n) >> axis) & 1); }

// sign of (p1 - p0) x (p2 - p0) . (x_out - x_in) for the triangle of edges (a0,b0), (a1,b1), (a2,b2), every t = 0.5
constexpr int tri_side(int tet, const int (&e)[3][2], int v_in, int v_out) {
    int p[3][3] = {};
    for (int v = 0; v < 3; ++v)
        for (int ax = 0; ax < 3; ++ax) p[v][ax] = mid2(tet, e[v][0], e[v][1], ax);
    const int u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const int w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const int c[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    int d = 0;
    for (int ax = 0; ax < 3; ++ax) d += c[ax] * (((tet_corner(tet, v_out) >> ax) & 1) - ((tet_corner(tet, v_in) >> ax) & 1));
    return d;
}

constexpr uint32_t edge_code(int m, int n) { return (uint32_t)(m < n ? (m | (n << 2)) : (n | (m << 2))); }

constexpr Table build_table() {
    Table t = {};
    t.quads_agree = true;
    t.oriented = true;
    for (int tet = 0; tet < 6; ++tet) {
        for (int mask = 0; mask < 16; ++mask) {
            int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
            for (int v = 0; v < 4; ++v) {
                if ((mask >> v) & 1) in[n_in++] = v;
                else out[n_out++] = v;
            }
            int tri[2][3][2] = {};
            int n_tri = 0, v_in = 0, v_out = 0;
            if (n_in == 1) {                                   // inside {a}, outside b < c < d: (ab, ac, ad)
                n_tri = 1, v_in = in[0], v_out = out[0];
                for (int v = 0; v < 3; ++v) tri[0][v][0] = in[0], tri[0][v][1] = out[v];
            } else if (n_in == 3) {                            // outside {a}, inside b < c < d: (ab, ac, ad)
                n_tri = 1, v_in = in[0], v_out = out[0];
                for (int v = 0; v < 3; ++v) tri[0][v][0] = out[0], tri[0][v][1] = in[v];
            } else if (n_in == 2) {                            // inside a < b, outside c < d: (ac, ad, bd), (ac, bd, bc)
                n_tri = 2, v_in = in[0], v_out = out[0];
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                const int q[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
                for (int k = 0; k < 2; ++k)
                    for (int v = 0; v < 3; ++v) tri[k][v][0] = q[k][v][0], tri[k][v][1] = q[k][v][1];
            }
            uint32_t e = (uint32_t)n_tri << 24;
            bool flip = false;
            for (int k = 0; k < n_tri; ++k) {
                const int side = tri_side(tet, tri[k], v_in, v_out);
                if (side == 0) t.oriented = false;
                if (k == 0) flip = side < 0;
                else if (flip != (side < 0)) t.quads_agree = false;
            }
            for (int k = 0; k < n_tri; ++k)
                for (int v = 0; v < 3; ++v) {
                    const int s = flip && v ? 3 - v : v;       // flip: the last two indices change places
                    e |= edge_code(tri[k][s][0], tri[k][s][1]) << (4 * (3 * k + v));
                }
            if (flip) e |= 1u << 26;
            t.entry[tet * 16 + mask] = e;
        }
    }
    return t;
}

constexpr bool counts_follow_the_corner_count(const Table& t) {
    for (int e = 0; e < 96; ++e) {
        const int m = e & 15, in = (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + (m >> 3);
        if ((int)(t.entry[e] >> 24 & 3u) != (in == 2 ? 2 : (in & 1))) return false;
    }
    return true;
}

constexpr Table TABLE = build_table();
static_assert(counts_follow_the_corner_count(TABLE), "nf_iso_cell_tris counts triangles from the number of inside corners");
static_assert(TABLE.quads_agree, "the two triangles of a quad must take the same flip");
static_assert(TABLE.oriented, "a triangle of the table is degenerate against its inside -> outside direction");
}  // namespace nfi

__constant__ nfi::Table c_iso_table = nfi::build_table();

extern "C" int nf_isosurface_table(uint32_t* out) {
    if (!out) return NF_EINVAL;
    for (int i = 0; i < 96; ++i) out[i] = nfi::TABLE.entry[i];
    return 0;
}

// ---- workspace plan
struct NfIsoPlan {
    int64_t n_points, n_blocks;
    size_t off_block_v, off_block_f, off_vbase, off_mask, off_inside, bytes;
};

// false: a grid the plan does not serve (nf_grid_points)
static inline bool nf_iso_plan(int nx, int ny, int nz, NfIsoPlan* p) {
    const int64_t n = nf_grid_points(nx, ny, nz);
    if (!n) return false;
    p->n_points = n;
    p->n_blocks = nf_blocks(n);
    NfWorkspace ws;
    p->off_block_v = ws.take((size_t)p->n_blocks * 4);
    p->off_block_f = ws.take((size_t)p->n_blocks * 4);
    p->off_vbase = ws.take((size_t)n * 4);
    p->off_mask = ws.take((size_t)n);
    p->off_inside = ws.take((size_t)n);
    p->bytes = ws.at;
    return true;
}

extern "C" size_t nf_isosurface_workspace_bytes(int nx, int ny, int nz) {
    NfIsoPlan p;
    return nf_iso_plan(nx, ny, nz, &p) ? p.bytes : 0;
}

// ---- device helpers (the workgroup scan nf_block_scan: nf_scan_dev.h; the index split nf_iso_point: nf_grid_dev.h)
// triangles of a cell from the inside bits of its eight corners: per tetrahedron 1 for one or three corners inside, 2 for two (the
// table's own counts, without a per-lane table read for every point of the grid)
__device__ __forceinline__ uint32_t nf_iso_cell_tris(uint32_t inside) {
    uint32_t n = 0;
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
        const uint32_t in = (inside & 1u) + ((inside >> nfi::tet_corner(tet, 1)) & 1u) + ((inside >> nfi::tet_corner(tet, 2)) & 1u) + ((inside >> 7) & 1u);
        n += in == 2u ? 2u : (in & 1u);
    }
    return n;
}

__global__ void __launch_bounds__(nfc::THREADS) k_iso_count(const float* __restrict__ grid, int nx, int ny, int nz, float level, int64_t n_points,
                                                            uint8_t* __restrict__ mask_out, uint8_t* __restrict__ inside_out,
                                                            uint32_t* __restrict__ block_v, uint32_t* __restrict__ block_f) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t p = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t n_vert = 0, n_tri = 0;
    if (p < n_points) {
        const NfIsoPoint g = nf_iso_point(p, nx, ny);
        const bool has_x = g.i + 1 < nx, has_y = g.j + 1 < ny, has_z = g.k + 1 < nz;
        const int64_t sy = nx, sz = (int64_t)nx * ny;
        uint32_t inside = 0, exists = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool here = (!(c & 1) || has_x) && (!(c & 2) || has_y) && (!(c & 4) || has_z);
            if (here) {
                const float v = grid[p + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz];
                exists |= 1u << c;
                inside |= (v > level ? 1u : 0u) << c;
            }
        }
        const uint32_t own = inside & 1u ? 0xffu : 0u;
        const uint32_t mask = ((inside ^ own) & exists) >> 1;       // bit e - 1: edge e exists and exactly one end is inside
        n_vert = __popc(mask);
        const bool cell = has_x && has_y && has_z;
        if (cell) n_tri = nf_iso_cell_tris(inside);
        mask_out[p] = (uint8_t)mask;
        inside_out[p] = cell ? (uint8_t)inside : (uint8_t)0;       // a point that is no cell's corner 0 reads as an empty cell
    }
    // both sums in one pass: <= 7 * 256 vertices below, <= 12 * 256 triangles above bit 16
    const uint32_t total = nf_block_total<nfc::WAVES>(n_vert | n_tri << 16, s_wave);
    if (threadIdx.x == 0) {
        block_v[blockIdx.x] = total & 0xffffu;
        block_f[blockIdx.x] = total >> 16;
    }
}

// one workgroup: both arrays of block sums -> exclusive prefixes in place, the totals to the header and to counts_out
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_iso_scan(uint32_t* __restrict__ block_v, uint32_t* __restrict__ block_f, int64_t n_blocks,
                                                           long long* __restrict__ header, long long* __restrict__ counts_out) {
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    for (int which = 0; which < 2; ++which) {
        const uint32_t carry = nf_scan_block_sums<nfi::SCAN_PER_THREAD>(which ? block_f : block_v, n_blocks, s_wave);
        if (threadIdx.x == 0) {
            header[which] = (long long)carry;
            counts_out[which] = (long long)carry;
        }
    }
}

// central difference of the grid along one axis at index a (stride s), one-sided at the box faces, divided by the spacing
__device__ __forceinline__ float nf_iso_diff(const float* __restrict__ grid, int64_t p, int a, int n, int64_t s, float h) {
    const int64_t up = a + 1 < n ? p + s : p, dn = a > 0 ? p - s : p;
    const float span = (a + 1 < n && a > 0) ? nf_mul(2.0f, h) : h;
    return nf_div(nf_sub(grid[up], grid[dn]), span);
}

__global__ void __launch_bounds__(nfc::THREADS) k_iso_verts(const float* __restrict__ grid, int nx, int ny, int nz, float level, int64_t n_points,
                                                            NfGridBox box, const uint8_t* __restrict__ mask_in,
                                                            const uint32_t* __restrict__ block_v, uint32_t* __restrict__ vbase_out,
                                                            float* __restrict__ verts, int64_t cap_verts, float* __restrict__ normals) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t p = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t mask = p < n_points ? mask_in[p] : 0u;
    const uint32_t n_vert = __popc(mask);
    uint32_t total;
    const uint32_t base = block_v[blockIdx.x] + nf_block_scan<nfc::WAVES>(n_vert, s_wave, &total) - n_vert;
    if (p >= n_points) return;
    vbase_out[p] = base;
    if (!mask) return;
    const NfIsoPoint g = nf_iso_point(p, nx, ny);
    const int64_t sy = nx, sz = (int64_t)nx * ny;
    const float va = grid[p];
    const float pa_x = nf_grid_coord(box.lo[0], box.h[0], g.i), pa_y = nf_grid_coord(box.lo[1], box.h[1], g.j),
                pa_z = nf_grid_coord(box.lo[2], box.h[2], g.k);
    const float pb_x = nf_grid_coord(box.lo[0], box.h[0], g.i + 1), pb_y = nf_grid_coord(box.lo[1], box.h[1], g.j + 1),
                pb_z = nf_grid_coord(box.lo[2], box.h[2], g.k + 1);
    float ga_x = 0.f, ga_y = 0.f, ga_z = 0.f;
    if (normals) {
        ga_x = nf_iso_diff(grid, p, g.i, nx, 1, box.h[0]);
        ga_y = nf_iso_diff(grid, p, g.j, ny, sy, box.h[1]);
        ga_z = nf_iso_diff(grid, p, g.k, nz, sz, box.h[2]);
    }
    int64_t id = base;
#pragma unroll
    for (int e = 1; e < 8; ++e) {
        if (!((mask >> (e - 1)) & 1u)) continue;
        const int dx = e & 1, dy = (e >> 1) & 1, dz = e >> 2;
        const int64_t q = p + dx + dy * sy + dz * sz;               // in the grid: the mask bit says the edge exists
        const float vb = grid[q];
        float t = nf_div(nf_sub(level, va), nf_sub(vb, va));
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;                    // NaN, +-inf and anything outside the edge
        if (id < cap_verts) {
            verts[id * 3 + 0] = nf_add(pa_x, nf_mul(t, nf_sub(dx ? pb_x : pa_x, pa_x)));
            verts[id * 3 + 1] = nf_add(pa_y, nf_mul(t, nf_sub(dy ? pb_y : pa_y, pa_y)));
            verts[id * 3 + 2] = nf_add(pa_z, nf_mul(t, nf_sub(dz ? pb_z : pa_z, pa_z)));
            if (normals) {
                const float gb_x = nf_iso_diff(grid, q, g.i + dx, nx, 1, box.h[0]), gb_y = nf_iso_diff(grid, q, g.j + dy, ny, sy, box.h[1]),
                            gb_z = nf_iso_diff(grid, q, g.k + dz, nz, sz, box.h[2]);
                const float gx = nf_add(ga_x, nf_mul(t, nf_sub(gb_x, ga_x))), gy = nf_add(ga_y, nf_mul(t, nf_sub(gb_y, ga_y))),
                            gz = nf_add(ga_z, nf_mul(t, nf_sub(gb_z, ga_z)));
                const float len = __fsqrt_rn(nf_add(nf_add(nf_mul(gx, gx), nf_mul(gy, gy)), nf_mul(gz, gz)));
                const bool ok = len > 0.0f && len < __builtin_inff();           // false for NaN as well
                normals[id * 3 + 0] = ok ? -nf_div(gx, len) : 0.0f;
                normals[id * 3 + 1] = ok ? -nf_div(gy, len) : 0.0f;
                normals[id * 3 + 2] = ok ? -nf_div(gz, len) : 0.0f;
            }
        }
        ++id;
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_iso_faces(int nx, int ny, int64_t n_points, const uint8_t* __restrict__ mask_in,
                                                            const uint8_t* __restrict__ inside_in, const uint32_t* __restrict__ vbase,
                                                            const uint32_t* __restrict__ block_f, int* __restrict__ faces, int64_t cap_faces) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t p = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t inside = p < n_points ? inside_in[p] : 0u;       // 0 where the point is no cell (k_iso_count)
    const uint32_t n_tri = nf_iso_cell_tris(inside);
    uint32_t total;
    int64_t f = (int64_t)block_f[blockIdx.x] + nf_block_scan<nfc::WAVES>(n_tri, s_wave, &total) - n_tri;
    if (!n_tri) return;
    const int64_t sy = nx, sz = (int64_t)nx * ny;
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
        const int c1 = nfi::tet_corner(tet, 1), c2 = nfi::tet_corner(tet, 2);
        const uint32_t m = (inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
        const uint32_t entry = c_iso_table.entry[tet * 16 + m];
        const uint32_t corners = (uint32_t)c1 << 3 | (uint32_t)c2 << 6 | 7u << 9;   // corner of tet vertex n in bits 3n..3n+2
        const int tris = (int)(entry >> 24 & 3u);
        for (int k = 0; k < tris; ++k) {
            if (f < cap_faces) {
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const uint32_t code = entry >> (4 * (3 * k + v)) & 15u;
                    const uint32_t ca = corners >> (3 * (code & 3u)) & 7u, cb = corners >> (3 * (code >> 2)) & 7u;   // ca's bits lie in cb
                    const int64_t owner = p + (ca & 1u) + ((ca >> 1) & 1u) * sy + (ca >> 2) * sz;                     // a corner of a whole cell
                    const uint32_t e = ca ^ cb;
                    faces[f * 3 + v] = (int)(vbase[owner] + __popc((uint32_t)mask_in[owner] & ((1u << (e - 1)) - 1u)));
                }
            }
            ++f;
        }
    }
}

extern "C" int nf_isosurface_count(const float* grid, int nx, int ny, int nz, float level, void* workspace, size_t workspace_bytes,
                                   int64_t* counts_dev, nf_stream_t stream) {
    NfIsoPlan p;
    if (!grid || !workspace || !counts_dev || !nf_iso_plan(nx, ny, nz, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    uint32_t* block_v = reinterpret_cast<uint32_t*>(ws + p.off_block_v);
    uint32_t* block_f = reinterpret_cast<uint32_t*>(ws + p.off_block_f);
    hipLaunchKernelGGL(k_iso_count, dim3((unsigned)p.n_blocks), dim3(nfc::THREADS), 0, nf_s(stream), grid, nx, ny, nz, level, p.n_points,
                       reinterpret_cast<uint8_t*>(ws + p.off_mask), reinterpret_cast<uint8_t*>(ws + p.off_inside), block_v, block_f);
    hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(nfc::SCAN_THREADS), 0, nf_s(stream), block_v, block_f, p.n_blocks, reinterpret_cast<long long*>(ws),
                       reinterpret_cast<long long*>(counts_dev));
    NF_RETURN_LAUNCH();
}

extern "C" int nf_isosurface_emit(const float* grid, int nx, int ny, int nz, float level, const float* lo, const float* hi, void* workspace,
                                  size_t workspace_bytes, float* verts, int64_t n_verts, int* faces, int64_t n_faces, float* normals,
                                  nf_stream_t stream) {
    NfIsoPlan p;
    if (!grid || !workspace || !lo || !hi || !verts || !faces || !nf_iso_plan(nx, ny, nz, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if (n_verts < 0 || n_faces < 0 || n_verts > 0x7fffffff || n_faces > 0x7fffffff) return NF_EINVAL;
    NfGridBox box;
    if (!nf_grid_box(lo, hi, nx, ny, nz, &box)) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    const uint8_t* mask = reinterpret_cast<const uint8_t*>(ws + p.off_mask);
    uint32_t* vbase = reinterpret_cast<uint32_t*>(ws + p.off_vbase);
    hipLaunchKernelGGL(k_iso_verts, dim3((unsigned)p.n_blocks), dim3(nfc::THREADS), 0, nf_s(stream), grid, nx, ny, nz, level, p.n_points, box, mask,
                       reinterpret_cast<const uint32_t*>(ws + p.off_block_v), vbase, verts, n_verts, normals);
    hipLaunchKernelGGL(k_iso_faces, dim3((unsigned)p.n_blocks), dim3(nfc::THREADS), 0, nf_s(stream), nx, ny, p.n_points, mask,
                       reinterpret_cast<const uint8_t*>(ws + p.off_inside), vbase, reinterpret_cast<const uint32_t*>(ws + p.off_block_f), faces,
                       n_faces);
    NF_RETURN_LAUNCH();
}
