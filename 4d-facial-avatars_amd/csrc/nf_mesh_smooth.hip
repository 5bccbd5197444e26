// Taubin smoothing of an indexed triangle mesh and the vertex normals of its faces (DESIGN.md "Mesh smoothing" is the normative text;
// tests/mesh_smooth_ref.py restates it in NumPy).
//
//   a face is valid iff its three indices lie in [0, V); a valid face (a, b, c) has the sides ab, bc, ca, a side with equal ends is
//   dropped; N(v) = the distinct w != v joined to v by a side, ascending; the multiplicity of {v, w} = the number of sides joining
//   them; a vertex is on the boundary iff it ends an edge of multiplicity 1.  One pass with factor f, from p to p' (two buffers):
//   s = the coordinates of N(v) summed in ascending order from the first, m = s / float(|N(v)|), t = m - p[v], u = f * t,
//   p'[v] = p[v] + u, every operation rounded on its own; a vertex without neighbours or pinned is copied.  Normals: per valid face
//   (p[b] - p[a]) x (p[c] - p[a]); per vertex their sum over the faces that hold it, each once, ascending face id, divided by its
//   length ((sx sx + sy sy) + sz sz, square root) if that is positive and finite, else zero.
//
// One thread per vertex, face or row, 256 per workgroup.  Both tables -- vertex -> neighbours and vertex -> faces -- are the same
// construction (template parameter ADJ: what a face emits, and whether equal entries of a row are merged and counted):
//   k_ms_zero     cursor[0 .. V] = 0; the boundary count = 0
//   k_ms_count    every valid face: cursor[row] += 1 per entry (integer atomicAdd: a sum)
//   k_ms_sum / k_ms_scan1 / k_ms_offsets   exclusive scan (the block sums: nf_scan_dev.h) -> raw_start[0 .. V]; cursor = raw_start
//   k_ms_fill     every valid face: raw[cursor[row]++] = entry (integer atomicAdd; the order WITHIN a row is arbitrary here ...)
//   k_ms_sort     ... and fixed here: a row of at most SHORT_ROW entries is sorted by its thread (insertion sort in an LDS column),
//                 a longer one by its wave (rank sort, O(d^2 / 64), into a second buffer).  ADJ: equal entries merged, their number
//                 = the multiplicity, the row's length to row_start[v]
//   k_ms_sum / k_ms_scan1 / k_ms_offsets   (ADJ) row_start scanned in place; E
//   k_ms_compact  (ADJ) rows moved to their final place; boundary[v]; the number of boundary vertices (integer atomicAdd of sums)
//   k_ms_pass     the gather, once per pass;  k_ms_face_cross, k_ms_vertex_normals
// No float atomics, no loop that waits for another workgroup; what one kernel writes the next one reads.  A row belongs to one
// thread or one wave from k_ms_sort on, so nothing after k_ms_fill depends on arrival order: two calls give the same bits.  The
// workspace may arrive with any content: every word a kernel reads was written by an earlier kernel of the same call.
#include <math.h>
#include "nf_mesh_dev.h"
#include "nf_scan_dev.h"

namespace nfs {
constexpr int SCAN_PER_THREAD = 4;         // k_ms_scan1: block sums per thread and round (a round takes 4096 sums: 2^20 rows)
constexpr int SHORT_ROW = 32;              // entries (repeats included) of the longest row one thread sorts; longer rows take a wave
}  // namespace nfs

// ---- workspace plan
struct NfMsPlan {
    int64_t rows, blocks_rows, blocks_v, blocks_f;         // rows = V + 1: the scans carry the total in their last entry
    size_t off_cursor, off_raw_start, off_block, off_a, off_b, off_c, bytes;
};

// false: a size the plan does not serve.  V and 6 F stay below 2^31 (ids, positions and counts are int32); either may be 0.
static inline bool nf_ms_plan(int64_t n_vertices, int64_t n_faces, NfMsPlan* p) {
    if (n_vertices < 0 || n_faces < 0 || n_vertices > 0x7fffffff || n_faces > 0x7fffffff / 6) return false;
    p->rows = n_vertices + 1;
    p->blocks_rows = nf_blocks(p->rows);
    p->blocks_v = nf_blocks(n_vertices);
    p->blocks_f = nf_blocks(n_faces);
    NfWorkspace ws;
    p->off_cursor = ws.take((size_t)p->rows * 4);
    p->off_raw_start = ws.take((size_t)p->rows * 4);
    p->off_block = ws.take((size_t)p->blocks_rows * 4);
    p->off_a = ws.take((size_t)n_faces * 24);                       // the unsorted rows; (ADJ) then the merged ones
    p->off_b = ws.take((size_t)n_faces * 24);                       // (ADJ) the multiplicities; else the sorted rows
    p->off_c = ws.take((size_t)n_faces * 24);                       // (ADJ) a long row, sorted, before it is merged; else the face vectors
    p->bytes = ws.at;
    return true;
}

extern "C" size_t nf_mesh_smooth_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    NfMsPlan p;
    return nf_ms_plan(n_vertices, n_faces, &p) ? p.bytes : 0;
}

// what a valid face puts into the table: ADJ, (v, w) and (w, v) per side with distinct ends -- at most 6; else (v, f) for each of
// its distinct vertices -- at most 3
template <bool ADJ, class Emit>
__device__ __forceinline__ void nf_ms_entries(const NfFace& t, int f, Emit emit) {
    if (ADJ) {
        if (t.a != t.b) emit(t.a, t.b), emit(t.b, t.a);
        if (t.b != t.c) emit(t.b, t.c), emit(t.c, t.b);
        if (t.c != t.a) emit(t.c, t.a), emit(t.a, t.c);
    } else {
        emit(t.a, f);
        if (t.b != t.a) emit(t.b, f);
        if (t.c != t.a && t.c != t.b) emit(t.c, f);
    }
}

// ---- the table builder
__global__ void __launch_bounds__(nfc::THREADS) k_ms_zero(int* __restrict__ cursor, int64_t rows, unsigned long long* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (i < rows) cursor[i] = 0;
    if (i == 0 && counts) counts[1] = 0ull;
}

template <bool ADJ>
__global__ void __launch_bounds__(nfc::THREADS) k_ms_count(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, int* __restrict__ cursor) {
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const NfFace t = nf_face(faces, f, n_vertices);                 // range-checked before anything is indexed
    if (!t.valid) return;
    nf_ms_entries<ADJ>(t, (int)f, [&](int row, int) { atomicAdd(cursor + row, 1); });
}

template <bool ADJ>
__global__ void __launch_bounds__(nfc::THREADS) k_ms_fill(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, int* __restrict__ cursor,
                                                          int* __restrict__ raw) {
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const NfFace t = nf_face(faces, f, n_vertices);
    if (!t.valid) return;
    nf_ms_entries<ADJ>(t, (int)f, [&](int row, int entry) { raw[atomicAdd(cursor + row, 1)] = entry; });   // the same faces as k_ms_count: inside the row
}

// the scan of x[0 .. n_valid) (entry n_valid .. rows-1 counts 0) in three kernels: the sum of every workgroup's 256 entries ...
__global__ void __launch_bounds__(nfc::THREADS) k_ms_sum(const int* x, int64_t n_valid, uint32_t* __restrict__ block) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t i = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t total = nf_block_total<nfc::WAVES>(i < n_valid ? (uint32_t)x[i] : 0u, s_wave);
    if (threadIdx.x == 0) block[blockIdx.x] = total;
}

// ... one workgroup: the block sums -> their exclusive prefixes in place; the total to *total_out ...
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_ms_scan1(uint32_t* __restrict__ a, int64_t n_blocks, long long* __restrict__ header_slot,
                                                               long long* __restrict__ total_out) {
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    const uint32_t carry = nf_scan_block_sums<nfs::SCAN_PER_THREAD>(a, n_blocks, s_wave);
    if (threadIdx.x == 0) {
        *header_slot = (long long)carry;
        if (total_out) *total_out = (long long)carry;
    }
}

// ... and out[i] = the sum of x[0 .. i) for i in [0, rows) (out2 too, unless NULL).  x may be out or out2: a thread reads its own
// entry before the workgroup's scan and writes it after.
__global__ void __launch_bounds__(nfc::THREADS) k_ms_offsets(const int* x, int64_t n_valid, int64_t rows, const uint32_t* __restrict__ block, int* out,
                                                             int* out2) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t i = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t mine = i < n_valid ? (uint32_t)x[i] : 0u;
    uint32_t total;
    const uint32_t before = block[blockIdx.x] + nf_block_scan<nfc::WAVES>(mine, s_wave, &total) - mine;
    if (i >= rows) return;
    out[i] = (int)before;
    if (out2) out2[i] = (int)before;
}

// Row v = raw[raw_start[v] .. raw_start[v + 1]).  MERGE: the row's distinct entries ascending to `raw` (in place), the number of
// times each was there to `out`, the number of distinct entries to length[v]; `sorted` holds a long row between its two steps.
// Otherwise the row, ascending, to `out` (sorted is not used).  No lane leaves early: the long rows are the whole wave's work.
template <bool MERGE>
__global__ void __launch_bounds__(nfc::THREADS) k_ms_sort(const int* __restrict__ raw_start, int64_t n_vertices, int* raw, int* sorted_buf, int* out,
                                                          int* __restrict__ length) {
    __shared__ int s_row[nfs::SHORT_ROW * nfc::THREADS];            // entry i of thread t at [i * THREADS + t]: no bank conflicts
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int begin = 0, d = 0;
    if (v < n_vertices) {
        begin = raw_start[v];
        d = raw_start[v + 1] - begin;
    }
    if (d <= nfs::SHORT_ROW) {
        int* r = s_row + threadIdx.x;
        for (int i = 0; i < d; ++i) r[i * nfc::THREADS] = raw[(int64_t)begin + i];
        for (int i = 1; i < d; ++i) {
            const int x = r[i * nfc::THREADS];
            int j = i;
            for (; j > 0 && r[(j - 1) * nfc::THREADS] > x; --j) r[j * nfc::THREADS] = r[(j - 1) * nfc::THREADS];
            r[j * nfc::THREADS] = x;
        }
        if (MERGE) {
            int u = 0;
            for (int i = 0; i < d;) {
                const int x = r[i * nfc::THREADS];
                int run = 1;
                while (i + run < d && r[(i + run) * nfc::THREADS] == x) ++run;
                raw[(int64_t)begin + u] = x;
                out[(int64_t)begin + u] = run;
                ++u, i += run;
            }
            if (v < n_vertices) length[v] = u;
        } else {
            for (int i = 0; i < d; ++i) out[(int64_t)begin + i] = r[i * nfc::THREADS];
        }
    }
    unsigned long long todo = __ballot(d > nfs::SHORT_ROW);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t rb = __builtin_amdgcn_readfirstlane(__shfl(begin, owner, 64));      // the same in every lane, and scalar for the compiler
        const int rd = __builtin_amdgcn_readfirstlane(__shfl(d, owner, 64));
        int* sorted = (MERGE ? sorted_buf : out) + rb;
        const int* row = raw + rb;
        // rank sort: entry i goes to the number of entries below it, equal ones in their order.  64 entries j per load, handed
        // round lane by lane
        for (int i0 = 0; i0 < rd; i0 += 64) {
            const int i = i0 + lane;
            const int x = i < rd ? row[i] : 0;
            int rank = 0;
            for (int j0 = 0; j0 < rd; j0 += 64) {
                const int y = j0 + lane < rd ? row[j0 + lane] : 0;
                const int m = rd - j0 < 64 ? rd - j0 : 64;
                for (int q = 0; q < m; ++q) {
                    const int yq = __builtin_amdgcn_readlane(y, q);
                    rank += (yq < x || (yq == x && j0 + q < i)) ? 1 : 0;
                }
            }
            if (i < rd) sorted[rank] = x;
        }
        if (!MERGE) continue;
        __threadfence();                                            // the wave reads next what its other lanes stored
        // a head = the first of equal entries; head number u goes to raw[u], and tells head u - 1 how many entries it led
        int heads_before = 0, last_head = 0;                        // the same in every lane
        for (int k0 = 0; k0 < rd; k0 += 64) {
            const int k = k0 + lane;
            const bool have = k < rd;
            const int x = have ? __hip_atomic_load(sorted + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            const int prev = have && k > 0 ? __hip_atomic_load(sorted + k - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            const bool head = have && (k == 0 || prev != x);
            const unsigned long long heads = __ballot(head);
            const unsigned long long lower = heads & ((1ull << lane) - 1ull);
            if (head) {
                const int u = heads_before + __popcll(lower);
                raw[rb + u] = x;                                    // u <= k, and the rank sort has read the whole row
                if (u > 0) out[rb + u - 1] = k - (lower ? k0 + 63 - __clzll((long long)lower) : last_head);
            }
            if (heads) last_head = k0 + 63 - __clzll((long long)heads);
            heads_before += __popcll(heads);
        }
        if (lane == owner) {
            out[rb + heads_before - 1] = rd - last_head;            // rd > 0: there is a head
            length[v] = heads_before;
        }
    }
}

// rows to their final place (E <= 6 F entries, and none past E is written); boundary[v] = some edge of v has multiplicity 1
__global__ void __launch_bounds__(nfc::THREADS) k_ms_compact(const int* __restrict__ raw_start, const int* __restrict__ merged, const int* __restrict__ times,
                                                             const int* __restrict__ row_start, int64_t n_vertices, int* __restrict__ neighbours,
                                                             int* __restrict__ multiplicity, uint8_t* __restrict__ boundary,
                                                             unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t open = 0;
    if (v < n_vertices) {
        const int64_t from = raw_start[v], to = row_start[v];
        const int n = row_start[v + 1] - (int)to;
        for (int i = 0; i < n; ++i) {
            const int m = times[from + i];
            neighbours[to + i] = merged[from + i];
            multiplicity[to + i] = m;
            open |= m == 1 ? 1u : 0u;
        }
        boundary[v] = (uint8_t)open;
    }
    const uint32_t total = nf_block_total<nfc::WAVES>(open, s_wave);
    if (threadIdx.x == 0 && total) atomicAdd(counts + 1, (unsigned long long)total);
}

// ---- the pass.  row_start == NULL: a copy
__global__ void __launch_bounds__(nfc::THREADS) k_ms_pass(const float* __restrict__ src, int64_t n_vertices, const int* __restrict__ row_start,
                                                          const int* __restrict__ neighbours, const uint8_t* __restrict__ pinned, float factor,
                                                          float* __restrict__ dst) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const float px = src[v * 3 + 0], py = src[v * 3 + 1], pz = src[v * 3 + 2];
    float ox = px, oy = py, oz = pz;
    if (row_start) {
        const int64_t b = row_start[v], e = row_start[v + 1];
        if (e > b && !(pinned && pinned[v])) {
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (int64_t i = b; i < e; ++i) {
                int64_t w = neighbours[i];
                w = w >= 0 && w < n_vertices ? w : v;               // a table of nf_mesh_smooth_adjacency holds no other id; no read outside all the same
                const float qx = src[w * 3 + 0], qy = src[w * 3 + 1], qz = src[w * 3 + 2];
                sx = i == b ? qx : nf_add(sx, qx);
                sy = i == b ? qy : nf_add(sy, qy);
                sz = i == b ? qz : nf_add(sz, qz);
            }
            const float d = (float)(e - b);
            ox = nf_add(px, nf_mul(factor, nf_sub(nf_div(sx, d), px)));
            oy = nf_add(py, nf_mul(factor, nf_sub(nf_div(sy, d), py)));
            oz = nf_add(pz, nf_mul(factor, nf_sub(nf_div(sz, d), pz)));
        }
    }
    dst[v * 3 + 0] = ox, dst[v * 3 + 1] = oy, dst[v * 3 + 2] = oz;
}

// ---- normals
__global__ void __launch_bounds__(nfc::THREADS) k_ms_face_cross(const float* __restrict__ vertices, const int* __restrict__ faces, int64_t n_vertices,
                                                                int64_t n_faces, float* __restrict__ cross) {
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const NfFace t = nf_face(faces, f, n_vertices);
    if (!t.valid) return;                                           // no row lists an invalid face
    const float* a = vertices + (int64_t)t.a * 3;
    const float* b = vertices + (int64_t)t.b * 3;
    const float* c = vertices + (int64_t)t.c * 3;
    const float ux = nf_sub(b[0], a[0]), uy = nf_sub(b[1], a[1]), uz = nf_sub(b[2], a[2]);
    const float wx = nf_sub(c[0], a[0]), wy = nf_sub(c[1], a[1]), wz = nf_sub(c[2], a[2]);
    cross[f * 3 + 0] = nf_sub(nf_mul(uy, wz), nf_mul(uz, wy));
    cross[f * 3 + 1] = nf_sub(nf_mul(uz, wx), nf_mul(ux, wz));
    cross[f * 3 + 2] = nf_sub(nf_mul(ux, wy), nf_mul(uy, wx));
}

__global__ void __launch_bounds__(nfc::THREADS) k_ms_vertex_normals(const int* __restrict__ raw_start, const int* __restrict__ incident,
                                                                    const float* __restrict__ cross, int64_t n_vertices, float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const int64_t b = raw_start[v], e = raw_start[v + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int64_t i = b; i < e; ++i) {
        const int64_t f = incident[i];
        const float qx = cross[f * 3 + 0], qy = cross[f * 3 + 1], qz = cross[f * 3 + 2];
        sx = i == b ? qx : nf_add(sx, qx);
        sy = i == b ? qy : nf_add(sy, qy);
        sz = i == b ? qz : nf_add(sz, qz);
    }
    // sqrtf, not __fsqrt_rn: the intrinsic is the hardware's approximate root in this toolchain (an ulp off now and then -- why the
    // normals of k_iso_verts are compared through a gate); sqrtf without fast-math flags is the correctly rounded one, as nf_div is
    const float len = __builtin_sqrtf(nf_add(nf_add(nf_mul(sx, sx), nf_mul(sy, sy)), nf_mul(sz, sz)));
    const bool ok = len > 0.f && len < INFINITY;                    // k_iso_verts' convention: zero or not finite -> the zero vector
    normals[v * 3 + 0] = ok ? nf_div(sx, len) : 0.f;
    normals[v * 3 + 1] = ok ? nf_div(sy, len) : 0.f;
    normals[v * 3 + 2] = ok ? nf_div(sz, len) : 0.f;
}

// ---- entry points
// the launches up to the sorted rows: raw_start, and the rows in `a` (unsorted) -- ADJ: merged in `a`, counted in `b`, their lengths
// in length[]; else sorted in `b`
template <bool ADJ>
static inline void nf_ms_build(const NfMsPlan& p, const int* faces, int64_t n_vertices, int64_t n_faces, char* ws, int* length,
                               unsigned long long* counts, hipStream_t s) {
    int* cursor = reinterpret_cast<int*>(ws + p.off_cursor);
    int* raw_start = reinterpret_cast<int*>(ws + p.off_raw_start);
    uint32_t* block = reinterpret_cast<uint32_t*>(ws + p.off_block);
    int* a = reinterpret_cast<int*>(ws + p.off_a);
    int* b = reinterpret_cast<int*>(ws + p.off_b);
    int* c = reinterpret_cast<int*>(ws + p.off_c);
    long long* header = reinterpret_cast<long long*>(ws);
    const dim3 threads(nfc::THREADS), grid_rows((unsigned)p.blocks_rows), grid_v((unsigned)p.blocks_v), grid_f((unsigned)p.blocks_f);
    const bool any = n_vertices && n_faces;
    hipLaunchKernelGGL(k_ms_zero, grid_rows, threads, 0, s, cursor, p.rows, counts);
    if (any) hipLaunchKernelGGL(k_ms_count<ADJ>, grid_f, threads, 0, s, faces, n_vertices, n_faces, cursor);
    hipLaunchKernelGGL(k_ms_sum, grid_rows, threads, 0, s, cursor, n_vertices, block);
    hipLaunchKernelGGL(k_ms_scan1, dim3(1), dim3(nfc::SCAN_THREADS), 0, s, block, p.blocks_rows, header, (long long*)nullptr);
    hipLaunchKernelGGL(k_ms_offsets, grid_rows, threads, 0, s, cursor, n_vertices, p.rows, block, raw_start, cursor);
    if (any) hipLaunchKernelGGL(k_ms_fill<ADJ>, grid_f, threads, 0, s, faces, n_vertices, n_faces, cursor, a);
    if (n_vertices) hipLaunchKernelGGL(k_ms_sort<ADJ>, grid_v, threads, 0, s, raw_start, n_vertices, a, c, b, length);
}

extern "C" int nf_mesh_smooth_adjacency(const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                                        int* row_start, int* neighbours, int* multiplicity, uint8_t* boundary, int64_t* counts_dev,
                                        nf_stream_t stream) {
    NfMsPlan p;
    if (!workspace || !row_start || !counts_dev || !nf_ms_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if ((n_faces && (!faces || !neighbours || !multiplicity)) || (n_vertices && !boundary)) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    uint32_t* block = reinterpret_cast<uint32_t*>(ws + p.off_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_dev);
    const dim3 threads(nfc::THREADS), grid_rows((unsigned)p.blocks_rows), grid_v((unsigned)p.blocks_v);
    hipStream_t s = nf_s(stream);
    nf_ms_build<true>(p, faces, n_vertices, n_faces, ws, row_start, counts, s);
    hipLaunchKernelGGL(k_ms_sum, grid_rows, threads, 0, s, row_start, n_vertices, block);
    hipLaunchKernelGGL(k_ms_scan1, dim3(1), dim3(nfc::SCAN_THREADS), 0, s, block, p.blocks_rows, reinterpret_cast<long long*>(ws) + 1,
                       reinterpret_cast<long long*>(counts_dev));
    hipLaunchKernelGGL(k_ms_offsets, grid_rows, threads, 0, s, row_start, n_vertices, p.rows, block, row_start, (int*)nullptr);
    if (n_vertices)
        hipLaunchKernelGGL(k_ms_compact, grid_v, threads, 0, s, reinterpret_cast<const int*>(ws + p.off_raw_start), reinterpret_cast<const int*>(ws + p.off_a),
                           reinterpret_cast<const int*>(ws + p.off_b), row_start, n_vertices, neighbours, multiplicity, boundary, counts);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_smooth_run(const float* vertices, int64_t n_vertices, const int* row_start, const int* neighbours, const uint8_t* pinned,
                                  int iterations, float lam, float mu, float* tmp, float* out, nf_stream_t stream) {
    if (n_vertices < 0 || n_vertices > 0x7fffffff || iterations < 0) return NF_EINVAL;
    if (!(lam > 0.f && lam <= 1.f) || !(mu >= -1.f && mu <= 0.f)) return NF_EINVAL;          // NaN fails both
    const int64_t passes = (int64_t)iterations * (mu != 0.f ? 2 : 1);
    if (n_vertices && (!vertices || !out || out == vertices)) return NF_EINVAL;
    if (n_vertices && passes && (!row_start || !neighbours)) return NF_EINVAL;
    if (n_vertices && passes > 1 && (!tmp || tmp == out || tmp == vertices)) return NF_EINVAL;
    if (!n_vertices) return 0;
    const dim3 threads(nfc::THREADS), grid((unsigned)nf_blocks(n_vertices));
    hipStream_t s = nf_s(stream);
    if (!passes) hipLaunchKernelGGL(k_ms_pass, grid, threads, 0, s, vertices, n_vertices, (const int*)nullptr, (const int*)nullptr, (const uint8_t*)nullptr, 0.f, out);
    const float* src = vertices;
    for (int64_t k = 0; k < passes; ++k) {
        float* dst = ((passes - 1 - k) & 1) ? tmp : out;            // the last pass writes `out`
        const float factor = mu != 0.f && (k & 1) ? mu : lam;
        hipLaunchKernelGGL(k_ms_pass, grid, threads, 0, s, src, n_vertices, row_start, neighbours, pinned, factor, dst);
        src = dst;
    }
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_smooth_normals(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace,
                                      size_t workspace_bytes, float* normals, nf_stream_t stream) {
    NfMsPlan p;
    if (!workspace || !nf_ms_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if ((n_faces && !faces) || (n_vertices && (!vertices || !normals))) return NF_EINVAL;
    if (!n_vertices) return 0;
    char* ws = static_cast<char*>(workspace);
    float* cross = reinterpret_cast<float*>(ws + p.off_c);
    hipStream_t s = nf_s(stream);
    nf_ms_build<false>(p, faces, n_vertices, n_faces, ws, (int*)nullptr, (unsigned long long*)nullptr, s);
    if (n_faces)
        hipLaunchKernelGGL(k_ms_face_cross, dim3((unsigned)p.blocks_f), dim3(nfc::THREADS), 0, s, vertices, faces, n_vertices, n_faces, cross);
    hipLaunchKernelGGL(k_ms_vertex_normals, dim3((unsigned)p.blocks_v), dim3(nfc::THREADS), 0, s, reinterpret_cast<const int*>(ws + p.off_raw_start),
                       reinterpret_cast<const int*>(ws + p.off_b), cross, n_vertices, normals);
    NF_RETURN_LAUNCH();
}
