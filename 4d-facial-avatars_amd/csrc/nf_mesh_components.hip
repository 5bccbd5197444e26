// Connected components of an indexed triangle mesh and the mesh of the components one rule keeps (DESIGN.md "Mesh components" is the
// normative text; tests/mesh_components_ref.py restates it in NumPy).
//
//   a face is valid iff its three indices lie in [0, V); two vertices are connected iff a chain of valid faces links them (a shared
//   vertex is enough); components are numbered 0 .. C-1 by ascending smallest vertex id; a face carries the label of its first
//   vertex, an invalid face -1.  Kept: the component with the most faces (ties: the lower label; nothing if no component has a face)
//   or every component with at least m faces.  The filtered mesh holds the kept vertices and the valid faces of kept components in
//   their original order, the indices renumbered.
//
// One thread per vertex or face, 256 per workgroup.  Labelling is a union-find over the vertices whose root is the SMALLEST id of its
// set: the larger root is hooked under the smaller with atomicMin, so parent[x] <= x always, parent[] only ever falls, and the final
// partition and its roots do not depend on the order in which the faces arrive.  Every access to parent[] that another workgroup may
// race with is a relaxed agent-scope atomic (the L2s of the XCDs are not coherent for plain loads); no loop waits for another
// workgroup: every turn of nf_mc_find and nf_mc_union strictly lowers an id.  Kernel boundaries give the rest of the visibility:
//   nf_mesh_components_label:  k_mc_init     parent[v] = v
//                              k_mc_hook     valid face (a, b, c): union(a, b), union(a, c)
//                              k_mc_flatten  parent[v] = find(v); per-workgroup number of roots
//                              k_mc_scan     one workgroup: the block sums -> exclusive prefixes (nf_scan_dev.h); C
//                              k_mc_rank     roots: vertex_label[root] = its rank (the numbering rule); the counts of that rank = 0
//                              k_mc_labels   the other vertices and the faces take their root's rank; counts by integer atomicAdd
//   nf_mesh_components_select: k_mc_select   one workgroup: the argmax of face_counts (largest) and the number of kept components
//                              k_mc_keep     per-workgroup numbers of kept vertices and kept faces
//                              k_mc_scan     both arrays of block sums; V' and F'
//   nf_mesh_components_emit:   k_mc_emit_verts  scan -> new id of every kept vertex; rows of vertices (and normals) copied
//                              k_mc_emit_faces  scan -> row of every kept face; indices through the new ids
// Integer sums only, in a fixed order or by integer atomics: two calls give the same bits.  The workspace may arrive with any
// content: every word a kernel reads was written by an earlier kernel of the same call chain.
#include "nf_mesh_dev.h"
#include "nf_scan_dev.h"

namespace nfm {
constexpr int SCAN_PER_THREAD = 4;         // k_mc_scan: block sums per thread and round (a round takes 4096 sums: 2^20 vertices)

struct Header {                            // the workspace's start
    long long components, kept_vertices, kept_faces, kept_components;
    long long min_faces;                   // the rule k_mc_select was given: largest (best_label) or min_faces >= 1
    int largest, best_label;               // best_label: -1 = keep nothing
};
static_assert(sizeof(Header) <= nfc::HEADER, "the header has 256 bytes");
}  // namespace nfm

// ---- workspace plan
struct NfMcPlan {
    int64_t blocks_v, blocks_f;
    size_t off_parent, off_new_id, off_block_v, off_block_f, bytes;
};

// false: a size the plan does not serve.  V and F stay below 2^31 (ids and counts are int32); either may be 0.
static inline bool nf_mc_plan(int64_t n_vertices, int64_t n_faces, NfMcPlan* p) {
    if (n_vertices < 0 || n_faces < 0 || n_vertices > 0x7fffffff || n_faces > 0x7fffffff) return false;
    p->blocks_v = nf_blocks(n_vertices);
    p->blocks_f = nf_blocks(n_faces);
    NfWorkspace ws;
    p->off_parent = ws.take((size_t)n_vertices * 4);
    p->off_new_id = ws.take((size_t)n_vertices * 4);
    p->off_block_v = ws.take((size_t)p->blocks_v * 4);
    p->off_block_f = ws.take((size_t)p->blocks_f * 4);
    p->bytes = ws.at;
    return true;
}

extern "C" size_t nf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    NfMcPlan p;
    return nf_mc_plan(n_vertices, n_faces, &p) ? p.bytes : 0;
}

// ---- union-find with the smallest id as the root
__device__ __forceinline__ int nf_mc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// an ancestor of x that was a root when it was read.  Path halving: x skips its parent (atomicMin: parent[x] only ever falls).  x
// falls with every turn (grandparent < parent < x), so the loop ends whatever the other workgroups do.
__device__ __forceinline__ int nf_mc_find(int* __restrict__ parent, int x) {
    for (;;) {
        const int p = nf_mc_load(parent + x);
        if (p == x) return x;
        const int g = nf_mc_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

// joins the sets of a and b.  The larger root goes under the smaller one; if it was a root no longer (atomicMin returns its parent of
// that moment, below hi), the link it had and the one it has now differ, so that parent and lo are joined next: max(x, y) falls
// with every turn.
__device__ __forceinline__ void nf_mc_union(int* __restrict__ parent, int a, int b) {
    int x = nf_mc_find(parent, a), y = nf_mc_find(parent, b);
    while (x != y) {
        const int hi = x > y ? x : y, lo = x > y ? y : x;
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) break;                                      // hi was a root and hangs under lo now
        x = nf_mc_find(parent, old);                               // <= old < hi
        y = nf_mc_find(parent, lo);                                // <= lo < hi
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_mc_init(int* __restrict__ parent, int64_t n_vertices) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (v < n_vertices) parent[v] = (int)v;
}

__global__ void __launch_bounds__(nfc::THREADS) k_mc_hook(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, int* __restrict__ parent) {
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const NfFace t = nf_face(faces, f, n_vertices);                 // range-checked before anything is indexed
    if (!t.valid) return;
    // two vertices with the same parent are joined already (a parent lies in its child's set): no find, which would end in a read
    // of the root's word -- in a mesh of one component the same word for every face
    const int pa = nf_mc_load(parent + t.a), pb = nf_mc_load(parent + t.b), pc = nf_mc_load(parent + t.c);
    if (pb != pa) nf_mc_union(parent, t.a, t.b);
    if (pc != pa && pc != pb) nf_mc_union(parent, t.a, t.c);
}

// parent[v] = the root of v (no hook runs any more, so a root stays one; other threads' halving and this store only lower
// parent[], towards the same root); the number of roots per workgroup
__global__ void __launch_bounds__(nfc::THREADS) k_mc_flatten(int* __restrict__ parent, int64_t n_vertices, uint32_t* __restrict__ block_v) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t is_root = 0;
    if (v < n_vertices) {
        const int r = nf_mc_find(parent, (int)v);
        if (r != (int)v) atomicMin(parent + v, r);
        is_root = r == (int)v ? 1u : 0u;
    }
    const uint32_t total = nf_block_total<nfc::WAVES>(is_root, s_wave);
    if (threadIdx.x == 0) block_v[blockIdx.x] = total;
}

// one workgroup: up to two arrays of block sums -> exclusive prefixes in place; their totals to header[slot] and counts_out[slot]
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_mc_scan(uint32_t* __restrict__ a0, int64_t n0, int slot0, uint32_t* __restrict__ a1, int64_t n1,
                                                          int slot1, int n_arrays, long long* __restrict__ header, long long* __restrict__ counts_out) {
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    for (int which = 0; which < n_arrays; ++which) {
        const uint32_t carry = nf_scan_block_sums<nfm::SCAN_PER_THREAD>(which ? a1 : a0, which ? n1 : n0, s_wave);
        if (threadIdx.x == 0) {
            const int slot = which ? slot1 : slot0;
            header[slot] = (long long)carry;
            counts_out[slot] = (long long)carry;
        }
    }
}

// a root's label is the number of roots below it; the two counts of that label start at 0 (labels >= C are never written)
__global__ void __launch_bounds__(nfc::THREADS) k_mc_rank(const int* __restrict__ parent, int64_t n_vertices, const uint32_t* __restrict__ block_v,
                                                          int* __restrict__ vertex_label, int* __restrict__ face_counts, int* __restrict__ vertex_counts) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t is_root = v < n_vertices && parent[v] == (int)v ? 1u : 0u;
    uint32_t total;
    const uint32_t rank = block_v[blockIdx.x] + nf_block_scan<nfc::WAVES>(is_root, s_wave, &total) - is_root;
    if (!is_root) return;
    vertex_label[v] = (int)rank;
    face_counts[rank] = 0;
    vertex_counts[rank] = 0;
}

// counts[label] += 1 for every lane with label >= 0, one atomicAdd per RUN of equal labels in the wave (every lane of the wave calls
// this).  Neighbouring vertices and faces mostly share their component, and adds to one address are served one after the other: one
// add per element made labelling a mesh of one component ten times as slow as its extraction.
__device__ __forceinline__ void nf_mc_count_runs(int* __restrict__ counts, int label, int* s_first) {
    if (threadIdx.x == 0) *s_first = label;
    __syncthreads();
    if (__syncthreads_and(label == *s_first)) {                    // the whole workgroup in one component: one add
        if (threadIdx.x == 0 && label >= 0) atomicAdd(counts + label, nfc::THREADS);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(label, 1, 64);
    const bool start = lane == 0 || before != label;
    const unsigned long long starts = __ballot(start);
    if (!start || label < 0) return;
    const unsigned long long later = lane == 63 ? 0ull : starts >> (lane + 1);      // the run ends where the next one starts
    atomicAdd(counts + label, later ? __ffsll(later) : 64 - lane);
}

// workgroups [0, blocks_v): vertices, the rest: faces.  Both read the labels of ROOTS only, which k_mc_rank wrote.
__global__ void __launch_bounds__(nfc::THREADS) k_mc_labels(const int* __restrict__ faces, const int* __restrict__ parent, int64_t n_vertices, int64_t n_faces,
                                                            int64_t blocks_v, int* __restrict__ vertex_label, int* __restrict__ face_label,
                                                            int* __restrict__ face_counts, int* __restrict__ vertex_counts) {
    __shared__ int s_first;
    int label = -1;
    if ((int64_t)blockIdx.x < blocks_v) {
        const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
        if (v < n_vertices) {
            const int root = parent[v];
            label = vertex_label[root];
            if (root != (int)v) vertex_label[v] = label;
        }
        nf_mc_count_runs(vertex_counts, label, &s_first);
    } else {
        const int64_t f = ((int64_t)blockIdx.x - blocks_v) * nfc::THREADS + threadIdx.x;
        if (f < n_faces) {
            const NfFace t = nf_face(faces, f, n_vertices);
            if (t.valid) label = vertex_label[parent[t.a]];
            face_label[f] = label;
        }
        nf_mc_count_runs(face_counts, label, &s_first);
    }
}

// ---- selection
__device__ __forceinline__ bool nf_mc_keeps(const nfm::Header* __restrict__ h, const int* __restrict__ face_counts, int label) {
    return h->largest ? label == h->best_label : (long long)face_counts[label] >= h->min_faces;
}

// one workgroup over the C components: the largest count and its lowest label (key = count << 32 | ~label, maximised), the number of
// components the rule keeps; the rule itself goes to the header, where k_mc_keep and the emit kernels read it
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_mc_select(const int* __restrict__ face_counts, int largest, long long min_faces,
                                                            nfm::Header* __restrict__ header, long long* __restrict__ counts_out) {
    __shared__ unsigned long long s_key[nfc::SCAN_WAVES];
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    const long long n = header->components;
    unsigned long long key = 0;
    uint32_t kept = 0;
    for (long long c = threadIdx.x; c < n; c += nfc::SCAN_THREADS) {
        const int count = face_counts[c];
        const unsigned long long k = (unsigned long long)(uint32_t)count << 32 | (uint32_t)~(uint32_t)c;
        key = k > key ? k : key;
        kept += (long long)count >= min_faces ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    const uint32_t total = nf_block_total<nfc::SCAN_WAVES>(kept, s_wave);
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nfc::SCAN_WAVES; ++w) key = s_key[w] > key ? s_key[w] : key;
        const bool any = (key >> 32) != 0;                          // some component has a face
        header->largest = largest;
        header->min_faces = min_faces;
        header->best_label = any ? (int)~(uint32_t)key : -1;
        const long long kept_components = largest ? (any ? 1 : 0) : (long long)total;
        header->kept_components = kept_components;
        counts_out[3] = kept_components;
    }
}

// workgroups [0, blocks_v): kept vertices per workgroup, the rest: kept faces per workgroup
__global__ void __launch_bounds__(nfc::THREADS) k_mc_keep(const int* __restrict__ vertex_label, const int* __restrict__ face_label,
                                                          const int* __restrict__ face_counts, int64_t n_vertices, int64_t n_faces, int64_t blocks_v,
                                                          const nfm::Header* __restrict__ header, uint32_t* __restrict__ block_v,
                                                          uint32_t* __restrict__ block_f) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const bool vertices = (int64_t)blockIdx.x < blocks_v;
    const int64_t block = vertices ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - blocks_v;
    const int64_t at = block * nfc::THREADS + threadIdx.x;
    uint32_t keep = 0;
    if (at < (vertices ? n_vertices : n_faces)) {
        const int label = vertices ? vertex_label[at] : face_label[at];
        keep = label >= 0 && nf_mc_keeps(header, face_counts, label) ? 1u : 0u;
    }
    const uint32_t total = nf_block_total<nfc::WAVES>(keep, s_wave);
    if (threadIdx.x == 0) (vertices ? block_v : block_f)[block] = total;
}

// ---- compaction
__global__ void __launch_bounds__(nfc::THREADS) k_mc_emit_verts(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                const int* __restrict__ vertex_label, const int* __restrict__ face_counts,
                                                                int64_t n_vertices, const nfm::Header* __restrict__ header,
                                                                const uint32_t* __restrict__ block_v, int* __restrict__ new_id,
                                                                float* __restrict__ out_vertices, int64_t cap_vertices, float* __restrict__ out_normals) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t keep = v < n_vertices && nf_mc_keeps(header, face_counts, vertex_label[v]) ? 1u : 0u;
    uint32_t total;
    const int64_t id = (int64_t)block_v[blockIdx.x] + nf_block_scan<nfc::WAVES>(keep, s_wave, &total) - keep;
    if (!keep) return;
    new_id[v] = (int)id;
    if (id >= cap_vertices) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[id * 3 + k] = vertices[v * 3 + k];
        if (normals) out_normals[id * 3 + k] = normals[v * 3 + k];
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_mc_emit_faces(const int* __restrict__ faces, const int* __restrict__ face_label,
                                                                const int* __restrict__ face_counts, int64_t n_faces,
                                                                int64_t n_vertices, const nfm::Header* __restrict__ header,
                                                                const uint32_t* __restrict__ block_f, const int* __restrict__ new_id,
                                                                int* __restrict__ out_faces, int64_t cap_faces) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t keep = 0;
    if (f < n_faces) {
        const int label = face_label[f];
        keep = label >= 0 && nf_mc_keeps(header, face_counts, label) ? 1u : 0u;
    }
    uint32_t total;
    const int64_t row = (int64_t)block_f[blockIdx.x] + nf_block_scan<nfc::WAVES>(keep, s_wave, &total) - keep;
    if (!keep || row >= cap_faces) return;
    const NfFace t = nf_face(faces, f, n_vertices);                 // label >= 0 says valid, and its vertices are kept; checked all the same
    out_faces[row * 3 + 0] = t.valid ? new_id[t.a] : -1;
    out_faces[row * 3 + 1] = t.valid ? new_id[t.b] : -1;
    out_faces[row * 3 + 2] = t.valid ? new_id[t.c] : -1;
}

// ---- entry points
extern "C" int nf_mesh_components_label(const int* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                                        int* vertex_label, int* face_label, int* face_counts, int* vertex_counts, int64_t* counts_dev,
                                        nf_stream_t stream) {
    NfMcPlan p;
    if (!workspace || !counts_dev || !nf_mc_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if ((n_faces && (!faces || !face_label)) || (n_vertices && (!vertex_label || !face_counts || !vertex_counts))) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    int* parent = reinterpret_cast<int*>(ws + p.off_parent);
    uint32_t* block_v = reinterpret_cast<uint32_t*>(ws + p.off_block_v);
    const dim3 threads(nfc::THREADS), grid_v((unsigned)p.blocks_v), grid_f((unsigned)p.blocks_f), grid_vf((unsigned)(p.blocks_v + p.blocks_f));
    hipStream_t s = nf_s(stream);
    if (n_vertices) {
        hipLaunchKernelGGL(k_mc_init, grid_v, threads, 0, s, parent, n_vertices);
        if (n_faces) hipLaunchKernelGGL(k_mc_hook, grid_f, threads, 0, s, faces, n_vertices, n_faces, parent);
        hipLaunchKernelGGL(k_mc_flatten, grid_v, threads, 0, s, parent, n_vertices, block_v);
    }
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(nfc::SCAN_THREADS), 0, s, block_v, p.blocks_v, 0, block_v, (int64_t)0, 0, 1,
                       reinterpret_cast<long long*>(ws), reinterpret_cast<long long*>(counts_dev));
    if (n_vertices)
        hipLaunchKernelGGL(k_mc_rank, grid_v, threads, 0, s, parent, n_vertices, block_v, vertex_label, face_counts, vertex_counts);
    if (n_vertices || n_faces)
        hipLaunchKernelGGL(k_mc_labels, grid_vf, threads, 0, s, faces, parent, n_vertices, n_faces, p.blocks_v, vertex_label, face_label, face_counts,
                           vertex_counts);
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_components_select(const int* vertex_label, const int* face_label, const int* face_counts, int64_t n_vertices,
                                         int64_t n_faces, int largest, int64_t min_faces, void* workspace, size_t workspace_bytes,
                                         int64_t* counts_dev, nf_stream_t stream) {
    NfMcPlan p;
    if (!workspace || !counts_dev || !nf_mc_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if ((n_faces && !face_label) || (n_vertices && (!vertex_label || !face_counts))) return NF_EINVAL;
    if ((largest != 0) == (min_faces != 0) || min_faces < 0) return NF_EINVAL;      // exactly one rule: largest, or min_faces >= 1
    char* ws = static_cast<char*>(workspace);
    nfm::Header* header = reinterpret_cast<nfm::Header*>(ws);
    uint32_t* block_v = reinterpret_cast<uint32_t*>(ws + p.off_block_v);
    uint32_t* block_f = reinterpret_cast<uint32_t*>(ws + p.off_block_f);
    hipStream_t s = nf_s(stream);
    hipLaunchKernelGGL(k_mc_select, dim3(1), dim3(nfc::SCAN_THREADS), 0, s, face_counts, largest ? 1 : 0, largest ? (long long)1 : (long long)min_faces,
                       header, reinterpret_cast<long long*>(counts_dev));
    if (n_vertices || n_faces)
        hipLaunchKernelGGL(k_mc_keep, dim3((unsigned)(p.blocks_v + p.blocks_f)), dim3(nfc::THREADS), 0, s, vertex_label, face_label, face_counts, n_vertices,
                           n_faces, p.blocks_v, header, block_v, block_f);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(nfc::SCAN_THREADS), 0, s, block_v, p.blocks_v, 1, block_f, p.blocks_f, 2, 2,
                       reinterpret_cast<long long*>(ws), reinterpret_cast<long long*>(counts_dev));
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_components_emit(const float* vertices, const int* faces, const float* normals, const int* vertex_label,
                                       const int* face_label, const int* face_counts, int64_t n_vertices, int64_t n_faces, void* workspace,
                                       size_t workspace_bytes, float* out_vertices, int64_t cap_vertices, int* out_faces, int64_t cap_faces,
                                       float* out_normals, nf_stream_t stream) {
    NfMcPlan p;
    if (!workspace || !nf_mc_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes) return NF_EINVAL;
    if (cap_vertices < 0 || cap_faces < 0 || cap_vertices > 0x7fffffff || cap_faces > 0x7fffffff) return NF_EINVAL;
    if ((n_faces && (!faces || !face_label)) || (n_vertices && (!vertices || !vertex_label || !face_counts))) return NF_EINVAL;
    if ((cap_vertices && !out_vertices) || (cap_faces && !out_faces) || ((normals != nullptr) != (out_normals != nullptr) && cap_vertices)) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    const nfm::Header* header = reinterpret_cast<const nfm::Header*>(ws);
    int* new_id = reinterpret_cast<int*>(ws + p.off_new_id);
    hipStream_t s = nf_s(stream);
    if (n_vertices)
        hipLaunchKernelGGL(k_mc_emit_verts, dim3((unsigned)p.blocks_v), dim3(nfc::THREADS), 0, s, vertices, out_normals ? normals : nullptr, vertex_label,
                           face_counts, n_vertices, header, reinterpret_cast<const uint32_t*>(ws + p.off_block_v), new_id, out_vertices, cap_vertices,
                           out_normals);
    if (n_faces)
        hipLaunchKernelGGL(k_mc_emit_faces, dim3((unsigned)p.blocks_f), dim3(nfc::THREADS), 0, s, faces, face_label, face_counts, n_faces, n_vertices,
                           header, reinterpret_cast<const uint32_t*>(ws + p.off_block_f), new_id, out_faces, cap_faces);
    NF_RETURN_LAUNCH();
}
