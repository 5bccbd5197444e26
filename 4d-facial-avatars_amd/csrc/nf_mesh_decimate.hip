// Decimation of an indexed triangle mesh by vertex clustering, with welded faces (DESIGN.md "Mesh decimation" is the normative text;
// tests/mesh_decimate_ref.py restates it in NumPy).
//
//   per axis t = (p - o) / c in float32, i = floor(t); a vertex is clustered iff all three t are finite and -2^20 <= i < 2^20, its key
//   (i_x + 2^20) + 2^21 (i_y + 2^20) + 2^42 (i_z + 2^20); rep(v) = the smallest id among the clustered vertices with v's key, v itself
//   for an unclustered one.  A valid face (a, b, c) becomes r = (rep a, rep b, rep c), dropped as degenerate iff two entries are equal;
//   of the faces with one vertex set, p of them even permutations of the ascending triple and m odd ones, none is kept if p = m, else
//   the one of the majority orientation with the smallest face id.  Kept faces stay in their order, each with its own r renumbered by
//   rank among the used representatives.  The position of a used cluster of n > 1 members: per member frac = t - float(i),
//   q = int64(frac * 2^30); S = their exact sum; x = double(o) + double(c) * (double(i) + (double(S) / double(n)) * 2^-30), every
//   double operation rounded on its own, rounded to float32.  One member: its floats, bit for bit.
//
// One thread per vertex, face or table slot, 256 per workgroup.  Two open-addressing hash sets in the workspace, one of cells and one of
// ascending triples of representatives, each of the smallest power of two >= 2 max(n, 128) slots (load <= 0.5):
//   k_md_init        both tables empty, their side words at their neutral values, the accumulators, the used marks and the header zero
//   k_md_keys        key[v] (NOKEY: not clustered); the number of unclustered vertices
//   k_md_cluster     every clustered vertex finds or claims its cell's slot (one 32-bit atomicCAS of the owner word against EMPTY, which
//                    then never changes; whose slot it is, is read from key[owner], written by the kernel before): atomicMin of the
//                    smallest id, atomicAdd of the member count; slot[v]
//   k_md_rep         rep[v] and, in a cluster of more than one, three unsigned 64-bit atomicAdds of q into the accumulators of rep[v];
//                    the largest cluster (atomicMax)
//   k_md_face_keys   tri[f] = the ascending triple of (rep a, rep b, rep c), tri[f][0] = -1 for an invalid or degenerate face; their numbers
//   k_md_face_set    every other face finds or claims its triple's slot (the triple is read from tri[owner]): atomicAdd of its
//                    orientation's count, atomicMin of its orientation's smallest face id; fslot[f]
//   k_md_face_keep   keep[f]; used[r] = 1 for the three entries of a kept face; the number of coincident faces
//   k_md_sum / k_md_scan1   (twice) the block sums of used[] and keep[] and their exclusive prefixes (nf_scan_dev.h); V', F'
//   k_md_counts      the header's eight counts to the caller's
//   k_md_emit_verts  new_id[v] (-1: not used); the position of every used representative
//   k_md_emit_faces  the kept faces, renumbered;  k_md_emit_map  vertex_map[v] = new_id[rep[v]]
// What the result depends on lives in side words updated with integer atomicMin / atomicAdd / atomicMax, so nothing depends on who
// claimed a slot nor on the hash function: two calls give the same bits.  Every probe loop stops after `capacity` slots and raises the
// overflow flag of the header (never at load <= 0.5: a bug ends as an error, not as a hang).  No float atomics, no kernel waits for
// another workgroup, what one kernel writes the next one reads, and every word read was written earlier in the same call: the
// workspace may arrive with any content.
#include <math.h>
#include "nf_mesh_dev.h"
#include "nf_scan_dev.h"

namespace nfd {
constexpr int SCAN_PER_THREAD = 4;                     // k_md_scan1: block sums per thread and round (a round takes 4096 sums: 2^20 elements)
constexpr int RANGE_BITS = 20;                         // cell indices lie in [-2^20, 2^20)
constexpr int64_t MAX_ELEMENTS = (int64_t)1 << 30;     // V and F: ids and both capacities (at most 2^31 slots) fit 31 bits
constexpr int64_t MIN_TABLE = 128;                     // a table is sized for at least this many elements
constexpr int EMPTY = -1;                              // owner word of a free slot
constexpr int NO_ID = 0x7fffffff;                      // neutral value of a smallest-id word
constexpr unsigned long long NOKEY = ~0ull;            // key of a vertex that is not clustered (a key has 63 bits)
// header words (int64): the eight counts in the order nf_mesh_decimate_count reports them
enum { H_VERTS, H_FACES, H_DEGENERATE, H_COINCIDENT, H_INVALID, H_UNCLUSTERED, H_LARGEST, H_OVERFLOW, H_COUNTS };
}  // namespace nfd

// ---- workspace plan
struct NfMdPlan {
    int64_t cap_v, cap_f, blocks_v, blocks_f, blocks_init;
    size_t off_key, off_slot, off_rep, off_acc, off_used, off_new_id, off_block_v, off_v_owner, off_v_min, off_v_count;
    size_t off_tri, off_fslot, off_keep, off_block_f, off_f_owner, off_f_count, off_f_min, bytes;
};

// the smallest power of two >= 2 max(n, MIN_TABLE)
static inline int64_t nf_md_capacity(int64_t n) {
    int64_t cap = 2 * nfd::MIN_TABLE;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

// false: a size the plan does not serve.  Either number may be 0.
static inline bool nf_md_plan(int64_t n_vertices, int64_t n_faces, NfMdPlan* p) {
    if (n_vertices < 0 || n_faces < 0 || n_vertices > nfd::MAX_ELEMENTS || n_faces > nfd::MAX_ELEMENTS) return false;
    p->cap_v = nf_md_capacity(n_vertices);
    p->cap_f = nf_md_capacity(n_faces);
    p->blocks_v = nf_blocks(n_vertices);
    p->blocks_f = nf_blocks(n_faces);
    int64_t most = p->cap_v > p->cap_f ? p->cap_v : p->cap_f;
    if (3 * n_vertices > most) most = 3 * n_vertices;
    p->blocks_init = nf_blocks(most);
    const size_t v = (size_t)n_vertices, f = (size_t)n_faces, cv = (size_t)p->cap_v, cf = (size_t)p->cap_f;
    NfWorkspace ws;
    p->off_key = ws.take(v * 8);                                    // the cell key of every vertex
    p->off_slot = ws.take(v * 4);                                   // its cell's slot, -1: not clustered
    p->off_rep = ws.take(v * 4);
    p->off_acc = ws.take(v * 24);                                   // S per axis, at the representative
    p->off_used = ws.take(v * 4);
    p->off_new_id = ws.take(v * 4);
    p->off_block_v = ws.take((size_t)p->blocks_v * 4);
    p->off_v_owner = ws.take(cv * 4);
    p->off_v_min = ws.take(cv * 4);
    p->off_v_count = ws.take(cv * 4);
    p->off_tri = ws.take(f * 12);                                   // the ascending triple of every face
    p->off_fslot = ws.take(f * 4);
    p->off_keep = ws.take(f * 4);
    p->off_block_f = ws.take((size_t)p->blocks_f * 4);
    p->off_f_owner = ws.take(cf * 4);
    p->off_f_count = ws.take(cf * 8);                               // even, odd
    p->off_f_min = ws.take(cf * 8);                                 // even, odd
    p->bytes = ws.at;
    return true;
}

extern "C" size_t nf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    NfMdPlan p;
    return nf_md_plan(n_vertices, n_faces, &p) ? p.bytes : 0;
}

// ---- device helpers
struct NfMdGrid { float ox, oy, oz, cx, cy, cz; };

__device__ __forceinline__ uint64_t nf_md_mix(uint64_t x) {         // any hash serves: the results do not depend on it
    x ^= x >> 33, x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33, x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// t = (p - o) / c and floor(t) of one axis; false: not finite or outside [-2^20, 2^20)
__device__ __forceinline__ bool nf_md_axis(float p, float o, float c, float* t, float* low) {
    *t = nf_div(nf_sub(p, o), c);
    *low = floorf(*t);
    const float range = (float)(1 << nfd::RANGE_BITS);
    return fabsf(*t) < INFINITY && *low >= -range && *low < range;  // NaN fails the first
}

__device__ __forceinline__ void nf_md_raise(unsigned long long* header, int word) { atomicMax(header + word, 1ull); }

// the owner of slot s, claiming a free one for `id`: the one atomicCAS of a slot's life
__device__ __forceinline__ int nf_md_owner(int* owner, uint32_t s, int id) {
    int o = __hip_atomic_load(owner + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == nfd::EMPTY) {
        o = atomicCAS(owner + s, nfd::EMPTY, id);
        if (o == nfd::EMPTY) o = id;
    }
    return o;
}

// ---- count
__global__ void __launch_bounds__(nfc::THREADS) k_md_init(int64_t cap_v, int64_t cap_f, int64_t n_vertices, int* __restrict__ v_owner, int* __restrict__ v_min,
                                                          int* __restrict__ v_count, int* __restrict__ f_owner, int* __restrict__ f_count,
                                                          int* __restrict__ f_min, unsigned long long* __restrict__ acc, int* __restrict__ used,
                                                          unsigned long long* __restrict__ header) {
    const int64_t i = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (i < cap_v) v_owner[i] = nfd::EMPTY, v_min[i] = nfd::NO_ID, v_count[i] = 0;
    if (i < cap_f) {
        f_owner[i] = nfd::EMPTY;
        f_count[i * 2 + 0] = 0, f_count[i * 2 + 1] = 0;
        f_min[i * 2 + 0] = nfd::NO_ID, f_min[i * 2 + 1] = nfd::NO_ID;
    }
    if (i < n_vertices * 3) acc[i] = 0ull;
    if (i < n_vertices) used[i] = 0;
    if (i < nfc::HEADER / 8) header[i] = 0ull;
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_keys(const float* __restrict__ vertices, int64_t n_vertices, NfMdGrid g,
                                                          unsigned long long* __restrict__ key, unsigned long long* __restrict__ header) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t loose = 0;
    if (v < n_vertices) {
        float t, lx, ly, lz;
        bool ok = nf_md_axis(vertices[v * 3 + 0], g.ox, g.cx, &t, &lx);
        ok = nf_md_axis(vertices[v * 3 + 1], g.oy, g.cy, &t, &ly) && ok;
        ok = nf_md_axis(vertices[v * 3 + 2], g.oz, g.cz, &t, &lz) && ok;
        const int64_t bias = (int64_t)1 << nfd::RANGE_BITS;
        unsigned long long k = nfd::NOKEY;
        if (ok) k = (unsigned long long)((int64_t)lx + bias) | (unsigned long long)((int64_t)ly + bias) << 21 | (unsigned long long)((int64_t)lz + bias) << 42;
        key[v] = k;
        loose = ok ? 0u : 1u;
    }
    const uint32_t total = nf_block_total<nfc::WAVES>(loose, s_wave);
    if (threadIdx.x == 0 && total) atomicAdd(header + nfd::H_UNCLUSTERED, (unsigned long long)total);
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_cluster(const unsigned long long* __restrict__ key, int64_t n_vertices, int64_t cap, int* v_owner,
                                                             int* v_min, int* v_count, int* __restrict__ slot, unsigned long long* header) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const unsigned long long k = key[v];
    int found = -1;
    if (k != nfd::NOKEY) {
        const uint32_t mask = (uint32_t)(cap - 1);
        uint32_t s = (uint32_t)nf_md_mix(k) & mask;
        for (int64_t tries = 0; tries < cap; ++tries, s = (s + 1) & mask) {
            const int o = nf_md_owner(v_owner, s, (int)v);
            if (o < 0 || o >= n_vertices) break;                    // no slot holds another word: nothing is indexed with it all the same
            if (key[o] == k) {
                found = (int)s;
                break;
            }
        }
        if (found < 0) nf_md_raise(header, nfd::H_OVERFLOW);
        else atomicMin(v_min + found, (int)v), atomicAdd(v_count + found, 1);
    }
    slot[v] = found;
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_rep(const float* __restrict__ vertices, int64_t n_vertices, NfMdGrid g, const int* __restrict__ slot,
                                                         const int* __restrict__ v_min, const int* __restrict__ v_count, int* __restrict__ rep,
                                                         unsigned long long* acc, unsigned long long* header) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    int members = 0;
    if (v < n_vertices) {
        const int s = slot[v];
        int r = (int)v;
        members = 1;
        if (s >= 0) {
            r = v_min[s], members = v_count[s];
            if (r < 0 || r >= n_vertices) r = (int)v;               // never: the smallest id of a claimed slot is a member's
        }
        rep[v] = r;
        if (s >= 0 && members > 1) {
            const float o[3] = {g.ox, g.oy, g.oz}, c[3] = {g.cx, g.cy, g.cz};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float t, low;
                nf_md_axis(vertices[v * 3 + a], o[a], c[a], &t, &low);
                const float frac = nf_sub(t, low);                  // low is float(i)
                const long long q = (long long)nf_mul(frac, 1073741824.f);             // exact scaling; the conversion truncates
                atomicAdd(acc + (int64_t)r * 3 + a, (unsigned long long)q);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(members, o, 64);
        members = other > members ? other : members;
    }
    if ((threadIdx.x & 63) == 0 && members > 0) atomicMax(header + nfd::H_LARGEST, (unsigned long long)members);
}

// r = (rep a, rep b, rep c) of a valid face and its ascending triple; returns whether r is an even permutation of it
__device__ __forceinline__ bool nf_md_sorted(int ra, int rb, int rc, int* s0, int* s1, int* s2) {
    int x = ra, y = rb, z = rc;
    bool even = true;
    if (x > y) { const int w = x; x = y, y = w, even = !even; }
    if (y > z) { const int w = y; y = z, z = w, even = !even; }
    if (x > y) { const int w = x; x = y, y = w, even = !even; }
    *s0 = x, *s1 = y, *s2 = z;
    return even;
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_face_keys(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces,
                                                               const int* __restrict__ rep, int* __restrict__ tri, unsigned long long* header) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t invalid = 0, degenerate = 0;
    if (f < n_faces) {
        const NfFace t = nf_face(faces, f, n_vertices);             // range-checked before anything is indexed
        int s0 = -1, s1 = -1, s2 = -1;
        if (!t.valid) invalid = 1;
        else {
            const int ra = rep[t.a], rb = rep[t.b], rc = rep[t.c];
            if (ra == rb || rb == rc || rc == ra) degenerate = 1;
            else nf_md_sorted(ra, rb, rc, &s0, &s1, &s2);
        }
        tri[f * 3 + 0] = s0, tri[f * 3 + 1] = s1, tri[f * 3 + 2] = s2;
    }
    const uint32_t n_invalid = nf_block_total<nfc::WAVES>(invalid, s_wave);
    const uint32_t n_degenerate = nf_block_total<nfc::WAVES>(degenerate, s_wave);
    if (threadIdx.x == 0 && n_invalid) atomicAdd(header + nfd::H_INVALID, (unsigned long long)n_invalid);
    if (threadIdx.x == 0 && n_degenerate) atomicAdd(header + nfd::H_DEGENERATE, (unsigned long long)n_degenerate);
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_face_set(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, const int* __restrict__ rep,
                                                              const int* __restrict__ tri, int64_t cap, int* f_owner, int* f_count, int* f_min,
                                                              int* __restrict__ fslot, unsigned long long* header) {
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const int s0 = tri[f * 3 + 0], s1 = tri[f * 3 + 1], s2 = tri[f * 3 + 2];
    int found = -1;
    if (s0 >= 0) {
        const NfFace t = nf_face(faces, f, n_vertices);             // valid: its triple says so
        int x, y, z;
        const int odd = nf_md_sorted(rep[t.a], rep[t.b], rep[t.c], &x, &y, &z) ? 0 : 1;
        const uint32_t mask = (uint32_t)(cap - 1);
        uint32_t s = (uint32_t)nf_md_mix(((uint64_t)(uint32_t)s0 << 32 | (uint32_t)s1) ^ nf_md_mix((uint64_t)(uint32_t)s2)) & mask;
        for (int64_t tries = 0; tries < cap; ++tries, s = (s + 1) & mask) {
            const int64_t o = nf_md_owner(f_owner, s, (int)f);
            if (o < 0 || o >= n_faces) break;
            if (tri[o * 3 + 0] == s0 && tri[o * 3 + 1] == s1 && tri[o * 3 + 2] == s2) {
                found = (int)s;
                break;
            }
        }
        if (found < 0) nf_md_raise(header, nfd::H_OVERFLOW);
        else atomicAdd(f_count + (int64_t)found * 2 + odd, 1), atomicMin(f_min + (int64_t)found * 2 + odd, (int)f);
    }
    fslot[f] = found;
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_face_keep(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, const int* __restrict__ rep,
                                                               const int* __restrict__ fslot, const int* __restrict__ f_count, const int* __restrict__ f_min,
                                                               int* __restrict__ keep, int* used, unsigned long long* header) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    uint32_t gone = 0;
    if (f < n_faces) {
        const int64_t s = fslot[f];
        int kept = 0;
        if (s >= 0) {
            const int even = f_count[s * 2 + 0], odd = f_count[s * 2 + 1];
            const int winner = even > odd ? f_min[s * 2 + 0] : odd > even ? f_min[s * 2 + 1] : -1;
            kept = winner == (int)f ? 1 : 0;
            gone = 1 - kept;
            if (kept) {
                const NfFace t = nf_face(faces, f, n_vertices);
                used[rep[t.a]] = 1, used[rep[t.b]] = 1, used[rep[t.c]] = 1;            // every writer stores the same word
            }
        }
        keep[f] = kept;
    }
    const uint32_t total = nf_block_total<nfc::WAVES>(gone, s_wave);
    if (threadIdx.x == 0 && total) atomicAdd(header + nfd::H_COINCIDENT, (unsigned long long)total);
}

// the sum of every workgroup's 256 flags ...
__global__ void __launch_bounds__(nfc::THREADS) k_md_sum(const int* __restrict__ x, int64_t n, uint32_t* __restrict__ block) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t i = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t total = nf_block_total<nfc::WAVES>(i < n ? (uint32_t)x[i] : 0u, s_wave);
    if (threadIdx.x == 0) block[blockIdx.x] = total;
}

// ... and one workgroup: the block sums -> their exclusive prefixes in place, the total to the header
__global__ void __launch_bounds__(nfc::SCAN_THREADS) k_md_scan1(uint32_t* __restrict__ a, int64_t n_blocks, unsigned long long* __restrict__ header_slot) {
    __shared__ uint32_t s_wave[nfc::SCAN_WAVES];
    const uint32_t carry = nf_scan_block_sums<nfd::SCAN_PER_THREAD>(a, n_blocks, s_wave);
    if (threadIdx.x == 0) *header_slot = (unsigned long long)carry;
}

__global__ void k_md_counts(const unsigned long long* __restrict__ header, long long* __restrict__ counts) {
    if (threadIdx.x < nfd::H_COUNTS) counts[threadIdx.x] = (long long)header[threadIdx.x];
}

// ---- emit
__global__ void __launch_bounds__(nfc::THREADS) k_md_emit_verts(const float* __restrict__ vertices, int64_t n_vertices, NfMdGrid g, const int* __restrict__ slot,
                                                                const int* __restrict__ v_count, const unsigned long long* __restrict__ acc,
                                                                const int* __restrict__ used, const uint32_t* __restrict__ block,
                                                                int* __restrict__ new_id, float* __restrict__ out, int64_t n_out) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t mine = v < n_vertices ? (uint32_t)used[v] : 0u;
    uint32_t total;
    const int64_t at = (int64_t)block[blockIdx.x] + nf_block_scan<nfc::WAVES>(mine, s_wave, &total) - mine;
    if (v >= n_vertices) return;
    new_id[v] = mine ? (int)at : -1;
    if (!mine || at >= n_out) return;                               // n_out = V': checked by the entry point
    const int s = slot[v];
    const int members = s >= 0 ? v_count[s] : 1;
    const float o[3] = {g.ox, g.oy, g.oz}, c[3] = {g.cx, g.cy, g.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = vertices[v * 3 + a];
        float x = p;
        if (members > 1) {
            float t, low;
            nf_md_axis(p, o[a], c[a], &t, &low);                    // the representative is a member: its cell is the cluster's
            const double m = __ddiv_rn((double)acc[v * 3 + a], (double)members);
            const double inside = __dadd_rn((double)low, __dmul_rn(m, 0x1p-30));
            x = __double2float_rn(__dadd_rn((double)o[a], __dmul_rn((double)c[a], inside)));
        }
        out[at * 3 + a] = x;
    }
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_emit_faces(const int* __restrict__ faces, int64_t n_vertices, int64_t n_faces, const int* __restrict__ rep,
                                                                const int* __restrict__ keep, const uint32_t* __restrict__ block,
                                                                const int* __restrict__ new_id, int* __restrict__ out, int64_t n_out) {
    __shared__ uint32_t s_wave[nfc::WAVES];
    const int64_t f = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    const uint32_t mine = f < n_faces ? (uint32_t)keep[f] : 0u;
    uint32_t total;
    const int64_t at = (int64_t)block[blockIdx.x] + nf_block_scan<nfc::WAVES>(mine, s_wave, &total) - mine;
    if (!mine || at >= n_out) return;
    const NfFace t = nf_face(faces, f, n_vertices);                 // kept: valid
    out[at * 3 + 0] = new_id[rep[t.a]], out[at * 3 + 1] = new_id[rep[t.b]], out[at * 3 + 2] = new_id[rep[t.c]];
}

__global__ void __launch_bounds__(nfc::THREADS) k_md_emit_map(const int* __restrict__ rep, const int* __restrict__ new_id, int64_t n_vertices,
                                                              int* __restrict__ vertex_map) {
    const int64_t v = (int64_t)blockIdx.x * nfc::THREADS + threadIdx.x;
    if (v < n_vertices) vertex_map[v] = new_id[rep[v]];
}

// ---- entry points
// what both entry points refuse alike; on success the grid's six floats
static inline bool nf_md_grid(const float* origin, const float* cell, NfMdGrid* g) {
    if (!origin || !cell) return false;
    for (int a = 0; a < 3; ++a)
        if (!(fabsf(origin[a]) < INFINITY) || !(cell[a] > 0.f) || !(cell[a] < INFINITY)) return false;          // NaN fails each
    g->ox = origin[0], g->oy = origin[1], g->oz = origin[2];
    g->cx = cell[0], g->cy = cell[1], g->cz = cell[2];
    return true;
}

extern "C" int nf_mesh_decimate_count(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                                      const float* cell, void* workspace, size_t workspace_bytes, int64_t* counts_dev, nf_stream_t stream) {
    NfMdPlan p;
    NfMdGrid g;
    if (!workspace || !counts_dev || !nf_md_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes || !nf_md_grid(origin, cell, &g)) return NF_EINVAL;
    if ((n_vertices && !vertices) || (n_faces && !faces)) return NF_EINVAL;
    char* ws = static_cast<char*>(workspace);
    unsigned long long* header = reinterpret_cast<unsigned long long*>(ws);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(ws + p.off_key);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + p.off_acc);
    auto ints = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
    int *slot = ints(p.off_slot), *rep = ints(p.off_rep), *used = ints(p.off_used), *v_owner = ints(p.off_v_owner), *v_min = ints(p.off_v_min);
    int *v_count = ints(p.off_v_count), *tri = ints(p.off_tri), *fslot = ints(p.off_fslot), *keep = ints(p.off_keep), *f_owner = ints(p.off_f_owner);
    int *f_count = ints(p.off_f_count), *f_min = ints(p.off_f_min);
    uint32_t* block_v = reinterpret_cast<uint32_t*>(ws + p.off_block_v);
    uint32_t* block_f = reinterpret_cast<uint32_t*>(ws + p.off_block_f);
    const dim3 threads(nfc::THREADS), grid_v((unsigned)p.blocks_v), grid_f((unsigned)p.blocks_f), one(1), scan(nfc::SCAN_THREADS);
    hipStream_t s = nf_s(stream);
    hipLaunchKernelGGL(k_md_init, dim3((unsigned)p.blocks_init), threads, 0, s, p.cap_v, p.cap_f, n_vertices, v_owner, v_min, v_count, f_owner, f_count, f_min,
                       acc, used, header);
    if (n_vertices) {
        hipLaunchKernelGGL(k_md_keys, grid_v, threads, 0, s, vertices, n_vertices, g, key, header);
        hipLaunchKernelGGL(k_md_cluster, grid_v, threads, 0, s, key, n_vertices, p.cap_v, v_owner, v_min, v_count, slot, header);
        hipLaunchKernelGGL(k_md_rep, grid_v, threads, 0, s, vertices, n_vertices, g, slot, v_min, v_count, rep, acc, header);
    }
    if (n_faces) {
        hipLaunchKernelGGL(k_md_face_keys, grid_f, threads, 0, s, faces, n_vertices, n_faces, rep, tri, header);
        hipLaunchKernelGGL(k_md_face_set, grid_f, threads, 0, s, faces, n_vertices, n_faces, rep, tri, p.cap_f, f_owner, f_count, f_min, fslot, header);
        hipLaunchKernelGGL(k_md_face_keep, grid_f, threads, 0, s, faces, n_vertices, n_faces, rep, fslot, f_count, f_min, keep, used, header);
    }
    if (n_vertices) hipLaunchKernelGGL(k_md_sum, grid_v, threads, 0, s, used, n_vertices, block_v);
    hipLaunchKernelGGL(k_md_scan1, one, scan, 0, s, block_v, p.blocks_v, header + nfd::H_VERTS);
    if (n_faces) hipLaunchKernelGGL(k_md_sum, grid_f, threads, 0, s, keep, n_faces, block_f);
    hipLaunchKernelGGL(k_md_scan1, one, scan, 0, s, block_f, p.blocks_f, header + nfd::H_FACES);
    hipLaunchKernelGGL(k_md_counts, one, dim3(NF_WAVE), 0, s, header, reinterpret_cast<long long*>(counts_dev));
    NF_RETURN_LAUNCH();
}

extern "C" int nf_mesh_decimate_emit(const float* vertices, const int* faces, int64_t n_vertices, int64_t n_faces, const float* origin, const float* cell,
                                     void* workspace, size_t workspace_bytes, float* out_vertices, int64_t n_out_vertices, int* out_faces,
                                     int64_t n_out_faces, int* vertex_map, nf_stream_t stream) {
    NfMdPlan p;
    NfMdGrid g;
    if (!workspace || !nf_md_plan(n_vertices, n_faces, &p) || workspace_bytes < p.bytes || !nf_md_grid(origin, cell, &g)) return NF_EINVAL;
    if ((n_vertices && (!vertices || !vertex_map)) || (n_faces && !faces)) return NF_EINVAL;
    if (n_out_vertices < 0 || n_out_vertices > n_vertices || n_out_faces < 0 || n_out_faces > n_faces) return NF_EINVAL;
    if ((n_out_vertices && !out_vertices) || (n_out_faces && !out_faces)) return NF_EINVAL;
    if (!n_vertices) return n_out_faces ? NF_EINVAL : 0;            // nothing is kept of no vertices, and there is no map to write
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = nf_s(stream);
    // the counts live on the device: read V' and F' as `count` left them, and write nothing if the outputs were sized for other numbers
    long long found[2] = {-1, -1};
    hipError_t e = hipMemcpyAsync(found, ws, sizeof(found), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return (int)e;
    if (found[0] != n_out_vertices || found[1] != n_out_faces) return NF_EINVAL;
    auto ints = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
    int *rep = ints(p.off_rep), *new_id = ints(p.off_new_id);
    const dim3 threads(nfc::THREADS), grid_v((unsigned)p.blocks_v), grid_f((unsigned)p.blocks_f);
    hipLaunchKernelGGL(k_md_emit_verts, grid_v, threads, 0, s, vertices, n_vertices, g, ints(p.off_slot), ints(p.off_v_count),
                       reinterpret_cast<const unsigned long long*>(ws + p.off_acc), ints(p.off_used), reinterpret_cast<const uint32_t*>(ws + p.off_block_v),
                       new_id, out_vertices, n_out_vertices);
    if (n_out_faces)
        hipLaunchKernelGGL(k_md_emit_faces, grid_f, threads, 0, s, faces, n_vertices, n_faces, rep, ints(p.off_keep),
                           reinterpret_cast<const uint32_t*>(ws + p.off_block_f), new_id, out_faces, n_out_faces);
    hipLaunchKernelGGL(k_md_emit_map, grid_v, threads, 0, s, rep, new_id, n_vertices, vertex_map);
    NF_RETURN_LAUNCH();
}
