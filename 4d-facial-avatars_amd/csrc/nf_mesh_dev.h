// The face read the units over an indexed triangle mesh share (nf_mesh_components.hip, nf_mesh_smooth.hip).
#pragma once
#include "nf_common.h"

// the three indices of face f (64-bit addressing: 3 * F passes 2^31) and whether all lie in [0, V): range-checked before anything is
// indexed with them
struct NfFace { int a, b, c; bool valid; };

__device__ __forceinline__ NfFace nf_face(const int* __restrict__ faces, int64_t f, int64_t n_vertices) {
    NfFace t;
    t.a = faces[f * 3 + 0], t.b = faces[f * 3 + 1], t.c = faces[f * 3 + 2];
    t.valid = t.a >= 0 && t.a < n_vertices && t.b >= 0 && t.b < n_vertices && t.c >= 0 && t.c < n_vertices;
    return t;
}
