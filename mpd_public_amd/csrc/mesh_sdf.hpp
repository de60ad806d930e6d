// mesh_sdf.hpp - a signed-distance grid from a triangle mesh on the device: every grid node against every triangle (mpdx_sdf_grid_from_mesh in
// k_grid.hip; the arithmetic is stated in include/mpdx.h and restated in fp64 numpy in tests/mesh_ref.py).  Replaces nothing in the reference: its
// environments are primitives.  The gradient plane is written afterwards by grid_gradient_kernel<3> (grid_field.hpp) from the finished sdf plane.
//
// One kernel, 256 threads per workgroup, MESH_NPT nodes per thread (node k of a thread = first node of the workgroup + k * 256 + thread: coalesced
// stores); one LDS read of a triangle serves MESH_NPT node-triangle pairs.  MESH_NPT = 1 as measured: a pair is about 290 instructions (160 without
// the winding number) against three LDS reads, so the reads are not what limits, and more nodes per thread cost registers (66 / 94 / 154 / 256 at
// 1 / 2 / 4 / 8 in the winding variant: 7 / 5 / 3 / 1 waves per SIMD) and leave the launches of a split call with too few workgroups - 189 / 174 /
// 144 / 88 G pairs per second (profiles/mesh_sdf_probe.md).  The faces are gathered from vertices / faces into an LDS tile of MESH_TILE records of
// 12 floats, read back as three 16-byte loads at an address every lane shares (a broadcast: no bank conflicts):
//   words 0-8   the vertices a, b, c as they are stored.  (NOT a, ab, ac: the winding number needs b - p and c - p computed the same way in every face
//               that shares the vertex - from a + ab the rounding differs from face to face and a node close to a mesh vertex sees slivers between
//               the faces.  The distance part takes ab = (b - p) - (a - p): six subtractions per pair.)
//   word 9      bias, added to the pair's squared distance: 0 for a face, +inf for a SKIPPED face
//   word 10     weight of the pair's solid angle: 1 for a face, 0 for a skipped one
//   word 11     spare
// A face with an index outside [0, n_vertices) or a non-finite vertex is skipped while staging - always, not as a debug option: its record is
// a = b = c = 0 (finite arithmetic throughout) with bias = +inf and weight 0, which gives d2 = +inf and a solid angle of exactly 0 through the same
// instructions as any other face.  No vertex is read through an index that was not checked.
// Per pair: the vertices relative to the node (A = a - p, ...: the rounding is relative to the node's distance from the vertex, not to the
// coordinates), Ericson's region test for the closest point cp of the closed triangle to the origin of that frame, d2 = cp . cp - the distance FROM
// THE CLOSEST POINT, so its error stays linear in the rounding even for a node in the triangle's plane - and, in the winding variant, Van Oosterom
// and Strackee's solid angle.  The best d2 is kept with fminf (a NaN from a degenerate face never wins); the solid angles are summed in fp32 per
// thread in face order (deterministic); one sqrtf per node at the end, where the sdf plane (and wind_out) is written.
// No atomics; nothing is allocated; no synchronisation with the host; no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpdx.h"
#include "grid_field.hpp"   // grid_f32x4

namespace mpdx {

// tile and nodes per thread: decided by tools/mesh_probe.py (profiles/mesh_sdf_probe.md); a build with other values is an A/B build (MPDX_BUILD_DEFS)
#ifndef MPDX_MESH_TILE
#define MPDX_MESH_TILE 256
#endif
#ifndef MPDX_MESH_NPT
#define MPDX_MESH_NPT 1
#endif
constexpr int MESH_TILE = MPDX_MESH_TILE;   // faces per LDS tile (12 KB at 256)
constexpr int MESH_NPT = MPDX_MESH_NPT;     // nodes per thread
constexpr int MESH_BLOCK_NODES = 256 * MESH_NPT;
static_assert(MESH_TILE >= 1 && MESH_TILE * 48 <= 64 * 1024 && MESH_NPT >= 1 && MESH_NPT <= 8, "mesh tile / nodes per thread");

struct MeshArgs {
    const float* vertices;   // [V][3]
    const int32_t* faces;    // [F][3]
    float* sdf;              // [nodes]
    float* wind;             // [nodes] or null
    int n_vertices, n_faces;
    int n[3];
    int node_begin, node_end;   // this launch's node range (the host splits the grid so that no launch exceeds 2^33 pairs)
    float origin[3], cell, inflate;
};

// one node-triangle pair.  p = the node, (a, b, c) = the record's vertices; best <- fminf(best, d2 + bias); wsum += weight * atan2f(...) (Omega / 2)
template <bool WIND>
__device__ __forceinline__ void mesh_pair(const float p[3], const float a[3], const float b[3], const float c[3], float bias, float weight, float& best, float& wsum) {
    float A[3], B[3], C[3], ab[3], ac[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        A[j] = a[j] - p[j]; B[j] = b[j] - p[j]; C[j] = c[j] - p[j];
        ab[j] = B[j] - A[j]; ac[j] = C[j] - A[j];
    }
    // Ericson, Real-Time Collision Detection 5.1.5, for the point 0 of this frame: ap = -A, bp = -B, cp = -C
    const float d1 = -(ab[0] * A[0] + ab[1] * A[1] + ab[2] * A[2]), d2 = -(ac[0] * A[0] + ac[1] * A[1] + ac[2] * A[2]);
    const float d3 = -(ab[0] * B[0] + ab[1] * B[1] + ab[2] * B[2]), d4 = -(ac[0] * B[0] + ac[1] * B[1] + ac[2] * B[2]);
    const float d5 = -(ab[0] * C[0] + ab[1] * C[1] + ab[2] * C[2]), d6 = -(ac[0] * C[0] + ac[1] * C[1] + ac[2] * C[2]);
    const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
    const float e43 = d4 - d3, e56 = d5 - d6;
    // closest point = base + u1 * (n1 / den) + ac * (n2 / den); the regions are tried from the last of Ericson's order to the first, so that the first
    // one that holds wins, as in the book: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, the face
    float base[3] = {A[0], A[1], A[2]}, u1[3] = {ab[0], ab[1], ab[2]};
    float n1 = vb, n2 = vc, den = va + vb + vc;
    const bool r_bc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
    const bool r_ac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
    const bool r_c = d6 >= 0.f && d5 <= d6;
    const bool r_ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
    const bool r_b = d3 >= 0.f && d4 <= d3;
    const bool r_a = d1 <= 0.f && d2 <= 0.f;
    if (r_bc) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { base[j] = B[j]; u1[j] = C[j] - B[j]; }
        n1 = e43; n2 = 0.f; den = e43 + e56;
    }
    if (r_ac) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { base[j] = A[j]; u1[j] = ac[j]; }
        n1 = d2; n2 = 0.f; den = d2 - d6;
    }
    if (r_ab) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { base[j] = A[j]; u1[j] = ab[j]; }
        n1 = d1; n2 = 0.f; den = d1 - d3;
    }
    // the vertices override the edges; vertex c yields to edge ab, which precedes it in the book's order
    const bool r_v = r_a || r_b || (r_c && !r_ab);
    if (r_v) {
#pragma unroll
        for (int j = 0; j < 3; ++j) base[j] = r_a ? A[j] : r_b ? B[j] : C[j];
        n1 = 0.f; n2 = 0.f; den = 1.f;
    }
    const float inv = 1.0f / den, t1 = n1 * inv, t2 = n2 * inv;
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = base[j] + u1[j] * t1 + ac[j] * t2;
    best = fminf(best, (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + bias);
    if (WIND) {
        const float la = sqrtf(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]), lb = sqrtf(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]),
                    lc = sqrtf(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
        const float det = A[0] * (B[1] * C[2] - B[2] * C[1]) + A[1] * (B[2] * C[0] - B[0] * C[2]) + A[2] * (B[0] * C[1] - B[1] * C[0]);
        const float AB = A[0] * B[0] + A[1] * B[1] + A[2] * B[2], BC = B[0] * C[0] + B[1] * C[1] + B[2] * C[2],
                    CA = C[0] * A[0] + C[1] * A[1] + C[2] * A[2];
        wsum += weight * atan2f(det, la * lb * lc + AB * lc + BC * la + CA * lb);
    }
}

// grid = ceil((node_end - node_begin) / MESH_BLOCK_NODES)
template <bool WIND>
__global__ __launch_bounds__(256) void mesh_sdf_kernel(const MeshArgs m) {
    __shared__ grid_f32x4 tile[MESH_TILE * 3];
    const int nx = m.n[0], ny = m.n[1];
    float p[MESH_NPT][3], best[MESH_NPT], wsum[MESH_NPT];
    int node[MESH_NPT];
#pragma unroll
    for (int k = 0; k < MESH_NPT; ++k) {
        node[k] = m.node_begin + blockIdx.x * MESH_BLOCK_NODES + k * 256 + threadIdx.x;
        const int q = min(node[k], m.node_end - 1);                 // a node past the range computes the last one's value and stores nothing
        const int id[3] = {q % nx, (q / nx) % ny, q / (nx * ny)};
#pragma unroll
        for (int j = 0; j < 3; ++j) p[k][j] = __fadd_rn(m.origin[j], __fmul_rn((float)id[j], m.cell));
        best[k] = __builtin_inff();
        wsum[k] = 0.f;
    }
    for (int f0 = 0; f0 < m.n_faces; f0 += MESH_TILE) {
        const int count = min(MESH_TILE, m.n_faces - f0);           // (uniform over the workgroup)
        __syncthreads();                                              // the previous tile has been read
        for (int i = threadIdx.x; i < count; i += 256) {
            const int32_t* fi = m.faces + 3 * (size_t)(f0 + i);
            const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
            float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            bool ok = (unsigned)i0 < (unsigned)m.n_vertices && (unsigned)i1 < (unsigned)m.n_vertices && (unsigned)i2 < (unsigned)m.n_vertices;
            if (ok) {                                                 // only checked indices reach the vertex array
                const int idx[3] = {i0, i1, i2};
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    v[e] = m.vertices[3 * (size_t)idx[e / 3] + e % 3];
                    ok = ok && fabsf(v[e]) < __builtin_inff();        // (false for NaN)
                }
            }
            if (!ok) {
#pragma unroll
                for (int e = 0; e < 9; ++e) v[e] = 0.f;
            }
            tile[3 * i + 0] = (grid_f32x4){v[0], v[1], v[2], v[3]};
            tile[3 * i + 1] = (grid_f32x4){v[4], v[5], v[6], v[7]};
            tile[3 * i + 2] = (grid_f32x4){v[8], ok ? 0.f : __builtin_inff(), ok ? 1.f : 0.f, 0.f};
        }
        __syncthreads();
        for (int f = 0; f < count; ++f) {
            const grid_f32x4 r0 = tile[3 * f], r1 = tile[3 * f + 1], r2 = tile[3 * f + 2];
            const float a[3] = {r0.x, r0.y, r0.z}, b[3] = {r0.w, r1.x, r1.y}, c[3] = {r1.z, r1.w, r2.x};
#pragma unroll
            for (int k = 0; k < MESH_NPT; ++k) mesh_pair<WIND>(p[k], a, b, c, r2.y, r2.z, best[k], wsum[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < MESH_NPT; ++k) {
        if (node[k] >= m.node_end) continue;
        const float d = sqrtf(best[k]);                               // IEEE sqrtf, once per node
        float s = d;
        if (WIND) {
            const float w = wsum[k] * 0.15915494309189535f;           // sum of Omega / 2 over 2 pi = sum of Omega over 4 pi
            if (m.wind) m.wind[node[k]] = w;
            s = w > 0.5f ? -d : d;
        }
        m.sdf[node[k]] = __fsub_rn(s, m.inflate);
    }
}

}  // namespace mpdx
