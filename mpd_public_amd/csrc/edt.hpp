// edt.hpp - an exact Euclidean distance transform on the device: an occupancy grid (or a point cloud voxelised here) becomes the sdf and gradient
// planes the MPDX_FIELD_GRID lookups of grid_field.hpp read (mpdx_sdf_grid_from_occupancy, mpdx_occupancy_from_points in k_grid.hip; the arithmetic is
// stated in include/mpdx.h and restated as brute-force numpy in tests/edt_ref.py).  Replaces nothing in the reference: its environments are primitives.
//
// Two squared-distance planes travel through the separable passes in the caller's workspace, ws = [2][nz][ny][nx] int32: plane 0 = distance to the
// nearest OCCUPIED node, plane 1 = to the nearest FREE node.  A node's own side gives 0 in the other plane, so the signed-side value is plane 0 at a
// free node and plane 1 at an occupied one.  `none` = (nx + ny + nz)^2 stands for "no seed": it exceeds every distance inside the grid, so a real
// candidate always beats it, and none + 4095^2 < 2^31.
//   pass x   one wave per row: the row's occupancy as 64-bit ballots in LDS (occupied words and free words), then per node the nearest set bit to
//            either side with count-leading / count-trailing zeros - no scan, and x stays the lane index (coalesced byte loads, coalesced stores).
//   pass y/z one workgroup per [line][x-chunk] tile of one plane, staged in LDS (x fastest: the rows of the tile are coalesced loads).  The chunk is the
//            widest power of two <= 64 with line * chunk <= 12288 ints = 48 KB (2 wide at the cap of 4096), narrowed down to 4 while the launch has
//            fewer than 1024 workgroups: a node far from every seed walks that far, so a small grid needs its nodes spread over the CUs
//            (2-D workspace at 1 cm: 378 -> 40 us per transform together with the four-distance trips, profiles/edt_probe.md).
//            Per node the minimum of g(y')^2 + (y - y')^2 walks outward from the node, four distances per trip (eight independent LDS reads),
//            and stops at (y - y')^2 >= best.  In place: a workgroup reads its tile before the barrier, writes it after, and no other
//            workgroup touches those nodes.
//   final    one thread per node: s from d2 in fp32, every step rounded (the single-operation intrinsics: the build's -ffp-contract=on fuses
//            within an expression only), then - a second launch, grid_gradient_kernel of grid_field.hpp - the gradient plane as differences of s,
//            one 16-byte store per node.
// No atomics; nothing is allocated; no synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpdx.h"
#include "grid_field.hpp"   // grid_gradient_kernel

namespace mpdx {

constexpr int EDT_TILE_INTS = 12288;   // LDS tile of a line pass (48 KB: three workgroups per CU)

struct EdtArgs {
    const uint8_t* occ;   // [nz][ny][nx]
    int32_t* ws;          // [2][nodes]
    float* sdf;           // [nodes]
    int n[3];
    int nodes;            // n[0] * n[1] * n[2] <= 2^29
    int32_t* d2;          // [nodes] or null.  (Behind the counts, not next to sdf: the order keeps edt_sdf_kernel's argument loads - profiles/grid_producers_refactor.md)
    int none;             // (n[0] + n[1] + n[2])^2
    float cell, inflate;
};

// distance from bit x to the nearest set bit of w[0 .. nw) (bits beyond the row are clear), or -1
__device__ __forceinline__ int edt_row_nearest(const unsigned long long* w, int nw, int x) {
    const int wi = x >> 6, b = x & 63;
    int best = -1;
    unsigned long long m = w[wi] & (~0ull >> (63 - b));          // bits <= b
    int k = wi;
    while (m == 0 && k > 0) m = w[--k];
    if (m) best = x - (k * 64 + 63 - __clzll(m));
    m = w[wi] & ((~0ull << b) << 1);                               // bits > b
    k = wi;
    while (m == 0 && k + 1 < nw) m = w[++k];
    if (m) {
        const int r = k * 64 + (__ffsll(m) - 1) - x;
        best = best < 0 ? r : min(best, r);
    }
    return best;
}

// pass x: 4 waves per workgroup, one row (iy, iz) per wave.  grid = ceil(rows / 4)
__global__ __launch_bounds__(256) void edt_pass_x_kernel(const EdtArgs a) {
    __shared__ unsigned long long words[4][2][64];                 // [wave][occupied | free][word]: 4096 bits per row at the cap
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rows = a.n[1] * a.n[2];
    const int row = blockIdx.x * 4 + wave;
    const bool valid = row < rows;                                 // (uniform over the wave)
    const int nx = a.n[0], nw = (nx + 63) >> 6;
    const size_t base = (size_t)row * nx;
    if (valid) {
        for (int c = 0; c < nw; ++c) {
            const int x = c * 64 + lane;
            const bool in = x < nx;
            const bool o = in && a.occ[base + x] != 0;
            const unsigned long long bo = __ballot(o), bf = __ballot(in && !o);
            if (lane == 0) { words[wave][0][c] = bo; words[wave][1][c] = bf; }
        }
    }
    __syncthreads();
    if (!valid) return;
    for (int c = 0; c < nw; ++c) {
        const int x = c * 64 + lane;
        if (x >= nx) break;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int d = edt_row_nearest(words[wave][p], nw, x);
            a.ws[(size_t)p * a.nodes + base + x] = d < 0 ? a.none : d * d;
        }
    }
}

// pass y / z over plane blockIdx.z: line l of the tile sits at ws[base + l * line_stride + tx].  X = 1 << xs columns per tile.
// grid = (ceil(nx / X), outer, 2); dynamic LDS = L * X ints
struct EdtLineArgs {
    int32_t* ws;
    int nodes, nx, L, xs;
    int line_stride, outer_stride;
    int none;
};

__global__ __launch_bounds__(256) void edt_pass_line_kernel(const EdtLineArgs a) {
    extern __shared__ __attribute__((aligned(16))) int32_t edt_tile[];
    const int X = 1 << a.xs, x0 = blockIdx.x << a.xs;
    int32_t* plane = a.ws + (size_t)blockIdx.z * a.nodes + (size_t)blockIdx.y * a.outer_stride + x0;
    const int total = a.L << a.xs;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int l = i >> a.xs, tx = i & (X - 1);
        edt_tile[i] = x0 + tx < a.nx ? plane[(size_t)l * a.line_stride + tx] : a.none;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256) {
        const int l = i >> a.xs, tx = i & (X - 1);
        if (x0 + tx >= a.nx) continue;
        int best = edt_tile[i];
        for (int d = 1; d * d < best; d += 4) {                    // candidates further out cannot win: g >= 0
            if (l - d < 0 && l + d >= a.L) break;
            // four distances per trip, their eight LDS reads independent of `best`: a candidate beyond the stopping distance is still a candidate
            // (it can only lose), one beyond the line reads the node itself and counts as `none`
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = d + u, ee = e * e;
                const bool lo = l - e >= 0, hi = l + e < a.L;
                const int vlo = edt_tile[lo ? i - (e << a.xs) : i], vhi = edt_tile[hi ? i + (e << a.xs) : i];
                best = min(best, min(lo ? vlo : a.none, hi ? vhi : a.none) + ee);
            }
        }
        plane[(size_t)l * a.line_stride + tx] = best;
    }
}

// s of node i: cell * (sqrt(d2) - 1/2) - inflate outside, -(cell * (sqrt(d2) - 1/2)) - inflate inside; every step one rounded fp32 operation
__device__ __forceinline__ float edt_signed(const EdtArgs& a, int d2, bool occupied) {
    const float t = __fmul_rn(a.cell, __fsub_rn(sqrtf((float)d2), 0.5f));   // sqrtf: correctly rounded (the __fsqrt_rn intrinsic is the native approximation)
    return __fsub_rn(occupied ? -t : t, a.inflate);
}

__global__ __launch_bounds__(256) void edt_sdf_kernel(const EdtArgs a) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= a.nodes) return;
    const bool o = a.occ[node] != 0;
    const int d2 = a.ws[(size_t)(o ? 1 : 0) * a.nodes + node];
    if (a.d2) a.d2[node] = d2;
    a.sdf[node] = edt_signed(a, d2, o);
}

// ---------------------------------------------------------------------------------------------------------------- voxelise
struct VoxelArgs {
    const float* points;   // [P][3]
    uint8_t* occ;
    int n_points, dim;
    int n[3];
    float origin[3], inv_cell;
};

__global__ __launch_bounds__(256) void occupancy_from_points_kernel(const VoxelArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.n_points) return;
    int idx[3] = {0, 0, 0};
    bool keep = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j >= a.dim) continue;                                                                       // (z is ignored in 2-D)
        const float u = __fmul_rn(__fsub_rn(a.points[3 * (size_t)p + j], a.origin[j]), a.inv_cell);   // grid_coord's two rounded operations
        const float r = rintf(u);                                                                       // half to even
        keep = keep && r >= 0.f && r <= (float)(a.n[j] - 1);                                            // (false for NaN and +-inf)
        idx[j] = (int)r;
    }
    if (!keep) return;
    a.occ[((size_t)idx[2] * a.n[1] + idx[1]) * a.n[0] + idx[0]] = 1;   // racing equal byte stores
}

}  // namespace mpdx
