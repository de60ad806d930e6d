// tsdf.hpp - depth-camera fusion on the device: projective TSDF integration (KinectFusion-style truncated signed distance) of up to
// MPDX_TSDF_MAX_CAMS depth frames into per-node tsdf / weight planes, and the occupancy bytes mpdx_sdf_grid_from_occupancy (edt.hpp) turns into the
// sdf and gradient planes (mpdx_tsdf_integrate in k_grid.hip; the arithmetic is stated in include/mpdx.h and restated in numpy in tests/tsdf_ref.py,
// which the kernel matches bit for bit).  Replaces nothing in the reference: its environments are primitives.
//
// One thread per node, 256 per workgroup, x fastest: the tsdf / weight loads and stores and the occupancy byte stores are coalesced.  The depth reads
// are a gather (neighbouring nodes project to neighbouring pixels, so they mostly hit the same lines).  Memory-bound: 9 bytes of planes per node
// and call, the weight and tsdf stores only where some camera measured.
// The camera records and the robot spheres are uniform over the launch, so they travel as kernel arguments (about 2.2 KB at the caps): the loops over
// cameras and spheres run on scalar loads from the argument segment - no LDS staging, no barrier, no copy.  Every step is one rounded fp32 operation
// (the build's -ffp-contract=on would fuse within an expression); rintf is half to even, as the voxeliser's.
// No atomics; nothing is allocated; no workspace; no synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpdx.h"

namespace mpdx {

struct TsdfCam {               // mpdx_depth_camera as the kernel reads it
    const float* depth;
    int width, height;
    float fx, fy, cx, cy;
    float A[12];               // cam_from_world
    float B[12];               // world_from_cam
    float min_depth, max_depth;
};

struct TsdfArgs {
    TsdfCam cams[MPDX_TSDF_MAX_CAMS];
    float spheres[MPDX_TSDF_MAX_SPHERES][4];   // centre, padded radius
    float* tsdf;
    float* weight;
    uint8_t* occ;
    int n[3];
    int nodes;
    int n_cams, n_spheres;
    float origin[3], cell;
    float trunc, max_weight;
};

// row j of a 3x4 [R | t] applied to p: ((M[j][0] p0 + M[j][1] p1) + M[j][2] p2) + M[j][3], every product and sum rounded
__device__ __forceinline__ float tsdf_row(const float* M, int j, float p0, float p1, float p2) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4 * j], p0), __fmul_rn(M[4 * j + 1], p1)), __fmul_rn(M[4 * j + 2], p2)), M[4 * j + 3]);
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfArgs a) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= a.nodes) return;
    const int ix = node % a.n[0], r = node / a.n[0];
    const int iy = r % a.n[1], iz = r / a.n[1];
    const float p0 = __fadd_rn(a.origin[0], __fmul_rn((float)ix, a.cell));
    const float p1 = __fadd_rn(a.origin[1], __fmul_rn((float)iy, a.cell));
    const float p2 = __fadd_rn(a.origin[2], __fmul_rn((float)iz, a.cell));
    float T = a.tsdf[node], W = a.weight[node];
    bool changed = false;
    for (int c = 0; c < a.n_cams; ++c) {
        const TsdfCam& cam = a.cams[c];
        const float x2 = tsdf_row(cam.A, 2, p0, p1, p2);
        if (!(x2 > 0.f)) continue;
        const float x0 = tsdf_row(cam.A, 0, p0, p1, p2), x1 = tsdf_row(cam.A, 1, p0, p1, p2);
        const float u = __fadd_rn(__fmul_rn(cam.fx, __fdiv_rn(x0, x2)), cam.cx);
        const float v = __fadd_rn(__fmul_rn(cam.fy, __fdiv_rn(x1, x2)), cam.cy);
        const float ru = rintf(u), rv = rintf(v);
        if (!(ru >= 0.f && ru <= (float)(cam.width - 1) && rv >= 0.f && rv <= (float)(cam.height - 1))) continue;   // (false for NaN and +-inf)
        const int iu = (int)ru, iv = (int)rv;
        const float d = cam.depth[(size_t)iv * cam.width + iu];
        if (!(d >= cam.min_depth && d <= cam.max_depth)) continue;
        if (a.n_spheres > 0) {
            const float q0 = __fmul_rn(__fdiv_rn(__fsub_rn(ru, cam.cx), cam.fx), d);
            const float q1 = __fmul_rn(__fdiv_rn(__fsub_rn(rv, cam.cy), cam.fy), d);
            const float P0 = tsdf_row(cam.B, 0, q0, q1, d), P1 = tsdf_row(cam.B, 1, q0, q1, d), P2 = tsdf_row(cam.B, 2, q0, q1, d);
            bool masked = false;
            for (int k = 0; k < a.n_spheres; ++k) {
                const float dx = __fsub_rn(P0, a.spheres[k][0]), dy = __fsub_rn(P1, a.spheres[k][1]), dz = __fsub_rn(P2, a.spheres[k][2]);
                const float e = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                masked = masked || e < __fmul_rn(a.spheres[k][3], a.spheres[k][3]);
            }
            if (masked) continue;
        }
        const float s = __fsub_rn(d, x2);
        if (s < -a.trunc) continue;                                               // occluded
        const float o = __fdiv_rn(fminf(s, a.trunc), a.trunc);
        const float w1 = __fadd_rn(W, 1.f);
        T = __fdiv_rn(__fadd_rn(__fmul_rn(T, W), o), w1);
        W = fminf(w1, a.max_weight);
        changed = true;
    }
    if (changed) { a.tsdf[node] = T; a.weight[node] = W; }
    a.occ[node] = (W > 0.f && T < 0.f) ? 1 : 0;
}

}  // namespace mpdx
