// grid_field.hpp - MPDX_FIELD_GRID: a precomputed signed-distance grid as a collision field of the guide and metrics kernels, and the kernel
// that bakes one from the sphere / box tables (mpdx_sdf_grid_bake), and the gradient-by-differences kernel of the producers that have no analytic
// gradient (occupancy and mesh grids).  The producers' entry points are in k_grid.hip.
//
// Replaces torch_robotics' GridMapSDF (the fixed objects' SDF sampled once per environment and looked up per link point) - un-vendored in the
// reference: the lookup is restated in include/mpdx.h (mpdx_field) with both plausible forms as an explicit
// switch, PARITY UNPINNED.
//
// Unlike the primitive fields (an FMA chain over a table staged in LDS, cost proportional to the number of primitives) a lookup is a gather
// from global memory - L2 / Infinity Cache for the sizes in question (0.27 MB: 2-D workspace at 1 cm; 7.8 MB: Panda workspace at 2 cm) - whose
// cost does not depend on the geometry:
//   - the 4 (2-D) / 8 (3-D) corner loads of a point are independent: all are issued before the first is used (one wait); the two x-neighbours
//     are adjacent floats, so a corner pair is ONE 8-byte load (dword alignment suffices for global loads on gfx950);
//   - grid_force_n issues the loads of all NPT points (the 1-4 link spheres of a Panda sphere group) before the first use, as objects_force_n
//     batches its LDS reads;
//   - index arithmetic in integers after one floor per axis; weights in fp32 from the clamped cell coordinate;
//   - the hinge is inactive for most points: the lookup is unconditional and the result selected (no per-lane branch around the loads).
// Kernel arguments.  The kernels do not take the ABI structs by value: appending the grid members to mpdx_field (48 -> 88 bytes) spreads the
// fields table of EVERY launch over more cache lines of the kernel-argument segment (measured on the primitive point-mass guide, one latency-bound
// workgroup per CU: 7.50 -> 7.73 us per launch).  dev_guide_params / dev_field are the blocks as they were before grids existed - the primitive-only
// instantiations get byte for byte the arguments they had - and the grid descriptors travel apart (dev_grids, with 1 / cell taken once on the host in
// fp32: the kernels never divide), read only by the HAS_GRID instantiations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mpdx.h"

namespace mpdx {

struct dev_field {      // = the primitive members of mpdx_field
    int32_t kind;
    float weight;
    int32_t sphere_off, n_spheres, box_off, n_boxes;
    float ws_min[3], ws_max[3];
};
struct dev_guide_params {   // = mpdx_guide_params without the grid members (same order)
    int32_t robot, q_dim, ws_dim, interpolate, n_interp, clip_grad;
    float max_grad_norm;
    float mins[16], maxs[16];
    float cutoff_margin, link_margin;
    int32_t n_fields;
    dev_field fields[MPDX_MAX_FIELDS];
    int32_t use_gp;
    float gp_weight, dt, sigma_gp;
    const float* prims;
    int32_t n_prim_floats;
    int32_t clip_rule;
    float max_grad_value;
    int32_t gp_half_factor, identity_normalizer;
};
struct dev_grid {       // the grid members of mpdx_field f, entry f of dev_grids::g
    int32_t sdf_off, grad_off;
    int32_t n[3];
    float origin[3];
    float inv_cell;     // 1.0f / cell
    int32_t mode;
};
struct dev_grids {
    const float* grids;
    dev_grid g[MPDX_MAX_FIELDS];
};

typedef float grid_f32x2 __attribute__((ext_vector_type(2), aligned(4)));   // an x-neighbour pair of the sdf plane: dword aligned
typedef float grid_f32x4 __attribute__((ext_vector_type(4)));                // a node of the gradient plane: 16-byte aligned

// cell coordinate of p along axis j: c = clamp((p - origin) * inv, 0, n - 1); `clamped` <- the point lay outside the grid box on this axis
// (a NaN coordinate clamps to node 0: fmaxf returns its non-NaN operand, so every index below stays inside the plane)
__device__ __forceinline__ float grid_coord(const dev_grid& f, int j, float pj, bool& clamped) {
    const float u = __fmul_rn(__fsub_rn(pj, f.origin[j]), f.inv_cell);
    const float c = fminf(fmaxf(u, 0.f), (float)(f.n[j] - 1));
    clamped = !(c == u);
    return c;
}

// LINEAR mode: the cell of p.  base = float index of its (0,0,0) corner in the sdf plane; w = weights; live[j] = the axis carries gradient
template <int DIM>
struct GridCell {
    int base;
    float w[DIM];
    bool live[DIM];
};

template <int DIM>
__device__ __forceinline__ GridCell<DIM> grid_cell(const dev_grid& f, const float (&p)[DIM]) {
    GridCell<DIM> c;
    int idx[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
        bool cl;
        const float cj = grid_coord(f, j, p[j], cl);
        int i = (int)floorf(cj);
        i = min(max(i, 0), f.n[j] - 2);
        c.w[j] = cj - (float)i;
        c.live[j] = !cl;
        idx[j] = i;
    }
    int b = idx[DIM - 1];
#pragma unroll
    for (int j = DIM - 2; j >= 0; --j) b = b * f.n[j] + idx[j];
    c.base = f.sdf_off + b;
    return c;
}

// the 2^(DIM-1) x-neighbour pairs of the cell: v[k] = (node at x0, node at x0 + 1) of row k = y + 2 z
template <int DIM>
__device__ __forceinline__ void grid_load_cell(const float* __restrict__ grids, const dev_grid& f, const GridCell<DIM>& c, grid_f32x2 (&v)[1 << (DIM - 1)]) {
    const int sy = f.n[0], sz = DIM == 3 ? f.n[0] * f.n[1] : 0;
#pragma unroll
    for (int k = 0; k < (1 << (DIM - 1)); ++k) v[k] = *(const grid_f32x2*)(grids + c.base + (k & 1) * sy + (k >> 1) * sz);
}

// the interpolant a + w (b - a) along x, then y, then z, and its derivative w.r.t. p (node differences times 1 / cell; 0 along a clamped axis)
template <int DIM, bool GRAD>
__device__ __forceinline__ float grid_interp(const dev_grid& f, const GridCell<DIM>& c, const grid_f32x2 (&v)[1 << (DIM - 1)], float (&g)[DIM]) {
    constexpr int NR = 1 << (DIM - 1);
    float s[NR], dx[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        dx[k] = v[k].y - v[k].x;
        s[k] = v[k].x + c.w[0] * dx[k];
    }
    float val, gx = 0.f, gy = 0.f, gz = 0.f;
    if constexpr (DIM == 2) {
        const float dy = s[1] - s[0];
        val = s[0] + c.w[1] * dy;
        if constexpr (GRAD) {
            gx = dx[0] + c.w[1] * (dx[1] - dx[0]);
            gy = dy;
        }
    } else {
        const float dy0 = s[1] - s[0], dy1 = s[3] - s[2];
        const float t0 = s[0] + c.w[1] * dy0, t1 = s[2] + c.w[1] * dy1;
        const float dz = t1 - t0;
        val = t0 + c.w[2] * dz;
        if constexpr (GRAD) {
            const float x0 = dx[0] + c.w[1] * (dx[1] - dx[0]), x1 = dx[2] + c.w[1] * (dx[3] - dx[2]);
            gx = x0 + c.w[2] * (x1 - x0);
            gy = dy0 + c.w[2] * (dy1 - dy0);
            gz = dz;
        }
    }
    (void)gx; (void)gy; (void)gz;
    if constexpr (GRAD) {
        g[0] = c.live[0] ? gx * f.inv_cell : 0.f;
        g[1] = c.live[1] ? gy * f.inv_cell : 0.f;
        if constexpr (DIM == 3) g[2] = c.live[2] ? gz * f.inv_cell : 0.f;
    }
    return val;
}

// NEAREST mode: node index of p (i_j = rint of the clamped cell coordinate: half to even, as torch.round)
template <int DIM>
__device__ __forceinline__ int grid_node(const dev_grid& f, const float (&p)[DIM]) {
    int idx[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
        bool cl;
        const int i = (int)rintf(grid_coord(f, j, p[j], cl));
        idx[j] = min(max(i, 0), f.n[j] - 1);
    }
    int b = idx[DIM - 1];
#pragma unroll
    for (int j = DIM - 2; j >= 0; --j) b = b * f.n[j] + idx[j];
    return b;
}

// signed distance of p in the grid field f (collision checking: the contract of objects_sdf)
template <int DIM>
__device__ __forceinline__ float grid_sdf(const float* __restrict__ grids, const dev_grid& f, const float (&p)[DIM]) {
    if (f.mode == MPDX_GRID_NEAREST) return grids[f.sdf_off + grid_node<DIM>(f, p)];
    const GridCell<DIM> c = grid_cell<DIM>(f, p);
    grid_f32x2 v[1 << (DIM - 1)];
    grid_load_cell<DIM>(grids, f, c, v);
    float g[DIM];
    return grid_interp<DIM, false>(f, c, v, g);
}

// the contract of objects_force_n for a grid field: per point the hinge relu(margin - sdf) and force = its gradient w.r.t. p (= -grad sdf where the
// hinge is active, else 0).  The loads of ALL points are issued before the first use.  `hinge` (or null) <- the hinge values.
template <int DIM, int NPT>
__device__ __forceinline__ void grid_force_n(const float* __restrict__ grids, const dev_grid& f, const float (&p)[NPT][DIM], const float (&margin)[NPT],
                                             float (&force)[NPT][DIM], float* hinge = nullptr) {
    float sd[NPT], g[NPT][DIM];
    if (f.mode == MPDX_GRID_NEAREST) {   // (uniform over the launch: a scalar branch)
        int node[NPT];
        grid_f32x4 gv[NPT];
#pragma unroll
        for (int n = 0; n < NPT; ++n) node[n] = grid_node<DIM>(f, p[n]);
#pragma unroll
        for (int n = 0; n < NPT; ++n) {
            sd[n] = grids[f.sdf_off + node[n]];
            gv[n] = *(const grid_f32x4*)(grids + f.grad_off + 4 * node[n]);
        }
#pragma unroll
        for (int n = 0; n < NPT; ++n) {
            g[n][0] = gv[n].x; g[n][1] = gv[n].y;
            if constexpr (DIM == 3) g[n][2] = gv[n].z;
        }
    } else {
        GridCell<DIM> c[NPT];
        grid_f32x2 v[NPT][1 << (DIM - 1)];
#pragma unroll
        for (int n = 0; n < NPT; ++n) c[n] = grid_cell<DIM>(f, p[n]);
#pragma unroll
        for (int n = 0; n < NPT; ++n) grid_load_cell<DIM>(grids, f, c[n], v[n]);
#pragma unroll
        for (int n = 0; n < NPT; ++n) sd[n] = grid_interp<DIM, true>(f, c[n], v[n], g[n]);
    }
#pragma unroll
    for (int n = 0; n < NPT; ++n) {
        const float h = margin[n] - sd[n];
        const bool on = h > 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j) force[n][j] = on ? -g[n][j] : 0.f;
        if (hinge) hinge[n] = on ? h : 0.f;
    }
}

// the contract of objects_force: returns relu(margin - sdf); force = its gradient w.r.t. p
template <int DIM>
__device__ __forceinline__ float grid_force(const float* __restrict__ grids, const dev_grid& f, const float (&p)[DIM], float margin, float (&force)[DIM]) {
    float p1[1][DIM], fo[1][DIM], h[1];
#pragma unroll
    for (int j = 0; j < DIM; ++j) p1[0][j] = p[j];
    const float m1[1] = {margin};
    grid_force_n<DIM, 1>(grids, f, p1, m1, fo, h);
#pragma unroll
    for (int j = 0; j < DIM; ++j) force[j] = fo[0][j];
    return h[0];
}

// ---------------------------------------------------------------------------------------------------------------- bake
// One thread per node: minimum signed distance to the primitives of field f (the arithmetic of objects_sdf: IEEE sqrtf) with its arg-min, then -
// if asked - the analytic gradient of the arg-min primitive (the arithmetic objects_force evaluates after its scan, with the sign of grad sdf).
struct GridBakeArgs {
    dev_field f;             // the OBJECTS field (offsets into prims)
    const float* prims;
    int n_prim_floats;
    float* sdf;              // [nz][ny][nx]
    float* grad;             // [nz][ny][nx][4] or null
    int n[3];
    float origin[3], cell;
};

template <int DIM>
__global__ __launch_bounds__(256) void sdf_grid_bake_kernel(const GridBakeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    for (int i = threadIdx.x; i < a.n_prim_floats; i += 256) sm[i] = a.prims[i];
    __syncthreads();
    const long long total = (long long)a.n[0] * a.n[1] * a.n[2];
    const long long node = (long long)blockIdx.x * 256 + threadIdx.x;
    if (node >= total) return;
    const int ix = (int)(node % a.n[0]), iy = (int)((node / a.n[0]) % a.n[1]), iz = (int)(node / ((long long)a.n[0] * a.n[1]));
    const int id[3] = {ix, iy, iz};
    float p[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) p[j] = __fadd_rn(a.origin[j], __fmul_rn((float)id[j], a.cell));
    const dev_field& f = a.f;
    const float* sp = sm + f.sphere_off;
    const float* bp = sm + f.box_off;
    float best = 3.0e38f;
    int bi = -1;   // arg-min: sphere index, or n_spheres + box index
    for (int s = 0; s < f.n_spheres; ++s) {
        float n2 = 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j) { const float d = p[j] - sp[s * 4 + j]; n2 += d * d; }
        const float sd = sqrtf(n2) - sp[s * 4 + 3];
        const bool better = sd < best;
        best = better ? sd : best;
        bi = better ? s : bi;
    }
    for (int s = 0; s < f.n_boxes; ++s) {
        float mx = -3.0e38f, n2 = 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            const float d = fabsf(p[j] - bp[s * 6 + j]) - bp[s * 6 + 3 + j];
            mx = fmaxf(mx, d);
            const float r = fmaxf(d, 0.f);
            n2 += r * r;
        }
        const float sd = fminf(mx, 0.f) + sqrtf(n2);
        const bool better = sd < best;
        best = better ? sd : best;
        bi = better ? f.n_spheres + s : bi;
    }
    a.sdf[node] = best;
    if (!a.grad) return;
    float g[3] = {0.f, 0.f, 0.f};
    if (bi >= 0 && bi < f.n_spheres) {
        float d[DIM], n2 = 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j) { d[j] = p[j] - sp[bi * 4 + j]; n2 += d[j] * d[j]; }
        const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j) g[j] = d[j] * inv;
    } else if (bi >= 0) {
        const int bb = bi - f.n_spheres;
        float d[DIM], sg[DIM], mx = -3.0e38f, n2 = 0.f;
        int jm = 0;
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            const float cc = p[j] - bp[bb * 6 + j];
            sg[j] = cc > 0.f ? 1.f : (cc < 0.f ? -1.f : 0.f);
            d[j] = fabsf(cc) - bp[bb * 6 + 3 + j];
            jm = d[j] > mx ? j : jm;
            mx = fmaxf(mx, d[j]);
            const float r = fmaxf(d[j], 0.f);
            n2 += r * r;
        }
        const bool outside = mx > 0.f;
        const float inv = outside ? 1.0f / sqrtf(n2) : 0.f;
#pragma unroll
        for (int j = 0; j < DIM; ++j)  // outside: gradient of |relu(d)|; inside (or on the surface): gradient of max_j d_j
            g[j] = outside ? sg[j] * fmaxf(d[j], 0.f) * inv : (j == jm ? sg[j] : 0.f);
    }
    *(grid_f32x4*)(a.grad + 4 * node) = (grid_f32x4){g[0], g[1], g[2], 0.f};
}

// ---------------------------------------------------------------------------------------------------------------- gradient by differences
// The gradient plane of a FINISHED sdf plane, for the producers without an analytic one (occupancy and mesh grids; launched by k_grid.hip after their
// sdf kernels): central differences inside, one-sided at the faces; the unused axis and the fourth word are 0.
struct GridGradientArgs {
    const float* sdf;   // [nodes]
    float* grad;        // [nodes][4]
    int n[3];
    int nodes;          // n[0] * n[1] * n[2] <= 2^29
    float k1, k2;       // 1 / cell, 0.5 / cell
};

template <int DIM>
__global__ __launch_bounds__(256) void grid_gradient_kernel(const GridGradientArgs a) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= a.nodes) return;
    const int nx = a.n[0], ny = a.n[1];
    const int ix = node % nx, iy = (node / nx) % ny, iz = node / (nx * ny);
    const int id[3] = {ix, iy, iz};
    const int stride[3] = {1, nx, nx * ny};
    float g[3] = {0.f, 0.f, 0.f};
    const float s = a.sdf[node];
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
        const bool first = id[j] == 0, last = id[j] == a.n[j] - 1;   // (n[j] >= 2: never both)
        const float hi = last ? s : a.sdf[node + stride[j]];
        const float lo = first ? s : a.sdf[node - stride[j]];
        g[j] = __fmul_rn(__fsub_rn(hi, lo), (first || last) ? a.k1 : a.k2);
    }
    *(grid_f32x4*)(a.grad + 4 * (size_t)node) = (grid_f32x4){g[0], g[1], g[2], 0.f};
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline bool has_grid_field(const mpdx_guide_params& gp) {
    for (int f = 0; f < gp.n_fields && f < MPDX_MAX_FIELDS; ++f)
        if (gp.fields[f].kind == MPDX_FIELD_GRID) return true;
    return false;
}

// The descriptor checks of every launcher that takes grid fields: nullptr = fine, else what is wrong.  After them every index the lookups form lies
// inside [0, n_grid_floats).
inline const char* grid_params_problem(const mpdx_guide_params& gp) {
    for (int i = 0; i < gp.n_fields && i < MPDX_MAX_FIELDS; ++i) {
        const mpdx_field& f = gp.fields[i];
        if (f.kind != MPDX_FIELD_GRID) continue;
        if (!gp.grids || gp.n_grid_floats <= 0) return "grid field without a grid buffer (grids == NULL)";
        if (gp.ws_dim != 2 && gp.ws_dim != 3) return "grid field: ws_dim must be 2 or 3";
        long long nodes = 1;
        for (int j = 0; j < 3; ++j) {
            const bool used = j < gp.ws_dim;
            if (used ? (f.n[j] < 2 || f.n[j] > 4096) : f.n[j] != 1) return "grid field: at least 2 (at most 4096) nodes along every used axis, 1 along an unused one";
            nodes *= f.n[j];
        }
        if (!(f.cell > 0.f) || !(f.cell < 3.0e38f)) return "grid field: cell must be positive and finite";
        for (int j = 0; j < gp.ws_dim; ++j)
            if (!(f.origin[j] > -3.0e38f && f.origin[j] < 3.0e38f)) return "grid field: origin must be finite";
        if (f.mode != MPDX_GRID_LINEAR && f.mode != MPDX_GRID_NEAREST) return "grid field: mode must be MPDX_GRID_LINEAR or MPDX_GRID_NEAREST";
        if (f.grid_sdf_off < 0 || (long long)f.grid_sdf_off + nodes > (long long)gp.n_grid_floats) return "grid field: sdf plane beyond the grid buffer";
        if (f.mode == MPDX_GRID_NEAREST && f.grid_grad_off < 0) return "grid field: MPDX_GRID_NEAREST needs a gradient plane";
        if (f.grid_grad_off >= 0) {
            if ((long long)f.grid_grad_off + 4 * nodes > (long long)gp.n_grid_floats) return "grid field: gradient plane beyond the grid buffer";
            if ((f.grid_grad_off & 3) || ((uintptr_t)gp.grids & 15)) return "grid field: the gradient plane must be 16-byte aligned (grids aligned, offset a multiple of 4)";
        }
        if ((uintptr_t)gp.grids & 3) return "grid buffer must be 4-byte aligned";
    }
    return nullptr;
}

inline dev_field dev_field_of(const mpdx_field& f) {
    dev_field d;
    d.kind = f.kind; d.weight = f.weight; d.sphere_off = f.sphere_off; d.n_spheres = f.n_spheres; d.box_off = f.box_off; d.n_boxes = f.n_boxes;
    for (int j = 0; j < 3; ++j) { d.ws_min[j] = f.ws_min[j]; d.ws_max[j] = f.ws_max[j]; }
    return d;
}

// the kernels' parameter block (see the header comment): every member but the grid ones
inline dev_guide_params dev_params_of(const mpdx_guide_params& gp) {
    dev_guide_params d;
    memset(&d, 0, sizeof(d));
    d.robot = gp.robot; d.q_dim = gp.q_dim; d.ws_dim = gp.ws_dim; d.interpolate = gp.interpolate; d.n_interp = gp.n_interp; d.clip_grad = gp.clip_grad;
    d.max_grad_norm = gp.max_grad_norm;
    for (int j = 0; j < 16; ++j) { d.mins[j] = gp.mins[j]; d.maxs[j] = gp.maxs[j]; }
    d.cutoff_margin = gp.cutoff_margin; d.link_margin = gp.link_margin; d.n_fields = gp.n_fields;
    for (int f = 0; f < MPDX_MAX_FIELDS; ++f) d.fields[f] = dev_field_of(gp.fields[f]);
    d.use_gp = gp.use_gp; d.gp_weight = gp.gp_weight; d.dt = gp.dt; d.sigma_gp = gp.sigma_gp; d.prims = gp.prims; d.n_prim_floats = gp.n_prim_floats;
    d.clip_rule = gp.clip_rule; d.max_grad_value = gp.max_grad_value; d.gp_half_factor = gp.gp_half_factor; d.identity_normalizer = gp.identity_normalizer;
    return d;
}

// the grid descriptors of a VALIDATED block (grid_params_problem), 1 / cell taken here, once, in fp32
inline dev_grids dev_grids_of(const mpdx_guide_params& gp) {
    dev_grids d;
    memset(&d, 0, sizeof(d));
    d.grids = gp.grids;
    for (int i = 0; i < gp.n_fields && i < MPDX_MAX_FIELDS; ++i) {
        const mpdx_field& f = gp.fields[i];
        if (f.kind != MPDX_FIELD_GRID) continue;
        dev_grid& g = d.g[i];
        g.sdf_off = f.grid_sdf_off; g.grad_off = f.grid_grad_off; g.mode = f.mode; g.inv_cell = 1.0f / f.cell;
        for (int j = 0; j < 3; ++j) { g.n[j] = f.n[j]; g.origin[j] = f.origin[j]; }
    }
    return d;
}

}  // namespace mpdx
