// costs.hpp - the VALUES of the guide's cost terms and the clearance per trajectory (mpdx_traj_costs): what the guide kernels differentiate, evaluated.
//
// Replaces the forward half of guides.py:190 in the reference,
//     cost(x, x_interpolated=..., return_invidual_costs_and_weights=True) -> ([B] per cost term, [weight per term]),
// for a composite of the reference's terms (CostCollision per field, CostGPTrajectory) and this package's tool-axis term; the cost arithmetic lives
// in un-vendored submodules there and is restated from the published formulas (oracle/costs.py header) - PARITY UNPINNED.  The clearance (how far
// a trajectory stays from each field) replaces nothing: the reference reports collision counts only.
//
// Mapping (the pattern of traj_metrics_kernel, guide.hpp, and traj_metrics_chain_kernel, chain.hpp).  One 64-lane workgroup per trajectory; x
// (unnormalised [H][D]), the primitive table or the scene image with the tracks behind it and - chain - the chain table are staged in LDS; lane i
// strides over the evaluated points and over the H - 1 segments of the GP prior; the link-sphere centres of a lane's point live in LDS (Panda, chain:
// odd stride per lane), so the sphere and pair loops are real loops; per-slot sums and minima live in registers and meet in the fixed
// __shfl_xor butterfly.  No atomics: two launches on the same input give the same bits.
//
// Arithmetic, all fp32, from the metrics kernels' device functions (objects_sdf, grid_sdf, panda_fk, chain_fk<QD, false>, interp_pair(true, ...),
// track_offset, scene_field): a clearance below zero and a collision flag of mpdx_traj_metrics_mask come from the same signed distance.  Stated step
// by step in include/mpdx.h (mpdx_traj_costs).
//
// Variants.  The robot (point mass 2-D / 3-D, Panda, chain with 1 ... 8 joints) is a template parameter, because the state layout and the FK are
// compile-time; a grid field, several scenes, a track and the tool term are WAVE-UNIFORM RUN-TIME branches on the kernel arguments: 11 instantiations
// where the metrics kernels' scheme would make 40.  Those kernels keep such switches compile-time to hold the register counts of instantiations on the
// plan path; this kernel runs once per plan and has no earlier instantiation to protect (profiles/cost_eval_resource_usage.md).
#pragma once
#include "chain.hpp"

namespace mpdx {

struct CostArgs {
    dev_guide_params gp;     // n_prim_floats = what a workgroup stages (dev_params_staged)
    const float* x;          // [B][H][D] unnormalised
    float* cost;             // [B][MPDX_COST_SLOTS]
    float* clearance;        // [B][MPDX_MAX_FIELDS] or null
    float* point;            // [B][N][MPDX_MAX_FIELDS + 1] or null
    int B, H, N;             // N: evaluated points per trajectory (2 ... 8192)
    dev_grids grid;          // read where a field is a grid
    dev_scenes scene;        // n_scenes > 1: the workgroup stages the block of its scene
    dev_motion motion;       // len[f] != 0: field f moves
    dev_tool tool;           // frame != 0: the tool-axis term (chain)
    const float* table;      // chain: the chain table, ntab floats of it staged
    int ntab;
};

constexpr float kNoClearance = 3.0e38f;   // the clearance of a slot without factors (objects_sdf's "no primitive")

// One link sphere (centre p, radius r, hinge margin m = r + cutoff_margin) against field f of kind OBJECTS, GRID or WORKSPACE: the factors
// CostCollision.factors lists for it are added to `sum`, their distances less r are folded into `clr`.  o: the offset of a moving OBJECTS field at
// this point (zeros: the field is static, p - 0 = p in every bit).
template <int DIM, bool GRID>
__device__ __forceinline__ void sphere_field_cost(const CostArgs& a, int f, int kind, const dev_field& fld, const float* __restrict__ sprim, const float (&p)[DIM],
                                                  const float (&o)[DIM], float r, float m, float& sum, float& clr) {
    if (kind == MPDX_FIELD_WORKSPACE) {
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            const float lo = p[j] - fld.ws_min[j], hi = fld.ws_max[j] - p[j];
            sum += fmaxf(m - lo, 0.f);
            sum += fmaxf(m - hi, 0.f);
            clr = fminf(clr, fminf(lo, hi) - r);
        }
        return;
    }
    float sd;
    if (GRID && kind == MPDX_FIELD_GRID) sd = grid_sdf<DIM>(a.grid.grids, a.grid.g[f], p);
    else if (kind == MPDX_FIELD_OBJECTS) {
        float pm[DIM];
#pragma unroll
        for (int j = 0; j < DIM; ++j) pm[j] = p[j] - o[j];
        sd = objects_sdf<DIM>(sprim, fld, pm);
    } else return;   // (a kind this robot has no factors for)
    sum += fmaxf(m - sd, 0.f);
    clr = fminf(clr, sd - r);
}

template <int QD, int DIM, int ROBOT>
__global__ __launch_bounds__(64) void traj_costs_kernel(const CostArgs a) {
    constexpr int D = 2 * QD, MAXF = MPDX_MAX_FIELDS;
    constexpr bool SPHERES = ROBOT != MPDX_ROBOT_POINTMASS, CHAIN = ROBOT == MPDX_ROBOT_CHAIN;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const dev_guide_params& gp = a.gp;
    const int lane = threadIdx.x, b = blockIdx.x, H = a.H, N = a.N;
    const MetricsLds L = metrics_lds_layout(SPHERES, H, D, gp.n_prim_floats, CHAIN ? a.ntab : 0);
    float* sx = sm + L.sx;
    float* stab = sm + L.stab;
    float* sprim = sm + L.sprim;
    float* P = sm + L.sP + lane * kChainPS;   // (Panda, chain) this lane's sphere centres
    const bool multi = a.scene.n_scenes > 1;   // (uniform: a kernel argument)
    SceneCounts sc_n = {};
    if (multi) sc_n = stage_prims<true>(gp, a.scene, b, sprim, lane, 64);
    else stage_prims(gp, sprim, lane, 64);
    ChainCounts cn = {kPandaNS, kPandaNP};
    if constexpr (CHAIN) {
        for (int i = lane; i < a.ntab; i += 64) stab[i] = a.table[i];
        cn = chain_counts<QD>(a.table, a.ntab);
    }
    for (int i = lane; i < H * D; i += 64) sx[i] = a.x[(size_t)b * H * D + i];
    __syncthreads();
    (void)stab; (void)P; (void)cn;

    // ---- slot MAXF: the GP prior over the supports, sum_h 12/dt^3 |eq|^2 - 12/dt^2 eq.ev + 4/dt |ev|^2
    float gpc = 0.f;
    if (gp.use_gp) {
        const float dt = gp.dt, k3 = 12.0f / (dt * dt * dt), k2 = 12.0f / (dt * dt), k1 = 4.0f / dt;
        for (int h = lane; h < H - 1; h += 64) {
            float qq = 0.f, qv = 0.f, vv = 0.f;
#pragma unroll
            for (int j = 0; j < QD; ++j) {
                const float v0 = sx[h * D + QD + j];
                const float eq = sx[(h + 1) * D + j] - sx[h * D + j] - dt * v0, ev = sx[(h + 1) * D + QD + j] - v0;
                qq += eq * eq; qv += eq * ev; vv += ev * ev;
            }
            gpc += k3 * qq - k2 * qv + k1 * vv;
        }
    }

    // ---- slots 0 ... MAXF - 1: the collision fields; slot MAXF + 1: the tool axis - over the evaluated points
    float acc[MAXF], clr[MAXF], toolc = 0.f;
#pragma unroll
    for (int k = 0; k < MAXF; ++k) { acc[k] = 0.f; clr[k] = kNoClearance; }
    const float scale = interp_scale(H, N);
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    constexpr int SPH = kChainHdr + QD * kChainJF;
    for (int i = lane; i < N; i += 64) {
        const InterpPair ip = interp_pair(true, scale, i, H);
        float tool_i = 0.f;
        float p[DIM];   // (point mass) the point itself
        if constexpr (CHAIN) {
            float w[3] = {0.f, 0.f, 0.f};
            const bool tool_on = a.tool.frame != 0;
            chain_fk<QD, false>(stab, cn.ns, sx + ip.i0 * D, sx + ip.i1 * D, ip.l0, ip.l1, nullptr, P, tool_on ? &a.tool : nullptr, w);
            if (tool_on) tool_i = fmaxf(a.tool.cos_min - (a.tool.world[0] * w[0] + a.tool.world[1] * w[1] + a.tool.world[2] * w[2]), 0.f);
        } else {
            float q[QD];
#pragma unroll
            for (int j = 0; j < QD; ++j) q[j] = ip.l0 * sx[ip.i0 * D + j] + ip.l1 * sx[ip.i1 * D + j];
            if constexpr (SPHERES) {
                float O[7][3], Z[7][3];
                panda_fk(q, O, Z);
#pragma unroll
                for (int s = 0; s < kPandaNS; ++s)
#pragma unroll
                    for (int r = 0; r < 3; ++r) P[s * 3 + r] = O[kPandaSF[s] - 1][r] + kPandaSO[s] * Z[kPandaSF[s] - 1][r];
            } else {
#pragma unroll
                for (int j = 0; j < DIM; ++j) p[j] = q[j];
            }
        }
        toolc += tool_i;
        float* prow = a.point ? a.point + ((size_t)b * N + i) * (MAXF + 1) : nullptr;
#pragma unroll 1
        for (int f = 0; f < MAXF; ++f) {   // (a real loop: unrolled, the four fields' descriptors stay live in scalar registers at once and spill)
            float s_f = 0.f, c_f = kNoClearance;
            if (f < gp.n_fields) {   // (uniform)
                const int kind = gp.fields[f].kind;
                dev_field fld;
                if (multi) fld = scene_field(gp, sc_n, f); else fld = gp.fields[f];
                float o[DIM];
#pragma unroll
                for (int j = 0; j < DIM; ++j) o[j] = 0.f;
                if constexpr (!CHAIN)
                    if (kind == MPDX_FIELD_OBJECTS && a.motion.len[f] != 0) track_offset<DIM, false>(sprim, a.motion.off[f], ip, o);
                if constexpr (!SPHERES) {
                    sphere_field_cost<DIM, true>(a, f, kind, fld, sprim, p, o, gp.link_margin, gp.link_margin + gp.cutoff_margin, s_f, c_f);
                } else if (kind == MPDX_FIELD_SELF) {
                    for (int pr = 0; pr < cn.np; ++pr) {
                        int sa, sb;
                        float ra, rb;
                        if constexpr (CHAIN) {
                            const int pr0 = SPH + cn.ns * kChainSF;
                            sa = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr], 0), cn.ns - 1));
                            sb = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr + 1], 0), cn.ns - 1));
                            ra = stab[SPH + sa * kChainSF + 4]; rb = stab[SPH + sb * kChainSF + 4];
                        } else {
                            sa = kPandaPA[pr]; sb = kPandaPB[pr];
                            ra = kPandaSR[sa]; rb = kPandaSR[sb];
                        }
                        const float dx = P[sa * 3] - P[sb * 3], dy = P[sa * 3 + 1] - P[sb * 3 + 1], dz = P[sa * 3 + 2] - P[sb * 3 + 2];
                        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
                        s_f += fmaxf(ra + rb - dist, 0.f);
                        c_f = fminf(c_f, dist - (ra + rb));
                    }
                } else {
                    for (int s = 0; s < cn.ns; ++s) {
                        float rad;
                        if constexpr (CHAIN) rad = stab[SPH + s * kChainSF + 4]; else rad = kPandaSR[s];
                        const float p3[DIM] = {P[s * 3], P[s * 3 + 1], P[s * 3 + 2]};
                        sphere_field_cost<DIM, !CHAIN>(a, f, kind, fld, sprim, p3, o, rad, rad + gp.cutoff_margin, s_f, c_f);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < MAXF; ++k) {   // (the accumulators are registers: static indices)
                acc[k] += k == f ? s_f : 0.f;
                clr[k] = k == f ? fminf(clr[k], c_f) : clr[k];
            }
            if (prow) prow[f] = s_f;
        }
        if (prow) prow[MAXF] = tool_i;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        gpc += __shfl_xor(gpc, s, 64);
        toolc += __shfl_xor(toolc, s, 64);
#pragma unroll
        for (int k = 0; k < MAXF; ++k) {
            acc[k] += __shfl_xor(acc[k], s, 64);
            clr[k] = fminf(clr[k], __shfl_xor(clr[k], s, 64));
        }
    }
    if (lane == 0) {
        float* out = a.cost + (size_t)b * MPDX_COST_SLOTS;
#pragma unroll
        for (int k = 0; k < MAXF; ++k) out[k] = acc[k];
        const float half = gp.gp_half_factor ? 0.5f : 1.0f;
        out[MAXF] = gp.use_gp ? half * gpc / (gp.sigma_gp * gp.sigma_gp) : 0.f;
        out[MAXF + 1] = toolc;
        if (a.clearance) {
#pragma unroll
            for (int k = 0; k < MAXF; ++k) a.clearance[(size_t)b * MAXF + k] = clr[k];
        }
    }
}

// ---- k_costs.hip: every traj_costs_kernel instantiation
int launch_traj_costs(const CostArgs& a, const ChainInfo& ci, hipStream_t st);

}  // namespace mpdx
