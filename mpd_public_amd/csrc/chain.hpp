// chain.hpp - the guide update and the trajectory metrics for a serial kinematic chain given at run time as a table (MPDX_ROBOT_CHAIN,
// include/mpdx.h: header | joints [R | t | type] | link spheres [frame | offset | radius] | self-collision pairs).
//
// Replaces nothing in the reference: it builds one of its own robots by name (scripts/inference/inference.py:107-123); a robot described by a
// table is this package's extension.  The arithmetic is that of the Panda kernel (guide.hpp) with the kinematics read
// from the table: forces on the link spheres from the same device functions (objects_force, workspace_force, the pair force of the self
// field), folded onto the joints (revolute g_j = z_j . sum (P_s - O_j) x F_s, prismatic g_j = z_j . sum F_s over the spheres joint j moves),
// then the Panda kernel's later phases as they are: the fixed-order gather to the supports with the clip and the weight, and guide_gp_apply.
//
// Mapping.  One 512-thread workgroup per trajectory.  The number of joints QD is a template parameter (1 ... 8: the state layout [H][2 QD]
// of guide_gp_apply is compile-time); the numbers of spheres and pairs are run-time values read from the staged table, clamped to the caps, and
// every index taken from the table (frame, pair member) is clamped before use.  Register arrays are indexed by unrolled loop counters only:
// per-sphere data live in LDS, the per-joint accumulators are predicated on the sphere's (wave-uniform) frame.  No scratch.
//   phase 1  FK once per interpolated point: O_k, z_k, P_s -> LDS (odd stride per point)
//   phase 2  wave = (point half, field): forces on every link sphere (or pair), folded to joint gradients -> LDS
//   phase 3  wave f gathers field f to the supports, clips, weights          phase 4  sum over fields, GP prior, apply (guide_gp_apply)
//
// The tool-axis term (the tool members of mpdx_guide_params, arithmetic in include/mpdx.h; dev_tool below) is a fifth cost next to the fields: the
// TOOL instantiations, chosen by the launcher when tool_frame != 0.  Phase 1 also stores w_i = Rot_f(q_i) a while frame f's rotation is in registers,
// phase 2 treats the term as slot n_fields of the (point half, slot) loop (with four fields: a second pass for two of the eight waves), phase 3
// gives it wave n_fields, phase 4 sums one slot more.  With four fields the gather takes five waves and three draw the step's noise instead of four:
// the draw is addressed by Philox counter, so its values do not depend on the partition.  TOOL is a template parameter because the measured off-path
// cost said so: as a wave-uniform branch on the kernel argument the term cost the 7-joint kernel 19 VGPRs and a launch WITHOUT the term 1.1 - 1.2 %;
// the TOOL = false instantiations have the register counts the kernel had before the term, and 0.7 - 0.9 % of that remain at 7 joints, unexplained
// (profiles/tool_axis_probe.md).  traj_tool_chain_kernel reports the term's d_i per trajectory (mpdx_traj_tool_metrics).
#pragma once
#include "guide.hpp"

namespace mpdx {

constexpr int kChainHdr = MPDX_ROBOT_CHAIN_HEADER_FLOATS, kChainJF = MPDX_ROBOT_CHAIN_JOINT_FLOATS, kChainSF = MPDX_ROBOT_CHAIN_SPHERE_FLOATS;
constexpr int kChainMaxS = MPDX_ROBOT_CHAIN_MAX_SPHERES, kChainMaxP = MPDX_ROBOT_CHAIN_MAX_PAIRS;

// the tool members of mpdx_guide_params (a validated block: frame 0 = no term, else 1 ... n_joints; unit axes)
struct dev_tool {
    int32_t frame;
    float axis[3], world[3];
    float cos_min, weight;
};
inline dev_tool dev_tool_of(const mpdx_guide_params& gp) {
    dev_tool t;
    t.frame = gp.tool_frame; t.cos_min = gp.tool_cos_min; t.weight = gp.tool_weight;
    for (int j = 0; j < 3; ++j) { t.axis[j] = gp.tool_axis[j]; t.world[j] = gp.tool_world[j]; }
    return t;
}

struct ChainGuideArgs {
    GuideArgs g;            // as the other guide kernels take it
    const float* table;     // the chain table (device)
    int n_table_floats;     // floats a workgroup stages: header + joints + spheres + pairs of the validated table
    dev_tool tool;          // the tool-axis term: read by the TOOL instantiations only
};

// sphere / pair counts of the staged table: the header's, clamped to the caps and to what the staged floats hold (scalar registers)
struct ChainCounts { int ns, np; };
template <int QD>
__device__ __forceinline__ ChainCounts chain_counts(const float* __restrict__ table, int n_floats) {
    const int32_t* h = reinterpret_cast<const int32_t*>(table);
    const int room_s = (n_floats - kChainHdr - QD * kChainJF) / kChainSF;
    ChainCounts c;
    c.ns = __builtin_amdgcn_readfirstlane(min(max(h[1], 0), min(kChainMaxS, max(room_s, 0))));
    const int room_p = (n_floats - kChainHdr - QD * kChainJF - c.ns * kChainSF) / 2;
    c.np = __builtin_amdgcn_readfirstlane(c.ns > 0 ? min(max(h[2], 0), min(kChainMaxP, max(room_p, 0))) : 0);
    return c;
}

// Forward kinematics of one configuration from the staged table: T_j = T_{j-1} [R_j | t_j] M_j(q_j).  The configuration is the interpolation
// l0 * qa + l1 * qb of two rows of the LDS-staged state, read joint by joint (the joint loop is a real loop: its index addresses LDS only).
// oz (or null): O_k at oz[3 k + r], z_k at oz[3 QD + 3 k + r]; pp: sphere centre s at pp[3 s + r].  The spheres of a frame are placed while that
// frame's transform is in registers (the frame of a sphere is wave-uniform: a scalar branch per (frame, sphere)).
// tool (or null) with tool->frame = f in 1 ... QD: w_out[r] <- (Rot_f a)[r], the tool axis in the world, stored while frame f's rotation is in registers.
template <int QD, bool WRITE_OZ>
__device__ __forceinline__ void chain_fk(const float* __restrict__ stab, int ns, const float* __restrict__ qa, const float* __restrict__ qb, float l0, float l1,
                                         float* __restrict__ oz, float* __restrict__ pp, const dev_tool* __restrict__ tool = nullptr, float* __restrict__ w_out = nullptr) {
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    const float* sph = stab + kChainHdr + QD * kChainJF;
    float R[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}, T[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k = -1; k < QD; ++k) {
        if (k >= 0) {
            const float* J = stab + kChainHdr + k * kChainJF;
            const bool prismatic = __builtin_amdgcn_readfirstlane(tabi[kChainHdr + k * kChainJF + 12]) != 0;
            const float qk = l0 * qa[k] + l1 * qb[k];
            float A[3][3], Tn[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A[r][c] = R[r][0] * J[c] + R[r][1] * J[3 + c] + R[r][2] * J[6 + c];
                Tn[r] = R[r][0] * J[9] + R[r][1] * J[10] + R[r][2] * J[11] + T[r];
            }
            float st = 0.f, ct = 1.f, dz = 0.f;
            if (prismatic) dz = qk;
            else { st = sinf(qk); ct = cosf(qk); }   // (joint limits are the caller's: the range-reduced forms, not the hardware approximations)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                R[r][0] = A[r][0] * ct + A[r][1] * st;
                R[r][1] = A[r][1] * ct - A[r][0] * st;
                R[r][2] = A[r][2];
                T[r] = Tn[r] + dz * A[r][2];
                if constexpr (WRITE_OZ) { oz[k * 3 + r] = T[r]; oz[QD * 3 + k * 3 + r] = R[r][2]; }
            }
            if (tool && tool->frame == k + 1) {   // (tool: null unless a TOOL instantiation; the frame is a kernel argument: wave-uniform)
#pragma unroll
                for (int r = 0; r < 3; ++r) w_out[r] = R[r][0] * tool->axis[0] + R[r][1] * tool->axis[1] + R[r][2] * tool->axis[2];
            }
        }
#pragma unroll 1
        for (int s = 0; s < ns; ++s) {   // the spheres of frame k + 1 (frame 0: the fixed base, before the first joint)
            const int fr = __builtin_amdgcn_readfirstlane(min(max(tabi[kChainHdr + QD * kChainJF + s * kChainSF], 0), QD));
            if (fr != k + 1) continue;
            const float ox = sph[s * kChainSF + 1], oy = sph[s * kChainSF + 2], oz_ = sph[s * kChainSF + 3];
#pragma unroll
            for (int r = 0; r < 3; ++r) pp[s * 3 + r] = T[r] + R[r][0] * ox + R[r][1] * oy + R[r][2] * oz_;
        }
    }
}

// phase 2 for one interpolated point and one field: the forces on the link spheres (or pairs), accumulated per joint k as the total force Ft[k]
// and moment about the world origin Mt[k] of the spheres joint k moves (frame > k, frames 1-based), then
//     revolute  g_k = z_k . (Mt[k] - O_k x Ft[k])        prismatic  g_k = z_k . Ft[k]
// fk: the point's FK record in LDS (O | Z | P); g_out: QD floats in LDS
template <int QD>
__device__ __forceinline__ void chain_point_field(const dev_guide_params& gp, const dev_field& fld, const float* __restrict__ sprim, const float* __restrict__ stab,
                                                  const ChainCounts& cn, const float* __restrict__ fk, float* __restrict__ g_out) {
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    constexpr int SPH = kChainHdr + QD * kChainJF;
    const float* P = fk + 6 * QD;
    float Ft[QD][3], Mt[QD][3];
#pragma unroll
    for (int k = 0; k < QD; ++k) { Ft[k][0] = Ft[k][1] = Ft[k][2] = 0.f; Mt[k][0] = Mt[k][1] = Mt[k][2] = 0.f; }
    // a force f on the sphere at p of frame fr (sign sg): every joint below the frame feels it
    auto push = [&](int fr, const float (&p)[3], const float (&f)[3], float sg) {
        const float m[3] = {p[1] * f[2] - p[2] * f[1], p[2] * f[0] - p[0] * f[2], p[0] * f[1] - p[1] * f[0]};
#pragma unroll
        for (int k = 0; k < QD; ++k) {
            if (fr > k) {   // (wave-uniform)
#pragma unroll
                for (int r = 0; r < 3; ++r) { Ft[k][r] += sg * f[r]; Mt[k][r] += sg * m[r]; }
            }
        }
    };
    if (fld.kind == MPDX_FIELD_SELF) {
        const int pr0 = SPH + cn.ns * kChainSF;
        for (int pr = 0; pr < cn.np; ++pr) {
            const int sa = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr], 0), cn.ns - 1));
            const int sb = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr + 1], 0), cn.ns - 1));
            const int fa = __builtin_amdgcn_readfirstlane(min(max(tabi[SPH + sa * kChainSF], 0), QD));
            const int fb = __builtin_amdgcn_readfirstlane(min(max(tabi[SPH + sb * kChainSF], 0), QD));
            const float ra = stab[SPH + sa * kChainSF + 4], rb = stab[SPH + sb * kChainSF + 4];
            const float pa[3] = {P[sa * 3], P[sa * 3 + 1], P[sa * 3 + 2]}, pb[3] = {P[sb * 3], P[sb * 3 + 1], P[sb * 3 + 2]};
            const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float dist = __builtin_amdgcn_sqrtf(d2);
            const float inv = (ra + rb - dist > 0.f && dist > 0.f) ? __builtin_amdgcn_rsqf(d2) : 0.f;
            const float f[3] = {dx * inv, dy * inv, dz * inv};   // d cost / d P_b = +f,  d cost / d P_a = -f
            push(fa, pa, f, -1.f);
            push(fb, pb, f, 1.f);
        }
    } else {
        for (int s = 0; s < cn.ns; ++s) {
            const int fr = __builtin_amdgcn_readfirstlane(min(max(tabi[SPH + s * kChainSF], 0), QD));
            const float margin = stab[SPH + s * kChainSF + 4] + gp.cutoff_margin;
            const float p[3] = {P[s * 3], P[s * 3 + 1], P[s * 3 + 2]};
            float f[3];
            if (fld.kind == MPDX_FIELD_OBJECTS) objects_force<3>(sprim, fld, p, margin, f);
            else if (fld.kind == MPDX_FIELD_WORKSPACE) workspace_force<3>(fld, p, margin, f);
            else { f[0] = f[1] = f[2] = 0.f; }
            push(fr, p, f, 1.f);   // (a base-frame sphere, fr = 0: felt, no joint moves it)
        }
    }
#pragma unroll
    for (int k = 0; k < QD; ++k) {
        const bool prismatic = __builtin_amdgcn_readfirstlane(tabi[kChainHdr + k * kChainJF + 12]) != 0;
        const float O[3] = {fk[k * 3], fk[k * 3 + 1], fk[k * 3 + 2]}, Z[3] = {fk[3 * QD + k * 3], fk[3 * QD + k * 3 + 1], fk[3 * QD + k * 3 + 2]};
        const float cx = O[1] * Ft[k][2] - O[2] * Ft[k][1], cy = O[2] * Ft[k][0] - O[0] * Ft[k][2], cz = O[0] * Ft[k][1] - O[1] * Ft[k][0];
        const float rev = Z[0] * (Mt[k][0] - cx) + Z[1] * (Mt[k][1] - cy) + Z[2] * (Mt[k][2] - cz);
        const float pri = Z[0] * Ft[k][0] + Z[1] * Ft[k][1] + Z[2] * Ft[k][2];
        g_out[k] = prismatic ? pri : rev;
    }
}

// phase 2 of the tool-axis term for one interpolated point: d = u . w, hinge relu(cos_min - d), and for a revolute joint k < frame (0-based: joint
// k + 1 <= f) g_k = -[hinge > 0] z_k . (w x u); 0 for a prismatic joint and above the frame.  fk: the point's FK record (Z at 3 QD), w: its tool axis.
template <int QD>
__device__ __forceinline__ void chain_point_tool(const dev_tool& tool, const float* __restrict__ stab, const float* __restrict__ fk, const float* __restrict__ w,
                                                 float* __restrict__ g_out) {
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    const float wx = w[0], wy = w[1], wz = w[2];
    const float d = tool.world[0] * wx + tool.world[1] * wy + tool.world[2] * wz;
    const bool active = tool.cos_min - d > 0.f;
    const float cx = wy * tool.world[2] - wz * tool.world[1], cy = wz * tool.world[0] - wx * tool.world[2], cz = wx * tool.world[1] - wy * tool.world[0];
#pragma unroll
    for (int k = 0; k < QD; ++k) {
        const bool prismatic = __builtin_amdgcn_readfirstlane(tabi[kChainHdr + k * kChainJF + 12]) != 0;
        const float zc = fk[3 * QD + k * 3] * cx + fk[3 * QD + k * 3 + 1] * cy + fk[3 * QD + k * 3 + 2] * cz;
        g_out[k] = (active && !prismatic && k < tool.frame) ? -zc : 0.f;
    }
}

template <int QD, bool MULTI_SCENE, bool TOOL>
__global__ __launch_bounds__(512, 2) void guide_step_chain_kernel(const ChainGuideArgs ca) {
    constexpr int D = 2 * QD, MAXF = MPDX_MAX_FIELDS, WPT = 8, FKS = chain_fk_stride(QD);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const GuideArgs& a = ca.g;
    const dev_guide_params& gp = a.gp;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    const int H = a.H;
    const int N = gp.interpolate ? gp.n_interp : H;
    const int nsw = (H + 63) >> 6;   // support waves (H <= 128)
    const int hs_ = (wv < nsw ? wv : 0) * 64 + lane;
    const bool live = hs_ < H;
    int tr_i = 0;
    G_STAMP();  // 0 entry
    const int ntab = ca.n_table_floats;
    const int n_slots = gp.n_fields + (TOOL ? 1 : 0);   // the tool-axis term: one more cost slot behind the fields
    const GuideLds L = guide_lds_layout(kGuideChain, H, D, N, gp.n_prim_floats, ntab, TOOL);
    float* sx = sm + L.sx;        // [H][D]  unnormalised state
    float* stab = sm + L.stab;    // the chain table
    float* sfk = sm + L.sfk;      // [N][FKS]  O | Z | P per interpolated point
    float* sW = sm + L.sW;        // tool term: [N][3]  the tool axis in the world per interpolated point
    float* sG = sm + L.sG;        // [MAXF (+ 1)][N][QD]  joint gradients per (slot, point)
    float* sC = sm + L.sC;        // [MAXF (+ 1)][H][QD]  clipped, weighted per-slot support-point gradients
    float* snz = sm + L.snz;      // 16-byte aligned: [H * D + 8] the step's noise, drawn in whole groups of four (H * D need not be a multiple of 4 here)
    float* snz_x = sm + L.snz_x;  // [H * D] the normalised state
    float* sprim = sm + L.sprim;
    float* shc = sm + L.shc;      // [2][D] this trajectory's hard conditions (apply mode)
    const SceneCounts sc_n = stage_prims<MULTI_SCENE>(gp, a.scene, b, sprim, threadIdx.x, 64 * WPT);
    for (int i = threadIdx.x; i < ntab; i += 64 * WPT) stab[i] = ca.table[i];
    const ChainCounts cn = chain_counts<QD>(ca.table, ntab);
    stage_hard_conds(a.hs, a.hg, !a.grad_out, b, D, shc);

    // ---- load + unnormalise (normalization.py:156-167) by the whole workgroup, dword loads (H * D need not be a multiple of 4)
    const int ctx = b / a.n_per_ctx;
    stage_state_unnormalised<D, 64 * WPT>(gp, a.x + (size_t)b * H * D, H * D, __uint_as_float(a.amax_in[ctx]) > 1.0001f, sx, snz_x, lane);
    __syncthreads();
    G_STAMP();  // 1 state unnormalised + staged, tables in LDS

    // ---- phase 1: interpolate + FK, once per point
    const float scale = interp_scale(H, N);
    for (int i = wv * 64 + lane; i < N; i += 64 * WPT) {
        const InterpPair ip = interp_pair(gp.interpolate, scale, i, H);
        float* fk = sfk + i * FKS;
        chain_fk<QD, true>(stab, cn.ns, sx + ip.i0 * D, sx + ip.i1 * D, ip.l0, ip.l1, fk, fk + 6 * QD, TOOL ? &ca.tool : nullptr, sW + 3 * i);
    }
    __syncthreads();
    G_STAMP();  // 2 FK in LDS

    // ---- phase 2: wave = (point half, field slot): every link sphere / pair of the field, folded to joint gradients
    {
        const int half = wv & 1, slot = wv >> 1;
        for (int f = slot; f < n_slots; f += WPT / 2) {
            if (!TOOL || f < gp.n_fields) {
                dev_field fld;
                if constexpr (MULTI_SCENE) fld = scene_field(gp, sc_n, f); else fld = gp.fields[f];
                for (int i = half * 64 + lane; i < N; i += 128) chain_point_field<QD>(gp, fld, sprim, stab, cn, sfk + i * FKS, sG + (f * N + i) * QD);
            } else {   // the tool-axis term (slot n_fields)
                for (int i = half * 64 + lane; i < N; i += 128) chain_point_tool<QD>(ca.tool, stab, sfk + i * FKS, sW + 3 * i, sG + (f * N + i) * QD);
            }
        }
    }
    G_STAMP();  // 3 this wave's forces done
    __syncthreads();
    G_STAMP();  // 4 all waves done

    // the step's noise (last guide iteration, drawn in place): by the waves that do not gather, under the gather.  Element k of the draw is a function
    // of its Philox counter alone: the values do not depend on how many waves draw (four, or three when four fields and the tool term gather)
    const unsigned long long ne0 = a.rng.elem0 + (unsigned long long)b * H * D;
    const int wdraw = TOOL && n_slots > MAXF ? MAXF + 1 : MAXF;
    if (a.rng.on && !a.grad_out && wv >= wdraw) guide_draw_noise(a.rng, ne0, H * D, snz, threadIdx.x - 64 * wdraw, 64 * (WPT - wdraw));

    // ---- phase 3: wave f gathers field f to the support points (transpose of the interpolation, fixed order), clips, weights
    if (wv < gp.n_fields) {
        const int f = wv;
        gather_clip_weight<QD>(gp, f, nsw, lane, H, N, scale, sC, [&](int i, int j) { return sG[(f * N + i) * QD + j]; });
    } else if (TOOL && wv < n_slots) {   // the tool-axis term: a wave of its own, the term's own weight
        const int f = wv;
        gather_clip_weight_as<QD>(gp, f, ca.tool.weight, nsw, lane, H, N, scale, sC, [&](int i, int j) { return sG[(f * N + i) * QD + j]; });
    }
    __syncthreads();
    G_STAMP();  // 5 gathered + clipped
    if (wv >= nsw) return;
    sum_fields_and_apply<QD>(a, n_slots, b, ctx, lane, wv, hs_, H, live, snz_x, sC, snz + (int)(ne0 & 3ull), shc);
}

// The tool-axis figures of mpdx_traj_tool_metrics: one wave per trajectory, lane = checked point (the pattern of traj_metrics_chain_kernel).  The rotation
// recurrence of chain_fk (the same statements; the translations and the spheres are not needed) up to frame f only, d_i = u . Rot_f(q_i) a; out2 =
// {min_i d_i, number of points with d_i < cos_min} by the fixed butterfly; mask (or null): the per-point flags.
template <int QD>
__global__ __launch_bounds__(64) void traj_tool_chain_kernel(const dev_tool tool, const float* __restrict__ x, float* __restrict__ out2, uint8_t* __restrict__ mask,
                                                             int B, int H, int n_check, const float* __restrict__ table, int ntab) {
    constexpr int D = 2 * QD;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x, b = blockIdx.x;
    float* sx = sm;                // [H][D]
    float* stab = sm + H * D;      // the joints of the chain table (header + QD joint records)
    for (int i = lane; i < ntab; i += 64) stab[i] = table[i];
    for (int i = lane; i < H * D; i += 64) sx[i] = x[(size_t)b * H * D + i];
    __syncthreads();
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    const int fr = __builtin_amdgcn_readfirstlane(min(max(tool.frame, 0), QD));
    const int N = n_check;
    const float scale = interp_scale(H, N);
    float dmin = 3.0e38f, nbad = 0.f;
    for (int i = lane; i < N; i += 64) {
        const InterpPair ip = interp_pair(true, scale, i, H);
        const float* qa = sx + ip.i0 * D;
        const float* qb = sx + ip.i1 * D;
        float R[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll 1
        for (int k = 0; k < fr; ++k) {
            const float* J = stab + kChainHdr + k * kChainJF;
            const bool prismatic = __builtin_amdgcn_readfirstlane(tabi[kChainHdr + k * kChainJF + 12]) != 0;
            const float qk = ip.l0 * qa[k] + ip.l1 * qb[k];
            float A[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A[r][c] = R[r][0] * J[c] + R[r][1] * J[3 + c] + R[r][2] * J[6 + c];
            }
            float st = 0.f, ct = 1.f;
            if (!prismatic) { st = sinf(qk); ct = cosf(qk); }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                R[r][0] = A[r][0] * ct + A[r][1] * st;
                R[r][1] = A[r][1] * ct - A[r][0] * st;
                R[r][2] = A[r][2];
            }
        }
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) d += tool.world[r] * (R[r][0] * tool.axis[0] + R[r][1] * tool.axis[1] + R[r][2] * tool.axis[2]);
        const bool bad = d < tool.cos_min;
        dmin = fminf(dmin, d);
        nbad += bad ? 1.f : 0.f;
        if (mask) mask[(size_t)b * N + i] = bad ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        dmin = fminf(dmin, __shfl_xor(dmin, s, 64));
        nbad += __shfl_xor(nbad, s, 64);
    }
    if (lane == 0) { out2[(size_t)b * 2 + 0] = dmin; out2[(size_t)b * 2 + 1] = nbad; }
}

// traj_metrics_kernel (guide.hpp) for a chain: the same out4 and mask; collision flags with the link radii, no margin, over the objects,
// workspace and self fields; path length and smoothness are joint-space figures, computed as there.  One wave per trajectory, lane = interpolated
// waypoint; the waypoint's sphere centres live in LDS (sP, odd stride per lane).
template <int QD, bool MULTI_SCENE>
__global__ __launch_bounds__(64) void traj_metrics_chain_kernel(const dev_guide_params gp, const float* __restrict__ x, float* __restrict__ out, int B, int H, int n_check,
                                                                uint8_t* __restrict__ mask, const dev_scenes scene, const float* __restrict__ table, int ntab) {
    constexpr int D = 2 * QD;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x, b = blockIdx.x;
    const MetricsLds L = metrics_lds_layout(true, H, D, gp.n_prim_floats, ntab);
    float* sx = sm + L.sx;
    float* stab = sm + L.stab;
    float* sP = sm + L.sP;
    float* sprim = sm + L.sprim;
    const SceneCounts sc_n = stage_prims<MULTI_SCENE>(gp, scene, b, sprim, lane, 64);
    for (int i = lane; i < ntab; i += 64) stab[i] = table[i];
    const ChainCounts cn = chain_counts<QD>(table, ntab);
    for (int i = lane; i < H * D; i += 64) sx[i] = x[(size_t)b * H * D + i];
    __syncthreads();
    float plen = 0.f, smooth = 0.f;
    for (int h = lane; h < H - 1; h += 64) {
        float a2 = 0.f, v2 = 0.f;
#pragma unroll
        for (int j = 0; j < QD; ++j) {
            const float dq = sx[(h + 1) * D + j] - sx[h * D + j], dv = sx[(h + 1) * D + QD + j] - sx[h * D + QD + j];
            a2 += dq * dq; v2 += dv * dv;
        }
        plen += sqrtf(a2); smooth += sqrtf(v2);
    }
    const int N = n_check;
    const float scale = interp_scale(H, N);
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    constexpr int SPH = kChainHdr + QD * kChainJF;
    float* P = sP + lane * kChainPS;
    float ncoll = 0.f;
    for (int i = lane; i < N; i += 64) {
        const InterpPair ip = interp_pair(true, scale, i, H);
        chain_fk<QD, false>(stab, cn.ns, sx + ip.i0 * D, sx + ip.i1 * D, ip.l0, ip.l1, nullptr, P);
        bool hit = false;
        for (int f = 0; f < gp.n_fields; ++f) {
            const int kind = gp.fields[f].kind;
            if (kind == MPDX_FIELD_SELF) {
                const int pr0 = SPH + cn.ns * kChainSF;
                for (int pr = 0; pr < cn.np; ++pr) {
                    const int sa = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr], 0), cn.ns - 1));
                    const int sb = __builtin_amdgcn_readfirstlane(min(max(tabi[pr0 + 2 * pr + 1], 0), cn.ns - 1));
                    const float dx = P[sa * 3] - P[sb * 3], dy = P[sa * 3 + 1] - P[sb * 3 + 1], dz = P[sa * 3 + 2] - P[sb * 3 + 2];
                    hit |= sqrtf(dx * dx + dy * dy + dz * dz) < stab[SPH + sa * kChainSF + 4] + stab[SPH + sb * kChainSF + 4];
                }
            } else if (kind == MPDX_FIELD_OBJECTS || kind == MPDX_FIELD_WORKSPACE) {
                dev_field fld;
                if constexpr (MULTI_SCENE) fld = scene_field(gp, sc_n, f); else fld = gp.fields[f];
                for (int s = 0; s < cn.ns; ++s) {
                    const float rad = stab[SPH + s * kChainSF + 4];
                    const float p3[3] = {P[s * 3], P[s * 3 + 1], P[s * 3 + 2]};
                    if (kind == MPDX_FIELD_OBJECTS) hit |= objects_sdf<3>(sprim, fld, p3) < rad;
                    else {
#pragma unroll
                        for (int j = 0; j < 3; ++j) hit |= (p3[j] - fld.ws_min[j] < rad) || (fld.ws_max[j] - p3[j] < rad);
                    }
                }
            }
        }
        ncoll += hit ? 1.f : 0.f;
        if (mask) mask[(size_t)b * N + i] = hit ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        ncoll += __shfl_xor(ncoll, s, 64);
        plen += __shfl_xor(plen, s, 64);
        smooth += __shfl_xor(smooth, s, 64);
    }
    if (lane == 0) {
        out[(size_t)b * 4 + 0] = ncoll; out[(size_t)b * 4 + 1] = plen; out[(size_t)b * 4 + 2] = smooth; out[(size_t)b * 4 + 3] = (float)N;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// what the launchers know of a validated chain table
struct ChainInfo { int n_joints, n_spheres, n_pairs, n_floats; };

inline int chain_table_floats(int nj, int ns, int np) { return kChainHdr + nj * kChainJF + ns * kChainSF + 2 * np; }

// The checks of a chain table held in HOST memory (t: gp.n_chain_floats floats) against its parameter block: nullptr = fine (*info filled), else
// what is wrong, naming the member at fault.  After them every offset the kernels form lies inside the table.
inline const char* chain_table_problem(const mpdx_guide_params& gp, const float* t, ChainInfo* info) {
    static thread_local char msg[200];
    const int32_t* ti = reinterpret_cast<const int32_t*>(t);
    const int nj = ti[0], ns = ti[1], np = ti[2];
    if (nj < 1 || nj > MPDX_ROBOT_CHAIN_MAX_JOINTS) { snprintf(msg, sizeof(msg), "chain: n_joints %d outside 1 ... %d (MPDX_ROBOT_CHAIN_MAX_JOINTS)", nj, MPDX_ROBOT_CHAIN_MAX_JOINTS); return msg; }
    if (ns < 1 || ns > kChainMaxS) { snprintf(msg, sizeof(msg), "chain: n_spheres %d outside 1 ... %d (MPDX_ROBOT_CHAIN_MAX_SPHERES)", ns, kChainMaxS); return msg; }
    if (np < 0 || np > kChainMaxP) { snprintf(msg, sizeof(msg), "chain: n_pairs %d outside 0 ... %d (MPDX_ROBOT_CHAIN_MAX_PAIRS)", np, kChainMaxP); return msg; }
    const int need = chain_table_floats(nj, ns, np);
    if (gp.n_chain_floats < need) { snprintf(msg, sizeof(msg), "chain: n_chain_floats %d does not cover the table (%d floats for %d joints, %d spheres, %d pairs)", gp.n_chain_floats, need, nj, ns, np); return msg; }
    if (gp.q_dim != nj) { snprintf(msg, sizeof(msg), "chain: q_dim %d != n_joints %d of the chain table", gp.q_dim, nj); return msg; }
    for (int j = 0; j < nj; ++j) {
        const float* J = t + kChainHdr + j * kChainJF;
        const int type = ti[kChainHdr + j * kChainJF + 12];
        if (type != MPDX_ROBOT_CHAIN_REVOLUTE && type != MPDX_ROBOT_CHAIN_PRISMATIC) { snprintf(msg, sizeof(msg), "chain: joint %d type %d (0 = revolute, 1 = prismatic)", j, type); return msg; }
        for (int r = 0; r < 3; ++r)
            for (int c = r; c < 3; ++c) {
                float d = 0.f;
                for (int k = 0; k < 3; ++k) d += J[r * 3 + k] * J[c * 3 + k];
                if (!(fabsf(d - (r == c ? 1.f : 0.f)) <= 1e-4f)) { snprintf(msg, sizeof(msg), "chain: joint %d R is not orthonormal to 1e-4 (rows %d . %d = %g)", j, r, c, (double)d); return msg; }
            }
        for (int k = 9; k < 12; ++k)
            if (!(fabsf(J[k]) < 3.0e38f)) { snprintf(msg, sizeof(msg), "chain: joint %d t is not finite", j); return msg; }
    }
    for (int s = 0; s < ns; ++s) {
        const float* S = t + kChainHdr + nj * kChainJF + s * kChainSF;
        const int fr = ti[kChainHdr + nj * kChainJF + s * kChainSF];
        if (fr < 0 || fr > nj) { snprintf(msg, sizeof(msg), "chain: sphere %d frame %d outside 0 ... n_joints (%d)", s, fr, nj); return msg; }
        if (!(S[4] > 0.f) || !(S[4] < 3.0e38f)) { snprintf(msg, sizeof(msg), "chain: sphere %d radius must be positive and finite", s); return msg; }
        for (int k = 1; k < 4; ++k)
            if (!(fabsf(S[k]) < 3.0e38f)) { snprintf(msg, sizeof(msg), "chain: sphere %d offset is not finite", s); return msg; }
    }
    for (int p = 0; p < np; ++p) {
        const int a = ti[kChainHdr + nj * kChainJF + ns * kChainSF + 2 * p], b = ti[kChainHdr + nj * kChainJF + ns * kChainSF + 2 * p + 1];
        if (a < 0 || a >= ns || b < 0 || b >= ns) { snprintf(msg, sizeof(msg), "chain: pair %d indices (%d, %d) outside n_spheres (%d)", p, a, b, ns); return msg; }
    }
    for (int f = 0; f < gp.n_fields && f < MPDX_MAX_FIELDS; ++f)
        if (gp.fields[f].kind == MPDX_FIELD_SELF && np == 0) return "chain: a MPDX_FIELD_SELF field needs n_pairs > 0 in the chain table";
    info->n_joints = nj; info->n_spheres = ns; info->n_pairs = np; info->n_floats = need;
    return nullptr;
}

// ---- k_guide.hip: the checks of a MPDX_ROBOT_CHAIN block, the table read where it lies (a device table: copied to the host once per (pointer, size))
const char* chain_params_check(const mpdx_guide_params& gp, ChainInfo* info);
// the checks of the tool members (nothing is dereferenced): nullptr = fine or no tool term (tool_frame == 0), else what is wrong, naming the member.
// For a chain robot call it behind chain_params_check (q_dim == n_joints by then).
const char* tool_params_problem(const mpdx_guide_params& gp);
// ---- k_chain.hip: every guide_step_chain_kernel / traj_metrics_chain_kernel / traj_tool_chain_kernel instantiation
int launch_chain_guide(const GuideArgs& a, const dev_tool& tool, const float* table, const ChainInfo& ci, bool multi, size_t lds, int B, hipStream_t st);
int launch_chain_tool_metrics(const dev_tool& tool, const float* x, float* out2, uint8_t* mask, int n_check, int B, int H, const float* table, const ChainInfo& ci,
                              hipStream_t st);
int launch_chain_metrics(const dev_guide_params& g, const float* x, float* out4, uint8_t* mask, int n_check, int B, int H, const dev_scenes& sc, const float* table,
                         const ChainInfo& ci, bool multi, hipStream_t st);

}  // namespace mpdx
