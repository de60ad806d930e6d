// guide_common.hpp - what the guide, metrics and baseline-planner kernels share (guide.hpp, chain.hpp, planner.hpp): the align_corners
// interpolation pair, the staging of the primitive table, of the hard conditions and of the state, the support window of the gather, the stamp
// macro, the dynamic-LDS layout of each kernel family (ONE function, read by the kernel's carve and by its launcher's byte count), and the
// launchers' run-time -> compile-time dispatch.
//
// Replaces nothing in the reference by itself: every helper is a phase of the kernels named above, moved here verbatim (same statements, same
// rounding: nothing re-associated, no product moved into or out of the statement that adds it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/mpdx.h"
#include "conv_block.hpp"
#include "scene_table.hpp"

namespace mpdx {

// cycle stamp of the guide kernels (dev tool, mpdx_guide_trace): slot tr_i of the wave's 16, workgroup 0 only.  Uses the kernel's a, b, lane, wv, tr_i.
#define G_STAMP() do { if (MPDX_TRACE_PTR(a.trace) && b == 0 && lane == 0) a.trace[wv * 16 + tr_i] = (long long)__builtin_readcyclecounter(); ++tr_i; } while (0)

// ---- interpolation H support points -> N points, align_corners=True (interpolate_points_v1, guides.py:184)
__device__ __forceinline__ float interp_scale(int H, int N) { return (N > 1) ? (float)(H - 1) / (float)(N - 1) : 0.f; }

// point i = l0 * support i0 + l1 * support i1  (interpolate == false: the point IS support i)
struct InterpPair { int i0, i1; float l0, l1; };
__device__ __forceinline__ InterpPair interp_pair(bool interpolate, float scale, int i, int H) {
    InterpPair p = {i, i, 1.f, 0.f};
    if (interpolate) {
        const float u = scale * (float)i;
        p.i0 = (int)u;
        if (p.i0 > H - 1) p.i0 = H - 1;
        p.i1 = p.i0 + 1 < H ? p.i0 + 1 : H - 1;
        p.l1 = u - (float)p.i0;
        p.l0 = 1.0f - p.l1;
    }
    return p;
}

// the points ilo ... ihi that can touch support hg: those of the segments (hg-1, hg) and (hg, hg+1), any number per segment
struct SupportWindow { int ilo, ihi; };
__device__ __forceinline__ SupportWindow support_window(int hg, float scale, int N, bool interpolate) {
    SupportWindow w = {hg, hg};
    if (interpolate && scale > 0.f) {
        w.ilo = (int)((float)(hg - 1) / scale) - 1;
        w.ihi = (int)((float)(hg + 1) / scale) + 1;
        if (w.ilo < 0) w.ilo = 0;
        if (w.ihi > N - 1) w.ihi = N - 1;
    }
    return w;
}

// ---- the primitive table into LDS: the whole table, or (MULTI_SCENE, scene_table.hpp) the block of trajectory b's scene + the shared tail.
// Returns the scene's primitive counts (read by the MULTI_SCENE instantiations only).
__device__ __forceinline__ void stage_prims(const dev_guide_params& gp, float* __restrict__ sprim, int tid, int nthr) {
    for (int i = tid; i < gp.n_prim_floats; i += nthr) sprim[i] = gp.prims[i];
}
template <bool MULTI_SCENE>
__device__ __forceinline__ SceneCounts stage_prims(const dev_guide_params& gp, const dev_scenes& scene, int b, float* __restrict__ sprim, int tid, int nthr) {
    SceneCounts sc_n = {};
    if constexpr (MULTI_SCENE) {
        const int s = scene_of_traj(scene, b);
        sc_n = scene_counts(gp, gp.prims + (size_t)s * scene.stride);
        stage_scene_table(gp, scene, s, sprim, tid, nthr);
    } else {
        stage_prims(gp, sprim, tid, nthr);
    }
    return sc_n;
}

// ---- one element of the state, unnormalised (normalization.py:156-167).  identity_normalizer: 0 limits (incl. the whole-tensor range test `clipall`),
// 1 Identity (:111-116), 2 GaussianNormalizer (:140-141: x * stds + means - the host passes means in `mins` = lo, stds in `maxs` = hi; no range test)
__device__ __forceinline__ float unnormalise_one(int identity_normalizer, float xn, float lo, float hi, bool clipall) {
    const float c = clipall ? fminf(fmaxf(xn, -1.f), 1.f) : xn;
    const float u01 = __fadd_rn(c, 1.0f) * 0.5f;
    return identity_normalizer == 1 ? xn : identity_normalizer == 2 ? __fadd_rn(__fmul_rn(xn, hi), lo) : __fadd_rn(__fmul_rn(u01, __fsub_rn(hi, lo)), lo);
}

// The same element in float64 from the float32 normalised value (the GP prior: guide_gp_apply).  The limits stay float32 and so does their difference:
// that is what a float64 evaluation of normalization.py gives, whose mins / maxs are float32 tensors.
__device__ __forceinline__ double unnormalise_one_f64(int identity_normalizer, float xn, float lo, float hi, bool clipall) {
    const float c = clipall ? fminf(fmaxf(xn, -1.f), 1.f) : xn;
    const double u01 = ((double)c + 1.0) * 0.5;
    return identity_normalizer == 1 ? (double)xn : identity_normalizer == 2 ? (double)xn * (double)hi + (double)lo : u01 * (double)__fsub_rn(hi, lo) + (double)lo;
}

// ---- this trajectory's hard conditions into shc: [start | goal] x D (apply mode only); their loads fly with the state's
__device__ __forceinline__ void stage_hard_conds(const float* __restrict__ hs, const float* __restrict__ hg, bool apply, int b, int D, float* __restrict__ shc) {
    if (apply && (int)threadIdx.x < 2 * D) {
        const int which = (int)threadIdx.x >= D ? 1 : 0, d = (int)threadIdx.x - which * D;
        const float* p = which ? hg : hs;
        if (p) shc[which * D + d] = p[(size_t)b * D + d];
    }
}

// ---- load + unnormalise by the whole workgroup of NTHR threads: the trajectory's n = H * D floats are CONTIGUOUS - coalesced loads into LDS (sxn:
// the normalised state, kept for the last phase), then element-wise unnormalisation into sx, the limits fetched per element through the lane
// crossbar.  Dword loads: H * D need not be a multiple of 4 (the Panda kernel, whose launcher demands it, keeps its own copy with 16-byte loads:
// guide.hpp).  Contains one workgroup barrier.
template <int D, int NTHR>
__device__ __forceinline__ void stage_state_unnormalised(const dev_guide_params& gp, const float* __restrict__ xb, int n, bool clipall, float* __restrict__ sx,
                                                         float* __restrict__ sxn, int lane) {
    for (int i = threadIdx.x; i < n; i += NTHR) sxn[i] = xb[i];
    float mn = 0.f, mx = 0.f;   // the limits, one per lane (static index -> scalar loads)
#pragma unroll
    for (int d = 0; d < D; ++d) { mn = lane == d ? gp.mins[d] : mn; mx = lane == d ? gp.maxs[d] : mx; }
    __syncthreads();
    for (int i = threadIdx.x; i < ((n + NTHR - 1) / NTHR) * NTHR; i += NTHR) {   // (whole waves take part in the shuffles)
        const int ic = i < n ? i : 0, d = ic % D;
        const float lo = __shfl(mn, d, 64), hi = __shfl(mx, d, 64);
        const float xud = unnormalise_one(gp.identity_normalizer, sxn[ic], lo, hi, clipall);
        if (i < n) sx[i] = xud;
    }
}

// ---- dynamic-LDS layouts: float offsets of every region and the total, per kernel family.  The kernels carve from them; the launchers size the
// launch (and refuse it) by .total * sizeof(float).
constexpr int kPandaFKS = 75;   // floats per interpolated point of the Panda's FK table: O[7][3] | Z[7][3] | P[11][3]  (odd stride: no bank conflicts)
constexpr int kPandaParts = 4;  // sphere / pair groups of the Panda kernel (guide.hpp)
// MPDX_ROBOT_CHAIN (chain.hpp): floats per interpolated point of the FK table, O[QD][3] | Z[QD][3] | P[MPDX_ROBOT_CHAIN_MAX_SPHERES][3]  (odd stride)
constexpr int chain_fk_stride(int qd) { return 6 * qd + 3 * MPDX_ROBOT_CHAIN_MAX_SPHERES + 1; }
constexpr int kChainPS = 3 * MPDX_ROBOT_CHAIN_MAX_SPHERES + 1;   // chain metrics: floats per lane of the sphere-centre table (odd stride)

__host__ __device__ constexpr int round_up4(int n) { return (n + 3) & ~3; }

enum GuideKind { kGuidePointMass, kGuidePandaSparse, kGuidePandaDense, kGuideChain };
struct GuideLds {
    int sx;           // [H][D] unnormalised state
    int sA, sB;       // point mass: [MAXF][N][QD] point forces weighted l0 / l1 (sC overlays sB)
    int stab;         // chain: the chain table
    int sfk;          // Panda sparse, chain: [N][stride] FK record per interpolated point
    int sW;           // chain with the tool-axis term: [N][3] the tool axis in the world, the part of a point's FK record the term adds (odd stride)
    int sG;           // Panda: [MAXF][parts][N][QD], chain: [MAXF (+ 1 with the tool term)][N][QD]  joint gradients per point
    int sC;           // [MAXF (+ 1: chain with the tool term)][H][QD] clipped, weighted per-field support-point gradients
    int snz, snz_x;   // Panda, chain: 16-byte aligned [H * D + pad] the step's noise, drawn in whole groups of four | all: [H * D] the normalised state
    int sprim, shc;   // the primitive table | Panda, chain: [2][D] hard conditions
    size_t total;
};
// n_prim / n_tab: the floats a workgroup stages of the primitive table / the chain table.  total of the Panda and chain layouts: every round-up to
// 16 bytes is counted as + 3 floats, as the launchers always have (the 80-KB dense and 160-KB refusal thresholds were set with it): >= shc + 2 D.
// tool (chain only): the tool-axis term is on - a fifth gradient slot in sG and sC and [N][3] floats of FK record (sW); off: the offsets and the total
// are what they were before the term existed.
__host__ __device__ inline GuideLds guide_lds_layout(GuideKind kind, int H, int D, int N, int n_prim, int n_tab = 0, bool tool = false) {
    constexpr int MAXF = MPDX_MAX_FIELDS;
    const int QD = D / 2;
    GuideLds l = {};
    if (kind == kGuidePointMass) {
        l.sA = H * D;
        l.sB = l.sA + MAXF * N * QD;
        l.sC = l.sB;
        l.sprim = l.sB + MAXF * N * QD;
        l.snz_x = l.sprim + round_up4(n_prim);
        l.total = (size_t)l.snz_x + (size_t)H * D;
        return l;
    }
    const bool chain = kind == kGuideChain;
    const int pad = chain ? 8 : 4;   // (chain: H * D need not be a multiple of 4, the draw starts up to 3 floats early and ends up to 3 late)
    const int slots = MAXF + (chain && tool ? 1 : 0);
    l.stab = H * D;
    l.sfk = l.stab + (chain ? round_up4(n_tab) : 0);
    l.sW = l.sfk + (chain ? N * chain_fk_stride(QD) : kind == kGuidePandaSparse ? N * kPandaFKS : 0);
    l.sG = l.sW + (chain && tool ? 3 * N : 0);
    l.sC = l.sG + slots * (chain ? 1 : kPandaParts) * N * QD;
    l.snz = round_up4(l.sC + slots * H * QD);
    l.snz_x = l.snz + H * D + pad;
    l.sprim = l.snz_x + H * D;
    l.shc = l.sprim + round_up4(n_prim);
    l.total = (size_t)H * D + (size_t)(chain ? n_tab + 3 : 0) + (size_t)(l.sC - l.sfk) + (size_t)slots * H * QD + (size_t)(2 * H * D + pad + 3) + (size_t)n_prim + 3 + 2 * D;
    return l;
}

struct MetricsLds { int sx, stab, sP, sprim; size_t total; };   // state | chain: table | chain: [64][kChainPS] sphere centres | primitives
__host__ __device__ inline MetricsLds metrics_lds_layout(bool chain, int H, int D, int n_prim, int n_tab = 0) {
    MetricsLds l = {};
    l.stab = H * D;
    l.sP = l.stab + (chain ? round_up4(n_tab) : 0);
    l.sprim = l.sP + (chain ? 64 * kChainPS : 0);
    l.total = (size_t)l.sprim + (size_t)n_prim;
    return l;
}

// ---- host side: run-time booleans / the built-in robot -> template arguments of a generic lambda
template <class F>
inline auto with_bools(F&& fn) { return fn(); }
// fn(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): one instantiation of fn per combination of the booleans given
template <class F, class... Bs>
inline auto with_bools(F&& fn, bool b0, Bs... rest) {
    return b0 ? with_bools([&](auto... c) { return fn(std::true_type{}, c...); }, rest...)
              : with_bools([&](auto... c) { return fn(std::false_type{}, c...); }, rest...);
}

// fn(QD, DIM, ROBOT) as integral constants for the three built-in robots; false: the block names none of them (fn not called).
// match_ws = false: the robot is chosen by (robot, q_dim) alone, as the baseline planners always have.
template <class F>
inline bool with_builtin_robot(const mpdx_guide_params& gp, F&& fn, bool match_ws = true) {
    using std::integral_constant;
    if (gp.robot == MPDX_ROBOT_POINTMASS && gp.q_dim == 2 && (!match_ws || gp.ws_dim == 2)) fn(integral_constant<int, 2>{}, integral_constant<int, 2>{}, integral_constant<int, MPDX_ROBOT_POINTMASS>{});
    else if (gp.robot == MPDX_ROBOT_POINTMASS && gp.q_dim == 3 && (!match_ws || gp.ws_dim == 3)) fn(integral_constant<int, 3>{}, integral_constant<int, 3>{}, integral_constant<int, MPDX_ROBOT_POINTMASS>{});
    else if (gp.robot == MPDX_ROBOT_PANDA && gp.q_dim == 7 && (!match_ws || gp.ws_dim == 3)) fn(integral_constant<int, 7>{}, integral_constant<int, 3>{}, integral_constant<int, MPDX_ROBOT_PANDA>{});
    else return false;
    return true;
}

}  // namespace mpdx
