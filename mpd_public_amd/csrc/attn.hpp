// attn.hpp - Residual(PreNorm(dim, LinearAttention(dim))) of a self_attention=True TemporalUnet (layers.py:174-226) as ONE launch,
// in place on the channel-last activation [B][L][C] of a U-Net level.
//
//   xn  = (x - mean_c) / sqrt(var_c + 1e-5) * g + b                per position, over the C channels       (layers.py:201-204)
//   qkv = W_qkv xn   (384 x C, no bias) -> q, k, v of 4 heads x 32 channels; q *= 32^-0.5                   (layers.py:217-219)
//   k   = softmax(k) along the positions of each row                                                       (layers.py:221)
//   ctx[d][e] = sum_n k[d][n] v[e][n];   out[e][n] = sum_d ctx[d][e] q[d][n]        per head                (layers.py:222-224)
//   y   = W_out out + b_out + x                                                                            (layers.py:226, :180)
//
// A workgroup of four waves owns NC = G * L consecutive rows of the activation (G whole trajectories; G = 1 from 64 positions on)
// and walks the four heads.  Every contraction is exact fp32 on v_mfma_f32_16x16x4_f32:
//   projection  D[row][pos] : A = packed weight fragments (pack_conv_weights_kernel's order, one tap), B = xn rows out of LDS (b128)
//   context     D[d][e]     : A = k[d][n], B = v[e][n] out of LDS, the K index runs over the trajectory's VALID positions
//   out         D[e][n]     : A = the context's D registers as they are (D's (4 rows x column) per lane IS an A fragment of the transposed
//                             matrix), B = q[n][d] out of LDS
//   to_out      D[c][pos]   : accumulated over the heads in registers, A = packed weight fragments, B = out[n][e] out of LDS
// A trajectory's numbers depend on nothing but its own rows: the columns of an MFMA are independent, the softmax reduces with a fixed
// butterfly, there are no atomics - so a result does not depend on the batch or on the trajectory's place in it.
// Zero-padded containers (Lv < L): the softmax and with it the context sum see the valid positions only (pad positions of k are stored as
// exact zeros), and the pad rows of the result are stored as zeros.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_block.hpp"

namespace mpdx {

constexpr int kAttnThreads = 256;
constexpr int kAttnHeads = 4, kAttnDh = 32, kAttnHid = kAttnHeads * kAttnDh;   // LinearAttention's own defaults (layers.py:208)
constexpr int kAttnQS = kAttnDh + 4;   // row stride of the position-major q / out buffers

struct AttnArgs {
    float* x;            // [B][L][C], in place
    const float* wqkv;   // to_qkv.weight, A-fragment order [24][C/16][1][64][4]
    const float* wout;   // to_out.weight, A-fragment order [C/16][8][1][64][4]
    const float* bout;   // [C]
    const float* g;      // [C] LayerNorm scale
    const float* b;      // [C] LayerNorm shift
    int B, L, Lv, C;
    int G, NC;           // trajectories / rows per workgroup (NC = G * L, a multiple of 16)
    int rsx;             // row stride (floats) of the normalised input in LDS
};

// rows per workgroup: whole trajectories, at least one MFMA tile of 16 columns, at most 64 columns unless a trajectory is longer, and at most
// 8192 floats of normalised input (a longer trajectory excepted) - which keeps the to_out accumulator at 32 tiles, 64 for those
inline int attn_cols(int C, int L) {
    int nc = std::max(16, std::min(64, 8192 / C));
    return std::max(nc, L);
}
inline size_t attn_lds_bytes(int C, int L, int rsx) {
    const int NC = attn_cols(C, L);
    return ((size_t)NC * rsx + 2 * (size_t)NC * kAttnQS + 2 * (size_t)kAttnDh * (NC + 4) + 16) * sizeof(float);
}

// MAXT: to_out accumulator tiles per wave ((C / 16) * (NC / 16) <= 4 * MAXT).  Three workgroups per CU for MAXT = 8 (147 VGPRs, no AGPRs, no scratch;
// left to itself the compiler takes 148 + 48 and two fit: 2965 -> 2564 us over the eight blocks of a pass at B = 6400, profiles/attention_probe.md)
template <int MAXT>
__global__ __launch_bounds__(kAttnThreads, MAXT <= 8 ? 3 : 2) void attn_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int C = a.C, L = a.L, Lv = a.Lv, NC = a.NC, G = a.G, rsx = a.rsx;
    const int KS = NC + 4;                       // row stride of the channel-major k / v buffers
    float* xn = sm;                              // [NC][rsx]
    float* qs = xn + (size_t)NC * rsx;           // [NC][36]   q of the head, position-major
    float* os = qs + (size_t)NC * kAttnQS;       // [NC][36]   out of the head, position-major
    float* ks = os + (size_t)NC * kAttnQS;       // [32][NC+4] k of the head, channel-major
    float* vs = ks + (size_t)kAttnDh * KS;       // [32][NC+4] (+ 16 floats of slack behind it: masked fragment reads may run past a row)
    const size_t row0 = (size_t)blockIdx.x * NC;                 // first activation row of this workgroup
    const int b0 = blockIdx.x * G;
    const int g_live = min(G, a.B - b0);                         // trajectories that exist
    const int rows_live = g_live * L;
    float* xg = a.x + row0 * C;

    // ---------------------------------------------------------------- LayerNorm over the channels of every row -> xn
    {
        const int c4n = C >> 2;
        const int S = min(64, c4n);              // lanes per row
        const int EPL = c4n / S;                 // float4 per lane (1; 2 at 512 channels)
        const int rpw = 64 / S;                  // rows per wave and iteration
        const int sl = lane & (S - 1);
        const float inv_c = 1.0f / (float)C;
        for (int r = wave * rpw + lane / S; r < NC; r += 4 * rpw) {
            f32x4 v[2];
            const bool live = r < rows_live;
#pragma unroll
            for (int e = 0; e < 2; ++e)
                v[e] = (live && e < EPL) ? *(const f32x4*)(xg + (size_t)r * C + (e * S + sl) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
            float s = (v[0][0] + v[0][1]) + (v[0][2] + v[0][3]) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
            for (int m = 1; m < S; m <<= 1) s += __shfl_xor(s, m, 64);
            const float mean = s * inv_c;
            float s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (e < EPL)
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const float d = v[e][k] - mean; s2 = fmaf(d, d, s2); }
            for (int m = 1; m < S; m <<= 1) s2 += __shfl_xor(s2, m, 64);
            const float sd = sqrtf(s2 * inv_c + 1e-5f);
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (e < EPL) {
                    const int c = (e * S + sl) * 4;
                    const f32x4 gg = *(const f32x4*)(a.g + c), bb = *(const f32x4*)(a.b + c);
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = live ? __fadd_rn(__fmul_rn((v[e][k] - mean) / sd, gg[k]), bb[k]) : 0.f;
                    *(f32x4*)(xn + (size_t)r * rsx + c) = o;
                }
        }
    }
    if (tid < 16) vs[(size_t)kAttnDh * KS + tid] = 0.f;
    __syncthreads();

    const int nc16 = C >> 4, nt_n = NC >> 4;
    const int n_out_tiles = nc16 * nt_n;         // to_out tiles (channel tile, column tile), tile t = wave + 4 i
    f32x4 yacc[MAXT];
#pragma unroll
    for (int i = 0; i < MAXT; ++i) yacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4* wq4 = (const f32x4*)a.wqkv;
    const f32x4* wo4 = (const f32x4*)a.wout;
    const float qscale = 0.17677669529663687f;   // 32 ** -0.5 rounded to fp32, as the reference's python float times an fp32 tensor gives

    for (int h = 0; h < kAttnHeads; ++h) {
        // ------------------------------------------------------------ q, k, v of head h: 6 row tiles x NC / 16 column tiles.  A work item is a row
        // tile on NG column tiles: the weight fragments of a step are loaded once for all of them, two channel chunks per step, the next step's
        // fragments requested before this step's MFMAs (unconditional, clamped loads: nothing in the loop waits for memory it has just asked for)
        const int NG = nt_n >= 4 ? nt_n >> 1 : 1, n_grp = nt_n / NG;
        for (int t = wave; t < 6 * n_grp; t += 4) {
            const int mt = t / n_grp, nt0 = (t - mt * n_grp) * NG;
            const int part = mt >> 1, half = mt & 1;             // 0 q, 1 k, 2 v
            const int m16 = part * 8 + h * 2 + half;
            const f32x4* wp = wq4 + (size_t)m16 * nc16 * 64 + lane;
            const float* bp = xn + (size_t)(nt0 * 16 + j) * rsx + 4 * q;
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 a0 = wp[0], a1 = wp[64];
            for (int c0 = 0; c0 < nc16; c0 += 2) {               // (C >= 32: an even number of 16-channel chunks)
                const int cn = min(c0 + 2, nc16 - 2);
                const f32x4 n0 = wp[(size_t)cn * 64], n1 = wp[(size_t)(cn + 1) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < NG) {
                        const f32x4 b0 = *(const f32x4*)(bp + (size_t)i * 16 * rsx + c0 * 16), b1 = *(const f32x4*)(bp + (size_t)i * 16 * rsx + c0 * 16 + 16);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b0[e], acc[i], 0, 0, 0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b1[e], acc[i], 0, 0, 0);
                    }
                a0 = n0; a1 = n1;
            }
            // the lane holds channels half * 16 + 4 q ... + 3 of the head at column (nt0 + i) * 16 + j
            const int ch = half * 16 + 4 * q;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < NG) {
                    const int n = (nt0 + i) * 16 + j;
                    if (part == 0) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][e] = __fmul_rn(acc[i][e], qscale);
                        *(f32x4*)(qs + (size_t)n * kAttnQS + ch) = acc[i];
                    } else {
                        float* dstp = (part == 1 ? ks : vs) + (size_t)ch * KS + n;
#pragma unroll
                        for (int e = 0; e < 4; ++e) dstp[(size_t)e * KS] = acc[i][e];
                    }
                }
        }
        __syncthreads();

        // ------------------------------------------------------------ softmax of every k row over the trajectory's valid positions
        {
            const int S = min(64, L), EPL = L / S, rpw = 64 / S;
            const int sl = lane & (S - 1);
            for (int r = wave * rpw + lane / S; r < kAttnDh * G; r += 4 * rpw) {
                const int d = r & (kAttnDh - 1), g = r >> 5;
                float* kp = ks + (size_t)d * KS + g * L;
                float v[2];
                float m = -INFINITY;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int p = e * S + sl;
                    const bool ok = e < EPL && p < Lv;
                    v[e] = ok ? kp[p] : -INFINITY;
                    m = fmaxf(m, v[e]);
                }
                for (int k = 1; k < S; k <<= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    v[e] = (e < EPL && e * S + sl < Lv) ? expf(v[e] - m) : 0.f;
                    s += v[e];
                }
                for (int k = 1; k < S; k <<= 1) s += __shfl_xor(s, k, 64);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                    if (e < EPL) kp[e * S + sl] = v[e] / s;   // (pad positions: exact zeros)
            }
        }
        __syncthreads();

        // ------------------------------------------------------------ context and out: one (trajectory, half of the e channels) per wave turn
        for (int u = wave; u < 2 * G; u += 4) {
            const int g = u >> 1, et = u & 1;
            f32x4 ctx[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // ctx[dt]: rows d = dt * 16 + 4 q ..., column e = et * 16 + j
            const float* vp = vs + (size_t)(et * 16 + j) * KS + g * L;
            for (int n0 = 0; n0 < Lv; n0 += 16) {
                const int p = n0 + 4 * q;
                f32x4 bf;
#pragma unroll
                for (int e = 0; e < 4; ++e) bf[e] = (p + e < Lv) ? vp[p + e] : 0.f;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const float* kp = ks + (size_t)(dt * 16 + j) * KS + g * L;
                    f32x4 af;
#pragma unroll
                    for (int e = 0; e < 4; ++e) af[e] = (p + e < Lv) ? kp[p + e] : 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) ctx[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bf[e], ctx[dt], 0, 0, 0);
                }
            }
            // out[e][n] = sum_d ctx[d][e] q[d][n]: the lane's ctx registers (d = dt * 16 + 4 q + r, e = et * 16 + j) are the A fragment (row e, k = d)
            const int c0 = g * L;                                 // first column of the trajectory
            for (int nt = c0 >> 4; nt * 16 < c0 + L; ++nt) {
                const float* qp = qs + (size_t)(nt * 16 + j) * kAttnQS + 4 * q;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const f32x4 bf = *(const f32x4*)(qp + dt * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ctx[dt][e], bf[e], acc, 0, 0, 0);
                }
                const int n = nt * 16 + j;
                if (n >= c0 && n < c0 + L) *(f32x4*)(os + (size_t)n * kAttnQS + et * 16 + 4 * q) = acc;
            }
        }
        __syncthreads();

        // ------------------------------------------------------------ to_out: the head's 32 of the 128 hidden channels.  Four tiles at a time: their
        // eight weight fragments are requested together (unconditional, clamped) ahead of the MFMAs - one wait for memory per four tiles
#pragma unroll
        for (int i0 = 0; i0 < MAXT; i0 += 4) {
            if (wave + 4 * i0 < n_out_tiles) {
                f32x4 af[4][2];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ct = min(wave + 4 * (i0 + i), n_out_tiles - 1) / nt_n;
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) af[i][kc] = wo4[((size_t)ct * (kAttnHid / 16) + h * 2 + kc) * 64 + lane];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = wave + 4 * (i0 + i);
                    if (t < n_out_tiles) {
                        const int nt = t - (t / nt_n) * nt_n;
                        const float* op = os + (size_t)(nt * 16 + j) * kAttnQS + 4 * q;
#pragma unroll
                        for (int kc = 0; kc < 2; ++kc) {
                            const f32x4 bf = *(const f32x4*)(op + kc * 16);
#pragma unroll
                            for (int e = 0; e < 4; ++e) yacc[i0 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][kc][e], bf[e], yacc[i0 + i], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // (no barrier: the next head's projection writes q / k / v, which nobody reads any more; `os` is written again two barriers later)
    }

    // ---------------------------------------------------------------- + bias + x, pad rows as zeros
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
        const int t = wave + 4 * i;
        if (t < n_out_tiles) {
            const int ct = t / nt_n, nt = t - ct * nt_n;
            const int n = nt * 16 + j, c = ct * 16 + 4 * q;
            if (n < rows_live) {
                float* p = xg + (size_t)n * C + c;
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if ((n & (L - 1)) < Lv) {
                    const f32x4 xv = *(const f32x4*)p, bo = *(const f32x4*)(a.bout + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(__fadd_rn(yacc[i][e], bo[e]), xv[e]);
                }
                *(f32x4*)p = o;
            }
        }
    }
}

}  // namespace mpdx
