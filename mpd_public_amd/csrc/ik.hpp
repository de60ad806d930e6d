// ik.hpp - batched damped-least-squares (Levenberg-Marquardt) inverse kinematics for a serial chain given as a table (MPDX_ROBOT_CHAIN,
// include/mpdx.h): n targets x R restarts in one launch (mpdx_ik_solve; the arithmetic is documented there, step by step).
//
// Replaces nothing in the reference: it takes every goal as a joint configuration (scripts/inference/inference.py:161 draws one with
// task.random_coll_free_q); a task-space goal for a table-driven robot is this package's extension.
//
// Mapping.  One lane owns one restart from its seed to its last iteration: there is no cross-lane data flow.  A 64-thread workgroup is 64
// restarts of one target, the grid is (ceil(R / 64), n).  The header and the joint records of the table are staged into LDS once per workgroup
// and read at wave-uniform addresses (the link spheres and pairs are not needed).  The number of joints QD is a template parameter (1 ... 8);
// the frame is a run-time, wave-uniform value that only predicates the unrolled joint loops, so every per-joint array (O_j, z_j, the Jacobian
// columns, the QD x QD normal matrix and its Cholesky factor) is indexed by unrolled counters and lives in registers: no scratch, no atomics,
// no LDS beyond the table.  The iteration loop ends when no lane of the wave is still running (a wave-uniform exit); a lane that has finished
// keeps its state - it goes through the arithmetic of the others with every update masked.
#pragma once
#include "chain.hpp"

namespace mpdx {

struct IkArgs {
    const float* table;      // the chain table (device); header + QD joint records are staged
    const float* target;     // [n][12]  p*, then R* row-major
    const float* q_init;     // [n][R][QD] or null: Philox seeds
    float* q_out;            // [n][R][QD]
    float* err_out;          // [n][R][2]  |p - p*|, |e_R|
    int32_t* status;         // [n][R]     bit 0 converged, bits 8 ... iterations used
    int R;
    int frame;               // 1 ... QD
    float offset[3];
    float q_lo[8], q_hi[8];
    float rot_weight, pos_tol, rot_tol;
    float lam_init, lam_up, lam_down, lam_min, lam_max;
    int adaptive, max_iters;
    unsigned long long seed;
};

// what one evaluation of a configuration leaves: the residual e = [p - p*; w_r e_R] and the figures of the stop rule
struct IkEval { float e[6], perr, rerr, trace; };

// FK of frame f with chain_fk's recurrence and operation order (T_j = T_{j-1} [R_j | t_j] M_j(q_j), sinf / cosf), the tool point and the residual.
// JAC: O_j and z_j of the joints j <= f are kept (rows j >= f of O / Z are not written).  Rm / p: Rot_f and the tool point.
template <int QD, bool JAC>
__device__ __forceinline__ IkEval ik_eval(const float* __restrict__ stab, const IkArgs& a, const float (&tg)[12], const float (&q)[QD], float (&O)[QD][3],
                                          float (&Z)[QD][3], float (&p)[3]) {
    const int32_t* tabi = reinterpret_cast<const int32_t*>(stab);
    float R[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}, T[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < QD; ++k) {
        if (k < a.frame) {   // (wave-uniform)
            // the joint records are loop-invariant: hoisted out of the iteration loop they hold a hundred registers for its whole length and the 7- and
            // 8-joint kernels spill; the compiler barrier keeps each record's LDS reads next to their use
            asm volatile("" ::: "memory");
            const float* J = stab + kChainHdr + k * kChainJF;
            const bool prismatic = __builtin_amdgcn_readfirstlane(tabi[kChainHdr + k * kChainJF + 12]) != 0;
            const float qk = q[k];
            float A[3][3], Tn[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) A[r][c] = R[r][0] * J[c] + R[r][1] * J[3 + c] + R[r][2] * J[6 + c];
                Tn[r] = R[r][0] * J[9] + R[r][1] * J[10] + R[r][2] * J[11] + T[r];
            }
            float st = 0.f, ct = 1.f, dz = 0.f;
            if (prismatic) dz = qk;
            else { st = sinf(qk); ct = cosf(qk); }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                R[r][0] = A[r][0] * ct + A[r][1] * st;
                R[r][1] = A[r][1] * ct - A[r][0] * st;
                R[r][2] = A[r][2];
                T[r] = Tn[r] + dz * A[r][2];
                if constexpr (JAC) { O[k][r] = T[r]; Z[k][r] = R[r][2]; }
            }
        }
    }
    IkEval ev;
    float s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p[r] = T[r] + R[r][0] * a.offset[0] + R[r][1] * a.offset[1] + R[r][2] * a.offset[2];
        ev.e[r] = p[r] - tg[r];
        s2 += ev.e[r] * ev.e[r];
    }
    ev.perr = sqrtf(s2);
    ev.e[3] = ev.e[4] = ev.e[5] = 0.f; ev.rerr = 0.f; ev.trace = 3.f;
    if (a.rot_weight > 0.f) {   // (wave-uniform) e_R = 1/2 sum_i Rot_f[:, i] x R*[:, i]; trace(Rot_f^T R*)
        float er[3] = {0.f, 0.f, 0.f}, tr = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a0 = R[0][i], a1 = R[1][i], a2 = R[2][i], b0 = tg[3 + i], b1 = tg[6 + i], b2 = tg[9 + i];
            er[0] += a1 * b2 - a2 * b1; er[1] += a2 * b0 - a0 * b2; er[2] += a0 * b1 - a1 * b0;
            tr += a0 * b0 + a1 * b1 + a2 * b2;
        }
        float r2 = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) { er[r] *= 0.5f; r2 += er[r] * er[r]; ev.e[3 + r] = a.rot_weight * er[r]; }
        ev.rerr = sqrtf(r2); ev.trace = tr;
    }
    return ev;
}

template <int QD>
__global__ __launch_bounds__(64) void ik_solve_kernel(const IkArgs a) {
    constexpr int NT = kChainHdr + QD * kChainJF;
    __shared__ float stab[NT];
    const int lane = threadIdx.x;
    const int ti = blockIdx.y;
    const int r_ = blockIdx.x * 64 + lane;
    const bool valid = r_ < a.R;
    const int r = valid ? r_ : a.R - 1;   // (a masked lane of the last workgroup computes on the last restart's seed and stores nothing)
    for (int i = lane; i < NT; i += 64) stab[i] = a.table[i];
    float tg[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) tg[i] = a.target[(size_t)ti * 12 + i];
    const size_t slot = (size_t)ti * a.R + r;
    float q[QD];
    if (a.q_init) {
#pragma unroll
        for (int j = 0; j < QD; ++j) q[j] = fminf(fmaxf(a.q_init[slot * QD + j], a.q_lo[j]), a.q_hi[j]);   // (a seed inside the limits is left as it is)
    } else {
        float u0[4], u1[4] = {0.f, 0.f, 0.f, 0.f};
        philox_uniform4(a.seed, ((uint64_t)ti << 32) | (uint64_t)(2 * r), u0);
        if constexpr (QD > 4) philox_uniform4(a.seed, ((uint64_t)ti << 32) | (uint64_t)(2 * r + 1), u1);
#pragma unroll
        for (int j = 0; j < QD; ++j) {
            const float u = j < 4 ? u0[j & 3] : u1[j & 3];
            q[j] = fminf(fmaxf(fmaf(a.q_hi[j] - a.q_lo[j], u, a.q_lo[j]), a.q_lo[j]), a.q_hi[j]);   // (the clamp: u can round to 1 and the product past q_hi by an ulp)
        }
    }
    __syncthreads();

    const bool rot = a.rot_weight > 0.f;
    float lam = a.lam_init, perr = 0.f, rerr = 0.f;
    int it = 0, conv = 0;
    bool running = valid;
    for (;;) {
        float O[QD][3], Z[QD][3], p[3];
        const IkEval ev = ik_eval<QD, true>(stab, a, tg, q, O, Z, p);
        if (running) {
            perr = ev.perr; rerr = ev.rerr;
            conv = (ev.perr <= a.pos_tol && (!rot || (ev.rerr <= a.rot_tol && ev.trace > 1.f))) ? 1 : 0;
            if (conv || it >= a.max_iters) running = false;
        }
        if (!__any(running)) break;   // wave-uniform exit

        // the residual's Jacobian, one column per joint j <= f: [Jv; -w_r Jw] (e_R points from the current to the target orientation: d e_R / dq is
        // -Jw to first order, the geometric-Jacobian Gauss-Newton approximation); joints above the frame: zero columns
        float J[QD][6];
#pragma unroll
        for (int j = 0; j < QD; ++j) {
#pragma unroll
            for (int c = 0; c < 6; ++c) J[j][c] = 0.f;
            if (j < a.frame) {
                const bool prismatic = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t*>(stab)[kChainHdr + j * kChainJF + 12]) != 0;
                if (prismatic) { J[j][0] = Z[j][0]; J[j][1] = Z[j][1]; J[j][2] = Z[j][2]; }
                else {
                    const float d0 = p[0] - O[j][0], d1 = p[1] - O[j][1], d2 = p[2] - O[j][2];
                    J[j][0] = Z[j][1] * d2 - Z[j][2] * d1; J[j][1] = Z[j][2] * d0 - Z[j][0] * d2; J[j][2] = Z[j][0] * d1 - Z[j][1] * d0;
                    if (rot) { J[j][3] = -a.rot_weight * Z[j][0]; J[j][4] = -a.rot_weight * Z[j][1]; J[j][5] = -a.rot_weight * Z[j][2]; }
                }
            }
        }
        // (J^T J + lambda I) dq = -J^T e: Cholesky L L^T of the lower triangle in registers, two triangular solves
        float L[QD][QD], inv[QD], dq[QD];
#pragma unroll
        for (int i = 0; i < QD; ++i) {
            float g = 0.f;
#pragma unroll
            for (int c = 0; c < 6; ++c) g += J[i][c] * ev.e[c];
            dq[i] = -g;
#pragma unroll
            for (int k = 0; k <= i; ++k) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 6; ++c) s += J[i][c] * J[k][c];
                L[i][k] = k == i ? s + lam : s;
            }
        }
#pragma unroll
        for (int j = 0; j < QD; ++j) {
            float d = L[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
            L[j][j] = sqrtf(fmaxf(d, lam));   // (in exact arithmetic the pivot is >= lambda: the floor acts only where rounding has eaten it, and keeps dq finite)
            inv[j] = 1.0f / L[j][j];
#pragma unroll
            for (int i = j + 1; i < QD; ++i) {
                float s = L[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
                L[i][j] = s * inv[j];
            }
        }
#pragma unroll
        for (int j = 0; j < QD; ++j) {
            float s = dq[j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[j][k] * dq[k];
            dq[j] = s * inv[j];
        }
#pragma unroll
        for (int j = QD - 1; j >= 0; --j) {
            float s = dq[j];
#pragma unroll
            for (int k = j + 1; k < QD; ++k) s -= L[k][j] * dq[k];
            dq[j] = s * inv[j];
        }
        // the candidate, clamped into the limits, and its cost
        float qc[QD];
#pragma unroll
        for (int j = 0; j < QD; ++j) qc[j] = fminf(fmaxf(q[j] + dq[j], a.q_lo[j]), a.q_hi[j]);
        float Oc[QD][3], Zc[QD][3], pc[3];
        const IkEval evc = ik_eval<QD, false>(stab, a, tg, qc, Oc, Zc, pc);
        float F = 0.f, Fc = 0.f;
#pragma unroll
        for (int c = 0; c < 6; ++c) { F += ev.e[c] * ev.e[c]; Fc += evc.e[c] * evc.e[c]; }
        F *= 0.5f; Fc *= 0.5f;
        bool accept = true;
        if (a.adaptive) {
            accept = Fc < F;
            if (running) lam = accept ? fmaxf(lam * a.lam_down, a.lam_min) : fminf(lam * a.lam_up, a.lam_max);
        }
        if (running) {
            if (accept) {
#pragma unroll
                for (int j = 0; j < QD; ++j) q[j] = qc[j];
            }
            ++it;
        }
    }
    if (valid) {
#pragma unroll
        for (int j = 0; j < QD; ++j) a.q_out[slot * QD + j] = q[j];
        a.err_out[slot * 2] = perr; a.err_out[slot * 2 + 1] = rerr;
        a.status[slot] = (it << 8) | conv;
    }
}

// ---- k_ik.hip: every ik_solve_kernel instantiation
int launch_ik(const IkArgs& a, int n_joints, int n, hipStream_t st);

}  // namespace mpdx
