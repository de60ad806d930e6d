// k_ik.hip - the inverse-kinematics kernel of a table-driven serial chain (ik.hpp): every instantiation (1 ... 8 joints) and its C-ABI entry point.
#include "host.hpp"
#include "ik.hpp"

namespace mpdx {

template <int QD = 1>
static int launch_ik_qd(const IkArgs& a, int n_joints, int n, hipStream_t st) {
    if constexpr (QD > MPDX_ROBOT_CHAIN_MAX_JOINTS) return fail(MPDX_E_INVALID, "ik: n_joints %d", n_joints);
    else {
        if (n_joints != QD) return launch_ik_qd<QD + 1>(a, n_joints, n, st);
        hipLaunchKernelGGL(ik_solve_kernel<QD>, dim3((a.R + 63) / 64, n), dim3(64), 0, st, a);
        return 0;
    }
}

int launch_ik(const IkArgs& a, int n_joints, int n, hipStream_t st) { return launch_ik_qd(a, n_joints, n, st); }

}  // namespace mpdx

extern "C" {

int mpdx_ik_solve(const mpdx_guide_params* gp, const mpdx_ik_opts* o, const float* target, const float* q_init, float* q_out, float* err_out,
                  int32_t* status, int n, int restarts, void* stream) {
    using namespace mpdx;
    if (!gp) return fail(MPDX_E_INVALID, "ik: gp is null");
    if (!o) return fail(MPDX_E_INVALID, "ik: opts is null");
    if (!target) return fail(MPDX_E_INVALID, "ik: target is null");
    if (!q_out) return fail(MPDX_E_INVALID, "ik: q_out is null");
    if (!err_out) return fail(MPDX_E_INVALID, "ik: err_out is null");
    if (!status) return fail(MPDX_E_INVALID, "ik: status is null");
    if (n < 1 || n > 65535) return fail(MPDX_E_INVALID, "ik: n %d outside 1 ... 65535", n);
    if (restarts < 1 || restarts > 4096) return fail(MPDX_E_INVALID, "ik: restarts %d outside 1 ... 4096", restarts);
    if (gp->robot != MPDX_ROBOT_CHAIN)
        return fail(MPDX_E_INVALID, "ik: gp->robot %d is a built-in robot: the solver runs on a chain table (MPDX_ROBOT_CHAIN; the Panda as a chain serves)", gp->robot);
    // of the block only robot, q_dim, chain and n_chain_floats count: the checks of a chain block run on a copy without fields
    mpdx_guide_params g = *gp;
    g.ws_dim = 3; g.n_fields = 0;
    ChainInfo ci;
    if (const char* why = chain_params_check(g, &ci)) return fail(MPDX_E_INVALID, "ik: %s", why);
    if (o->frame < 1 || o->frame > ci.n_joints)
        return fail(MPDX_E_INVALID, "ik: opts->frame %d outside 1 ... n_joints (%d); frame 0 is the fixed base", o->frame, ci.n_joints);
    for (int k = 0; k < 3; ++k)
        if (!finite_f(o->offset[k])) return fail(MPDX_E_INVALID, "ik: opts->offset is not finite");
    for (int j = 0; j < ci.n_joints; ++j) {
        if (!finite_f(o->q_lo[j]) || !finite_f(o->q_hi[j])) return fail(MPDX_E_INVALID, "ik: opts->q_lo / q_hi of joint %d are not finite", j);
        if (o->q_lo[j] > o->q_hi[j]) return fail(MPDX_E_INVALID, "ik: opts->q_lo > q_hi at joint %d (%g > %g)", j, (double)o->q_lo[j], (double)o->q_hi[j]);
    }
    if (!(o->rot_weight >= 0.f) || !finite_f(o->rot_weight)) return fail(MPDX_E_INVALID, "ik: opts->rot_weight %g must be finite and >= 0 (0: position only)", (double)o->rot_weight);
    if (!(o->pos_tol > 0.f) || !finite_f(o->pos_tol)) return fail(MPDX_E_INVALID, "ik: opts->pos_tol %g must be positive and finite", (double)o->pos_tol);
    if (!(o->rot_tol > 0.f) || !finite_f(o->rot_tol)) return fail(MPDX_E_INVALID, "ik: opts->rot_tol %g must be positive and finite", (double)o->rot_tol);
    if (!(o->lambda_init > 0.f) || !finite_f(o->lambda_init)) return fail(MPDX_E_INVALID, "ik: opts->lambda_init %g must be positive and finite", (double)o->lambda_init);
    if (o->adaptive && (!(o->lambda_up >= 1.f) || !finite_f(o->lambda_up) || !(o->lambda_down > 0.f) || !(o->lambda_down <= 1.f) || !(o->lambda_min > 0.f) ||
                        !(o->lambda_max >= o->lambda_min) || !finite_f(o->lambda_max)))
        return fail(MPDX_E_INVALID, "ik: adaptive needs opts->lambda_up >= 1, 0 < lambda_down <= 1, 0 < lambda_min <= lambda_max (got %g, %g, %g, %g)", (double)o->lambda_up,
                    (double)o->lambda_down, (double)o->lambda_min, (double)o->lambda_max);
    if (o->max_iters < 0 || o->max_iters > (1 << 22)) return fail(MPDX_E_INVALID, "ik: opts->max_iters %d outside 0 ... 2^22", o->max_iters);
    IkArgs a;
    memset(&a, 0, sizeof(a));
    a.table = gp->chain; a.target = target; a.q_init = q_init; a.q_out = q_out; a.err_out = err_out; a.status = status;
    a.R = restarts; a.frame = o->frame;
    for (int k = 0; k < 3; ++k) a.offset[k] = o->offset[k];
    for (int j = 0; j < 8; ++j) { a.q_lo[j] = o->q_lo[j]; a.q_hi[j] = o->q_hi[j]; }
    a.rot_weight = o->rot_weight; a.pos_tol = o->pos_tol; a.rot_tol = o->rot_tol;
    a.lam_init = o->lambda_init; a.lam_up = o->lambda_up; a.lam_down = o->lambda_down; a.lam_min = o->lambda_min; a.lam_max = o->lambda_max;
    a.adaptive = o->adaptive ? 1 : 0; a.max_iters = o->max_iters; a.seed = o->seed;
    if (int rc = launch_ik(a, ci.n_joints, n, (hipStream_t)stream)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
