// k_guide.hip - the cost-guidance and trajectory-metrics kernels (guide.hpp) and their C-ABI entry points.
#include "host.hpp"
#include "guide.hpp"
#include "chain.hpp"   // the chain robot's block checks and the launchers of its kernels (instantiated in k_chain.hip)

namespace mpdx {

static long long* g_guide_trace = nullptr;  // dev tool (mpdx_guide_trace)

// The checks of a MPDX_ROBOT_CHAIN block, in the order: members of the block (nothing is dereferenced), then the table.  A table in host (or
// managed) memory is read where it lies; a device table is copied to the host ONCE per (pointer, size) and the verdict kept - launches inside
// the planning loop neither copy nor synchronise (the kernels clamp every index they take from the table).
const char* chain_params_check(const mpdx_guide_params& gp, ChainInfo* info) {
    if (!gp.chain) return "chain robot without a chain table (chain == NULL)";
    if (gp.n_chain_floats < chain_table_floats(1, 1, 0)) return "chain: n_chain_floats does not cover the table header, one joint and one sphere";
    if (gp.q_dim < 1 || gp.q_dim > MPDX_ROBOT_CHAIN_MAX_JOINTS) return "chain: q_dim outside 1 ... MPDX_ROBOT_CHAIN_MAX_JOINTS";
    if (gp.ws_dim != 3) return "chain: ws_dim must be 3 (a planar arm is a chain whose axes are all z, among 3-D primitives)";
    if (has_grid_field(gp)) return "chain: a MPDX_FIELD_GRID field is not supported with a chain robot (primitive, workspace and self fields)";
    if ((uintptr_t)gp.chain & 3) return "chain table must be 4-byte aligned";
    struct Seen { const float* p; int n; ChainInfo ci; };
    static std::mutex mu;
    static std::vector<Seen> seen;
    const int n = std::min(gp.n_chain_floats, chain_table_floats(MPDX_ROBOT_CHAIN_MAX_JOINTS, MPDX_ROBOT_CHAIN_MAX_SPHERES, MPDX_ROBOT_CHAIN_MAX_PAIRS));
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, gp.chain);
    if (e != hipSuccess) (void)hipGetLastError();   // (an ordinary host pointer, or no device at all: not an error of this call)
    const bool on_device = e == hipSuccess && at.type == hipMemoryTypeDevice;
    if (!on_device) return chain_table_problem(gp, gp.chain, info);
    {
        std::lock_guard<std::mutex> lock(mu);
        for (const Seen& s : seen)
            if (s.p == gp.chain && s.n == gp.n_chain_floats && s.ci.n_joints == gp.q_dim) {
                *info = s.ci;
                for (int f = 0; f < gp.n_fields && f < MPDX_MAX_FIELDS; ++f)
                    if (gp.fields[f].kind == MPDX_FIELD_SELF && s.ci.n_pairs == 0) return "chain: a MPDX_FIELD_SELF field needs n_pairs > 0 in the chain table";
                return nullptr;
            }
    }
    std::vector<float> host((size_t)n);
    if (hipMemcpy(host.data(), gp.chain, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return "chain: the chain table could not be read from the device";
    }
    if (const char* why = chain_table_problem(gp, host.data(), info)) return why;
    std::lock_guard<std::mutex> lock(mu);
    if (seen.size() >= 64) seen.clear();
    seen.push_back({gp.chain, gp.n_chain_floats, *info});
    return nullptr;
}

// The checks of the tool members (the tool-axis term, include/mpdx.h): members only, nothing is dereferenced.  A chain block has passed
// chain_params_check by now, so q_dim is the table's n_joints.
const char* tool_params_problem(const mpdx_guide_params& gp) {
    static thread_local char msg[200];
    if (gp.tool_frame == 0) return nullptr;
    if (gp.robot != MPDX_ROBOT_CHAIN) {
        snprintf(msg, sizeof(msg), "tool_frame %d: the tool-axis term needs robot == MPDX_ROBOT_CHAIN (robot %d; the Panda takes it as RobotChain.panda())", gp.tool_frame, gp.robot);
        return msg;
    }
    if (gp.tool_frame < 1 || gp.tool_frame > gp.q_dim) { snprintf(msg, sizeof(msg), "tool_frame %d outside 1 ... n_joints (%d)", gp.tool_frame, gp.q_dim); return msg; }
    const float* axes[2] = {gp.tool_axis, gp.tool_world};
    const char* names[2] = {"tool_axis", "tool_world"};
    for (int k = 0; k < 2; ++k) {
        float n2 = 0.f;
        for (int j = 0; j < 3; ++j) {
            if (!(fabsf(axes[k][j]) < 3.0e38f)) { snprintf(msg, sizeof(msg), "%s is not finite", names[k]); return msg; }
            n2 += axes[k][j] * axes[k][j];
        }
        if (!(fabsf(sqrtf(n2) - 1.f) <= 1e-4f)) { snprintf(msg, sizeof(msg), "%s is not a unit vector to 1e-4 (norm %g)", names[k], (double)sqrtf(n2)); return msg; }
    }
    if (!(gp.tool_cos_min >= -1.f && gp.tool_cos_min <= 1.f)) { snprintf(msg, sizeof(msg), "tool_cos_min %g outside [-1, 1]", (double)gp.tool_cos_min); return msg; }
    if (!(fabsf(gp.tool_weight) < 3.0e38f)) return "tool_weight is not finite";
    return nullptr;
}

const char* chain_params_problem(const mpdx_guide_params& gp) {
    if (gp.robot != MPDX_ROBOT_CHAIN) return nullptr;
    ChainInfo ci;
    return chain_params_check(gp, &ci);
}

// per-context max|x| (the range test of LimitsNormalizer.unnormalize) for the API path
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, uint32_t* out, size_t per_ctx, int n_ctx) {
    const int ctx = blockIdx.y;
    const float* p = x + (size_t)ctx * per_ctx;
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_ctx; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(p[i]));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out + ctx, __float_as_uint(m));
}

int guide_block_problem(const mpdx_guide_params* gp, int D, ChainInfo* chain_info, int H) {
    if (D != 2 * gp->q_dim || D > 16) return fail(MPDX_E_INVALID, "state dim %d != 2*q_dim (%d)", D, gp->q_dim);
    if (gp->n_fields < 0 || gp->n_fields > MPDX_MAX_FIELDS) return fail(MPDX_E_INVALID, "n_fields %d", gp->n_fields);
    if (gp->n_prim_floats > 0 && !gp->prims) return fail(MPDX_E_INVALID, "primitive table missing");
    if (!chain_info) {   // (the baseline planners: built-in robots, one scene, no grid - refusals of their own)
        if (gp->tool_frame != 0) return fail(MPDX_E_INVALID, "tool_frame %d: the baseline planners do not take the tool-axis term (guide, mpdx_plan and mpdx_traj_tool_metrics only)", gp->tool_frame);
        for (int f = 0; f < MPDX_MAX_FIELDS; ++f)   // a planner would silently plan among the obstacles' positions at time 0
            if (field_track_len(*gp, f) != 0) return fail(MPDX_E_INVALID, "fields[%d].track_len = %d: the baseline planners do not take moving obstacles (guide, metrics and mpdx_plan only)", f, field_track_len(*gp, f));
        return 0;
    }
    if (const char* why = motion_params_problem(*gp, H)) return fail(MPDX_E_INVALID, "%s", why);   // (members only, and before a chain table is read: a track refuses a chain)
    memset(chain_info, 0, sizeof(*chain_info));
    if (gp->robot == MPDX_ROBOT_CHAIN)   // (a chain robot's own refusals first: it takes no grid field at all)
        if (const char* why = chain_params_check(*gp, chain_info)) return fail(MPDX_E_INVALID, "%s", why);
    if (const char* why = tool_params_problem(*gp)) return fail(MPDX_E_INVALID, "%s", why);
    if (const char* why = grid_params_problem(*gp)) return fail(MPDX_E_INVALID, "%s", why);
    if (const char* why = scene_params_problem(*gp)) return fail(MPDX_E_INVALID, "%s", why);
    return 0;
}

// What a workgroup of a guide launch stages (the LDS carve is sized by it), and whether the launch takes the Panda's dense variant (no FK table, 128
// VGPRs: two workgroups per CU): at large batch, or as MPDX_GUIDE_DENSE=0/1 forces it off / on - and only where its layout fits 80 KB.
static mpdx_guide_params guide_params_staged(const mpdx_guide_params& gp, const ChainInfo& chain_info) {
    mpdx_guide_params staged = gp;
    staged.n_prim_floats = staged_prim_floats(gp);
    if (gp.robot == MPDX_ROBOT_CHAIN) staged.n_chain_floats = chain_info.n_floats;
    return staged;
}
static bool guide_takes_dense(const mpdx_guide_params& staged, int B, int H, int D) {
    const int dense_env = sw::guide_dense();
    return staged.robot == MPDX_ROBOT_PANDA && (dense_env >= 0 ? dense_env != 0 : B >= 512) && guide_lds_bytes(staged, H, D, true) <= 80 * 1024;
}

int launch_guide(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hs, const float* hg,
                        const uint32_t* amax_in, uint32_t* amax_out, int n_per_ctx, int B, int H, int D, hipStream_t st,
                        const float* noise, float noise_scale, float noise_extra, float* chain, float guide_scale, const NoiseRng* rng) {
    if (!gp || !x || !amax_in) return fail(MPDX_E_INVALID, "null argument");
    if (H > 128 || H < 2) return fail(MPDX_E_INVALID, "guide kernel: one support point per lane of one or two waves: H=%d unsupported (max 128)", H);
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;
    if (gp->interpolate && (gp->n_interp < H || gp->n_interp > 8 * H)) return fail(MPDX_E_INVALID, "n_interp %d unsupported", gp->n_interp);
    if (gp->robot == MPDX_ROBOT_PANDA && (((uintptr_t)x & 15) || ((size_t)H * D) % 4))
        return fail(MPDX_E_INVALID, "Panda guide: x must be 16-byte aligned with H * D a multiple of 4 (the trajectory is staged with 16-byte loads)");
    GuideArgs a;
    a.gp = dev_params_staged(*gp); a.x = x; a.grad_out = grad_out; a.hs = hs; a.hg = hg; a.amax_in = amax_in; a.amax_out = amax_out;
    a.B = B; a.H = H; a.D = D; a.n_per_ctx = n_per_ctx > 0 ? n_per_ctx : B;
    a.noise = noise; a.noise_scale = noise_scale; a.noise_extra = noise_extra; a.chain = chain;
    a.guide_scale = guide_scale;
    memset(&a.rng, 0, sizeof(a.rng));
    if (rng) a.rng = *rng;
    if (gp->clip_grad && gp->clip_rule != 0 && gp->clip_rule != 1) return fail(MPDX_E_INVALID, "clip_rule %d (0 = 'norm', 1 = 'value')", gp->clip_rule);
    a.trace = g_guide_trace;
    // a grid field selects the HAS_GRID instantiations (grid_field.hpp): the primitive-only ones are the code they were before grids existed
    const bool grid = has_grid_field(*gp);
    memset(&a.grid, 0, sizeof(a.grid));
    if (grid) a.grid = dev_grids_of(*gp);
    // several scenes select the MULTI_SCENE instantiations (scene_table.hpp), for the same reason; a workgroup stages one scene block + the shared tail
    const bool multi = has_scenes(*gp);
    a.scene = dev_scenes_of(*gp);
    const mpdx_guide_params staged = guide_params_staged(*gp, chain_info);
    const bool dense = guide_takes_dense(staged, B, H, D);
    const size_t lds = guide_lds_bytes(staged, H, D, dense);
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "guide needs %zu B of LDS (n_interp %d too large)", lds, gp->n_interp);
    if (gp->robot == MPDX_ROBOT_CHAIN) return launch_chain_guide(a, dev_tool_of(*gp), gp->chain, chain_info, multi, lds, B, st);   // (q_dim == n_joints, ws_dim == 3: checked above)
    // a track selects the MOVING instantiations (motion.hpp), for the same reason; their arguments carry the track descriptor behind the block
    const bool moving = has_motion(*gp);
    GuideArgsMoving am;   // (filled for a MOVING launch only: the static launches pass `a`)
    if (moving) {
        static_cast<GuideArgs&>(am) = a;
        am.motion = dev_motion_of(*gp);
    }
    int rc = 0;
    const bool known = with_builtin_robot(*gp, [&](auto qd, auto, auto robot) {
        if constexpr (decltype(robot)::value == MPDX_ROBOT_PANDA)
            rc = with_bools([&](auto dense_c, auto grid_c) {
                return with_scene_mode([&](auto multi_c, auto moving_c) {
                    auto kern = guide_step_panda_kernel<decltype(dense_c)::value, decltype(grid_c)::value, decltype(multi_c)::value, decltype(moving_c)::value>;
                    if (int r = raise_lds_limit((const void*)kern)) return r;
                    if constexpr (decltype(moving_c)::value) hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, am);
                    else hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, a);
                    return 0;
                }, multi, moving);
            }, dense, grid);
        else   // (the point mass has no dense variant and stays under the default LDS limit's refusal: no raise_lds_limit)
            with_bools([&](auto grid_c) {
                return with_scene_mode([&](auto multi_c, auto moving_c) {
                    constexpr int QD = decltype(qd)::value;
                    auto kern = guide_step_kernel<QD, QD, MPDX_ROBOT_POINTMASS, 8, decltype(grid_c)::value, decltype(multi_c)::value, decltype(moving_c)::value>;
                    if constexpr (decltype(moving_c)::value) hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, am);
                    else hipLaunchKernelGGL(kern, dim3(B), dim3(512), lds, st, a);
                    return 0;
                }, multi, moving);
            }, grid);
    });
    if (!known) return fail(MPDX_E_INVALID, "unsupported robot %d / q_dim %d / ws_dim %d", gp->robot, gp->q_dim, gp->ws_dim);
    return rc;
}

}  // namespace mpdx

using namespace mpdx;

extern "C" {

int mpdx_guide_step(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hard_start, const float* hard_goal,
                    const uint32_t* absmax_in, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, void* stream) {
    if (int rc = launch_guide(gp, x, grad_out, hard_start, hard_goal, absmax_in, absmax_out, n_per_ctx, B, H, D, (hipStream_t)stream)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_guide_step_scaled(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hard_start, const float* hard_goal,
                           const uint32_t* absmax_in, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, float guide_scale, void* stream) {
    if (int rc = launch_guide(gp, x, grad_out, hard_start, hard_goal, absmax_in, absmax_out, n_per_ctx, B, H, D, (hipStream_t)stream, nullptr, 0.f,
                              0.f, nullptr, guide_scale))
        return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_traj_metrics(const mpdx_guide_params* gp, const float* x_unnormalised, float* out4, int n_check, int B, int H, int D, void* stream) {
    return mpdx_traj_metrics_mask(gp, x_unnormalised, out4, nullptr, n_check, B, H, D, stream);
}

int mpdx_traj_metrics_mask(const mpdx_guide_params* gp, const float* x_unnormalised, float* out4, uint8_t* mask, int n_check, int B, int H, int D,
                           void* stream) {
    if (!gp || !x_unnormalised || !out4 || B <= 0) return fail(MPDX_E_INVALID, "bad argument");
    if (H > 128 || H < 2) return fail(MPDX_E_INVALID, "H=%d unsupported (max 128)", H);
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;
    if (n_check < 2) n_check = H;
    hipStream_t st = (hipStream_t)stream;
    const bool grid = has_grid_field(*gp), multi = has_scenes(*gp), moving = has_motion(*gp);
    const dev_motion mo = dev_motion_of(*gp);
    const dev_guide_params g = dev_params_staged(*gp);   // (n_prim_floats = what a workgroup stages: the table, or one scene block + the shared tail)
    const dev_scenes sc = dev_scenes_of(*gp);
    if (gp->robot == MPDX_ROBOT_CHAIN) {
        if (int rc = launch_chain_metrics(g, x_unnormalised, out4, mask, n_check, B, H, sc, gp->chain, chain_info, multi, st)) return rc;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const size_t lds = metrics_lds_layout(false, H, D, g.n_prim_floats).total * sizeof(float);
    dev_grids gr;
    memset(&gr, 0, sizeof(gr));
    if (grid) gr = dev_grids_of(*gp);
    const bool known = with_builtin_robot(*gp, [&](auto qd, auto dim, auto robot) {
        with_bools([&](auto grid_c) {
            return with_scene_mode([&](auto multi_c, auto moving_c) {
                if constexpr (decltype(moving_c)::value)
                    hipLaunchKernelGGL((traj_metrics_kernel<decltype(qd)::value, decltype(dim)::value, decltype(robot)::value, decltype(grid_c)::value, false, true, dev_motion>),
                                       dim3(B), dim3(64), lds, st, g, x_unnormalised, out4, B, H, n_check, mask, gr, sc, mo);
                else
                    hipLaunchKernelGGL((traj_metrics_kernel<decltype(qd)::value, decltype(dim)::value, decltype(robot)::value, decltype(grid_c)::value, decltype(multi_c)::value>),
                                       dim3(B), dim3(64), lds, st, g, x_unnormalised, out4, B, H, n_check, mask, gr, sc);
                return 0;
            }, multi, moving);
        }, grid);
    });
    if (!known) return fail(MPDX_E_INVALID, "unsupported robot %d / q_dim %d / ws_dim %d", gp->robot, gp->q_dim, gp->ws_dim);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_traj_tool_metrics(const mpdx_guide_params* gp, const float* x_unnormalised, float* out2, uint8_t* mask, int n_check, int B, int H, int D,
                           void* stream) {
    if (!gp || !x_unnormalised || !out2 || B <= 0) return fail(MPDX_E_INVALID, "bad argument");
    if (H > 128 || H < 2) return fail(MPDX_E_INVALID, "H=%d unsupported (max 128)", H);
    if (gp->tool_frame == 0) return fail(MPDX_E_INVALID, "tool_frame 0: mpdx_traj_tool_metrics needs the tool members of the block");
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;   // (a built-in robot with tool_frame != 0 is refused there)
    if (n_check < 2) n_check = H;
    if (int rc = launch_chain_tool_metrics(dev_tool_of(*gp), x_unnormalised, out2, mask, n_check, B, H, gp->chain, chain_info, (hipStream_t)stream)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_guide_time(const mpdx_guide_params* gp, float* x, float* grad_out, const uint32_t* absmax_in, int n_per_ctx, int B, int H, int D,
                    int reps, void* stream, float* ms_avg) {
    if (!gp || !x || !grad_out || !absmax_in || !ms_avg || reps < 1) return fail(MPDX_E_INVALID, "bad argument");
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;   // (before the events: nothing is created for a refused block)
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    int rc = 0;
    for (int i = 0; i < 3 && !rc; ++i) rc = launch_guide(gp, x, grad_out, nullptr, nullptr, absmax_in, nullptr, n_per_ctx, B, H, D, st);
    HIP_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < reps && !rc; ++i) rc = launch_guide(gp, x, grad_out, nullptr, nullptr, absmax_in, nullptr, n_per_ctx, B, H, D, st);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    if (!rc) HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_avg = ms / (float)reps;
    return rc;
}

/* dev tool: one guide launch with s_memtime stamps (16 slots per wave, 8 waves -> 128 values) of workgroup 0 */
int mpdx_guide_trace(const mpdx_guide_params* gp, float* x, const uint32_t* absmax_in, int B, int H, int D, void* stream, long long* stamps64) {
    if (int rc = dev_hooks_missing(__func__)) return rc;
    if (!stamps64) return fail(MPDX_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    long long* dev = nullptr;
    HIP_TRY(hipMalloc(&dev, 128 * sizeof(long long)));
    HIP_TRY(hipMemsetAsync(dev, 0, 128 * sizeof(long long), st));
    static float* scratch = nullptr;
    static size_t scratch_n = 0;
    const size_t need = (size_t)B * H * D;
    if (scratch_n < need) { if (scratch) (void)hipFree(scratch); HIP_TRY(hipMalloc(&scratch, need * sizeof(float))); scratch_n = need; }
    g_guide_trace = dev;
    int rc = launch_guide(gp, x, scratch, nullptr, nullptr, absmax_in, nullptr, B, B, H, D, st);
    g_guide_trace = nullptr;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(stamps64, dev, 128 * sizeof(long long), hipMemcpyDeviceToHost));
    (void)hipFree(dev);
    return rc;
}

int mpdx_guide_variant(const mpdx_guide_params* gp, int B, int H, int D) {
    if (!gp) return fail(MPDX_E_INVALID, "null argument");
    ChainInfo chain_info;
    if (int rc = guide_block_problem(gp, D, &chain_info, H)) return rc;
    return guide_takes_dense(guide_params_staged(*gp, chain_info), B, H, D) ? 1 : 0;
}

int mpdx_absmax(const float* x, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, void* stream) {
    if (!x || !absmax_out || B <= 0) return fail(MPDX_E_INVALID, "bad argument");
    const int npc = n_per_ctx > 0 ? n_per_ctx : B;
    if (B % npc) return fail(MPDX_E_INVALID, "B=%d is not a multiple of n_per_ctx=%d", B, npc);
    const size_t per = (size_t)npc * H * D;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((per + 255) / 256, 64), B / npc), dim3(256), 0, (hipStream_t)stream, x,
                       absmax_out, per, B / npc);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
