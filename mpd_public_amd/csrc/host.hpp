// host.hpp - the host-side model (layer plan, parameter table, fused segments) and the launcher interface between the translation
// units of libmpdx.so.  The library is built from one host TU (mpdx.hip: model building, tile choice, the launch units of a pass and the ONE walk
// over them, mpdx_plan's launch schedule and loop, the C ABI, the small streaming kernels; it alone includes fused_build.hpp - the fused-segment builder and build_units - and
// unet_measure.hpp - the timing / trace entry points and the launch-unit queries) and one TU per kernel family - k_conv.hip (conv_block.hpp), k_ws.hip (conv_ws.hpp), k_fused.hip /
// k_fused_train.hip (fused_level.hpp), k_guide.hip (guide.hpp), k_chain.hip (chain.hpp), k_costs.hip (costs.hpp), k_ik.hip (ik.hpp), k_grid.hip (the grid producers: edt.hpp, mesh_sdf.hpp, grid_field.hpp's bake), k_attn.hip (attn.hpp), k_inner_run.hip (inner_run.hpp), k_train.hip (train.hpp + train_host.hpp), k_planner.hip
// (planner.hpp + planner_host.hpp) - so that an edit to one kernel family recompiles that family only (mpd_public_amd/build.py
// compiles the TUs in parallel and keeps the objects).  A kernel template is instantiated in exactly ONE TU, behind a plain function
// declared here; no device code crosses a TU (no -fgpu-rdc).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mpdx.h"
#include "conv_block.hpp"
#include "conv_ws.hpp"
#include "fused_level.hpp"
#include "switches.hpp"
#include "train_types.hpp"

namespace mpdx {

// ------------------------------------------------------------------------------------------------ error plumbing (mpdx.hip)
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return ::mpdx::fail((int)e_, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
int raise_lds_limit(const void* kern);   // hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel)
int dev_hooks_missing(const char* fn);   // 0 in a development build (-DMPDX_DEV_HOOKS); else the MPDX_E_STATE error of a trace / ablation entry point
inline bool finite_f(float v) { return fabsf(v) < 3.0e38f; }   // an entry point's float argument is usable (false for NaN)

// final_conv[1] (Conv1d(32 -> D, k=1), temporal_unet.py:113-116) fused with the DDPM posterior step
// (diffusion_model_base.py:121-155, sample_functions.py:31-62) and hard conditioning (sample_functions.py:5-8).
// One thread per (trajectory, horizon index); the arithmetic is rounded op by op exactly as the reference's
// separate elementwise ATen kernels are (no fma contraction), so given the same eps the update is bit-identical.
struct FinalArgs {
    const float* h;      // [B][H][C] output of final_conv[0]
    const float* w;      // [D][C]
    const float* bias;   // [D]
    const float* x_in;   // [B][H][D]
    const float* noise;  // [B][H][D] or null
    const float* hs;     // hard start [B][D] or null
    const float* hg;     // hard goal  [B][D] or null
    float* out;          // eps (mode 0) or x_next (mode 1/2)
    float* chain;        // optional second destination
    uint32_t* absmax;    // optional per-context max|out| (bit pattern)
    int B, H, D, C;
    int Hc;              // rows per trajectory of h (the container; 0: H)
    int mode;            // 0: eps only; 1: full step; 2: posterior mean only (guide insertion point); 3: DDIM update
    int n_per_ctx;
    mpdx_step_coefs k;
    NoiseRng rng;        // rng.on: the step's noise is drawn in place (noise pointer ignored)
};

// ------------------------------------------------------------------------------------------------ host-side model
enum ParamKind { PK_VEC = 0, PK_CONV = 1, PK_CONVT = 2 };

struct Param {
    std::string name;
    int32_t shape[3] = {0, 0, 0};
    int32_t ndim = 0;
    size_t n = 0;       // floats in the reference tensor
    size_t off = 0;     // offset (floats) in the packed buffer
    size_t foff = 0;    // offset (floats) in the flat reference-layout parameter vector (training, train_host.hpp)
    size_t pn = 0;      // floats in the packed buffer
    int kind = PK_VEC;
    int cout = 0, cin = 0, ksz = 0, cin_pad = 0, nslot = 0;
    bool done = false;
};

enum { SRC_X = -1, SRC_NONE = -2 };

struct Layer {
    int mode = CONV_S1, ks = 5, epi = EPI_GN_MISH;
    int c1 = 0, c2 = 0, cout = 0, L_in = 0, L_out = 0, gs = 0;
    int Lv_out = 0;           // valid rows of the output when the horizon runs in a power-of-two container (0: all L_out rows; ConvArgs::Lv_out)
    int src1 = SRC_NONE, src2 = SRC_NONE, dst = 0, res = SRC_NONE;  // workspace slots
    int w = -1, b = -1, gamma = -1, beta = -1;                       // param indices
    int tb_off = -1;                                                 // offset in a time-table row
    int cin_pad = 0, rs = 0;
    // a Residual(PreNorm(LinearAttention)) block of a self_attention network (attn.hpp), in place on slot `dst` (== src1): w = to_qkv.weight,
    // w2 / b2 = to_out.weight / bias, gamma / beta = the LayerNorm's g / b; cout channels on L_out positions; no convolution fields apply
    bool attn = false;
    int w2 = -1, b2 = -1;
    // convolutions of a self_attention network: the tile width of a layer WITHOUT the 8-wave K split is pinned (choose_tile), because there the
    // split of K over the waves - the summation order - follows the width, and the width follows the batch; such a network runs every layer on this
    // path at every batch and promises results that do not depend on the batch
    bool pin_nt = false;
    std::string name;
};

}  // namespace mpdx

struct mpdx_unet {
    mpdx_unet_cfg cfg;
    std::vector<mpdx::Param> params;
    std::unordered_map<std::string, int> pidx;
    std::vector<mpdx::Layer> layers;
    size_t packed_floats = 0;
    size_t slot_floats = 0;   // per-trajectory floats of one activation slot
    int n_slots = 0;
    int tt_row = 0;           // floats per time-table row
    std::vector<int> tt_w, tt_b, tt_cout, tt_off;  // cond_mlp param indices per block
    int final_slot = 0;       // slot holding final_conv[0]'s output
    int n_done = 0;
    // horizons that are not powers of two: the network runs in a container of Hc = next power of two rows per trajectory (ConvArgs::Lv_out);
    // the network input is copied into workspace slot `xpad_slot` ([B][Hc][D], zero rows behind the H real ones) at the head of a pass
    int Hc = 0, xpad_slot = -1;
    bool masked() const { return Hc != cfg.n_support_points; }
    int plan_join = 1;        // mpdx_unet_set_plan_join: mpdx_plan may run a step's up program and the next step's down program as one launch
    // mpdx_unet_set_inner_run / _set_inner_run_parts: the runs mpdx_plan may take (inner_run.hpp) - kRunSeven: the seven 256 -> 256 layers of the
    // innermost level, kRunTail: the tail of up level 0 - as one persistent launch each
    enum RunPart { kRunSeven = 1, kRunTail = 2 };
    int inner_run = kRunSeven | kRunTail;
    int inner_run_width = 0;   // mpdx_unet_set_inner_run_width: positions per cluster of both runs - 0 automatic (by batch), 16, 32
    int plan_joined = 0, inner_runs = 0;   // joined / seven-layer run launches of the last mpdx_plan call (mpdx_unet_plan_joined, mpdx_unet_inner_runs)
    int inner_run_layers = 0;              // layers that ran inside run launches of either kind in the last mpdx_plan call (mpdx_unet_inner_run_layers)
    // The run's device state, made at the first mpdx_plan call that may take the run (a handle is created without a device).  mpdx.hip's
    // inner_run_create / _begin / _free and mpdx_unet_set_status alone write it: every counter of a launch's clusters holds `base` when the launch starts.
    struct InnerRunState {
        int capacity = -1;            // compute units of this device (-1: not asked yet; 0: no run on this handle)
        // workgroups per compute unit each run kernel's occupancy query answered, per width ([0]: 32, [1]: 16; 0: the query failed).  A launch
        // is admitted where its grid is resident at once: one workgroup per compute unit at width 32, up to two at width 16.
        int seven_wgs[2] = {0, 0}, tail_wgs[2] = {0, 0};
        long long budget = 0;         // s_memtime ticks of 4 ms
        unsigned* counters = nullptr; // device: one arrival counter per cluster (not reset between launches: base advances by 8 x layers per launch)
        // One set of counters per width ([0]: 32, [1]: 16; both inside `counters`): the launches of one width cover the same clusters and advance
        // them together, whatever the other run of the plan takes.
        struct Counters {
            unsigned* p = nullptr;
            unsigned base = 0;
            int live = 1 << 30;       // clusters whose counters hold base (all of them while every counter is zero)
            bool rezero = false;      // the counters hold a give-up's poison: zero them (and base) before the next launch
        } ctr[2];
        unsigned *status = nullptr, *status_dev = nullptr;   // host-mapped pinned sticky word a workgroup that gives up sets; the device's address of it
        unsigned status_host = 0;     // stands in for *status until the device state exists
        unsigned status_word() const { return status ? __atomic_load_n(status, __ATOMIC_RELAXED) : status_host; }
    } run;
    // mpdx_unet_set_level_split: mpdx_plan may run a joined launch in its paired form (fused_join_split_kernel: the 128-channel down level on two compute
    // units per trajectory) - 0 never, 1 wherever it is admitted, -1 automatic (by batch)
    int level_split = -1;
    int plan_split = 0;       // paired launches of the last mpdx_plan call (mpdx_unet_plan_split)
    // The paired launch's device state, made at the first mpdx_plan call that may take it (mpdx.hip level_split_create / _begin / _free)
    struct LevelSplitState {
        int capacity = -1;            // compute units (-1: not asked yet; 0: no paired launch on this handle)
        int wgs = 0;                  // workgroups per compute unit the kernel's occupancy query answered
        float* xch = nullptr;         // exchange area [kSplitMaxB][kSplitTrajFloats]
        unsigned* counters = nullptr; // one 128-byte line per trajectory, not reset between launches: base advances by kSplitAdvance per launch
        unsigned base = 0;
        int live = 1 << 30;           // trajectories whose counters hold base (all of them while every counter is zero)
        bool rezero = false;          // a give-up's poison: zero the counters (and base) before the next launch
    } split;
    // launch units: fused whole-trajectory segments (fused_level.hpp) or single layers
    struct CopyJob { size_t src, dst; int n0, ss0, ds0, n1, ss1, ds1, n_inner; };   // strided copy inside `packed` (float units)
    struct Fused {
        int first = 0, count = 0;       // layer range [first, first+count)
        bool has_final = false;         // final_conv[1] + DDPM step folded in
        int in1 = 0, in2 = 0;           // input slots (SRC_X / SRC_NONE allowed)
        int in3 = mpdx::SRC_NONE;       // slot of a skip tensor concatenated INSIDE the program (FusedArgs::gsrc3)
        int gout_slot[3] = {-1, -1, -1};
        size_t lds_bytes = 0;
        mpdx::FusedArgs tmpl;
        int program = -1;               // index of the matching static program (fused_program_kernel), -1: generic op-list kernel
        std::vector<CopyJob> jobs;      // assemble the stream-ordered weight copies + the contiguous parameter block
        std::vector<int> op_layer;      // conv op k computes layer op_layer[k] (a folded residual conv has no op of its own)
        int in3_consumer = -1;          // layer whose second source is the in3 skip tensor
    };
    std::vector<Fused> fused;
    void* jobs_dev = nullptr;           // device copy of every segment's CopyJobs (restream_all_kernel)
    int n_jobs = 0;
    const float* streams_for = nullptr; // `packed` buffer the fused streams were last assembled in
    int pack_version = 0, streams_version = -1;
    // one launch of a pass: it covers layers [layer, layer + count) - a program its segment fused[fused], a pair blocks[0] + the block's residual 1x1
    // conv, the inner run and the tail run (mpdx_plan's schedule only, never in current_units) their kInnerRunLayers / kTailRunLayers
    enum UnitKind { kProgram, kLayer, kPair, kInnerRun, kTailRun };
    struct Unit { UnitKind kind; int fused; int layer; int count; int width = 0; };   // width: of a kInnerRun / kTailRun unit
    std::vector<int> owner;                  // layer -> fused segment (-1: per-layer launch)
    // training (train_host.hpp)
    struct TrainLayer {
        int src1_l = -2, src2_l = -2, res_l = -2;   // layer that produced the tensor (-1: the network input, -2: none)
        bool need_dgrad = false;
        size_t dgrad_woff = 0;                      // offset of the dgrad weights in packedT
        mpdx::Layer dg;                             // the stride-1 convolution that computes the input gradient
    };
    bool train_ready = false;
    size_t flat_floats = 0, packedT_floats = 0;
    std::vector<TrainLayer> tl;
    std::vector<mpdx::PackDesc> pack_descs_host;
    void* pack_descs_dev = nullptr;
    void* pack_chunks_dev = nullptr;   // PackChunk table of pack_train_kernel
    size_t n_pack_chunks = 0;
};

namespace mpdx {

// ---- mpdx.hip
int pick_row_stride(int cin_pad, int mode, int L_in, int L_out, int LP);
void choose_tile(const Layer& l, int B, int& MT, int& NT);
bool layer_ksplit(const Layer& l);
int check_ready(const mpdx_unet* u);
unsigned fused_mask(int B);
bool fused_save_variant(const mpdx_unet::Fused& f);
int ensure_fused_streams(mpdx_unet* u, const float* packed, hipStream_t st);
int claim_fused_stream_jobs(mpdx_unet* u, const float* packed, const void** jobs, int* n);   // training: the copies ride on the pass's first launch
int launch_final_step(const FinalArgs& fa, hipStream_t st);   // final_step_kernel (fa.B/H/D/C set)
// ---- k_conv.hip: every conv_block_kernel / conv_pair_kernel instantiation
int launch_conv_layer(const Layer& l, ConvArgs& a, int B, hipStream_t st);
bool pair_tile(const Layer& l1, const Layer& l2, int B, int& MT, int& NT);   // (mpdx.hip) do blocks[0] + the block's residual 1x1 conv run as one launch, on which tile?
int launch_conv_pair(int MT, int NT, const ConvArgs& a1, const ConvArgs& a2, const Layer& l1, const Layer& l2, hipStream_t st);   // 1 launched, 0 does not fit, -1 error
// ---- k_inner_run.hip: the persistent run of the innermost level's 256 -> 256 layers (inner_run.hpp)
template <int N> struct RunArgs;
bool inner_run_width_ok(int width);                // 32 or 16 positions per cluster (inner_run.hpp kRunWide / kRunNarrow)
int inner_run_clusters(int B, int width);          // clusters of width / 8 trajectories for batch B
int inner_run_grid(int B, int width);              // workgroups of a launch (the placement's surplus ones included); the same for both runs
void inner_run_slot(int block, int* cluster, int* tile);   // the (cluster, channel tile) the kernel gives a block (a cluster >= inner_run_clusters: it leaves)
int inner_run_workgroups_per_cu(int width);        // one occupancy query per run kernel and width; 0: failed
int tail_run_workgroups_per_cu(int width);
int launch_inner_run(const RunArgs<7>& ra, int B, int width, hipStream_t st);   // InnerRunArgs
int launch_tail_run(const RunArgs<4>& ra, int B, int width, hipStream_t st);    // TailRunArgs
// ---- k_attn.hip: the linear self-attention block (attn.hpp); a.x and the five parameter pointers set by the caller
struct AttnArgs;
const char* attn_unsupported(int C, int L);   // null, or why attn_kernel cannot run a level of C channels on L positions
int launch_attention(const Layer& l, AttnArgs& a, int B, hipStream_t st);
// ---- k_ws.hip: the weight-stationary persistent kernels
int launch_weight_stationary(int variant, const Layer& l, ConvArgs& a, const ConvArgs& a2, int B, hipStream_t st);
// ---- k_fused.hip (planning programs) / k_fused_train.hip (the variants that keep activations for the backward pass)
int launch_fused_args(const mpdx_unet::Fused& f, const FusedArgs& a, int B, hipStream_t st, bool save = false);
int launch_fused_train(const mpdx_unet::Fused& f, const FusedArgs& a, int B, hipStream_t st);
int launch_fused_join(const FusedJoinArgs& ja, int B, hipStream_t st);   // fused_join_kernel<FusedSeqUpAB, FusedSeqDown3> (programs 3 and 5)
size_t fused_join_lds_bytes();
int launch_fused_join_split(const FusedJoinArgs& ja, const FusedSplitArgs& sa, int B, hipStream_t st);   // fused_join_split_kernel, split_grid(B) workgroups
int fused_join_split_workgroups_per_cu();   // one occupancy query; 0: failed
// ---- k_guide.hip
struct NoiseRng;
int launch_guide(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hs, const float* hg, const uint32_t* amax_in,
                 uint32_t* amax_out, int n_per_ctx, int B, int H, int D, hipStream_t st, const float* noise = nullptr, float noise_scale = 0.f,
                 float noise_extra = 0.f, float* chain = nullptr, float guide_scale = 1.0f, const NoiseRng* rng = nullptr);
const char* chain_params_problem(const mpdx_guide_params& gp);   // nullptr, or why a MPDX_ROBOT_CHAIN block is refused (any other robot: nullptr)
const char* tool_params_problem(const mpdx_guide_params& gp);    // nullptr, or why the tool members are refused (tool_frame == 0: nullptr); chain.hpp
struct ChainInfo;
// The checks every launcher applies to a guide parameter block: D == 2 q_dim, n_fields, the primitive table; with chain_info (the guide, its timer
// and the metrics; filled for a chain robot, else zeroed) also the track (H: the support points of the launch; motion.hpp), chain, grid and scene members;
// without it (the baseline planners) any track is refused.  0, or fail(MPDX_E_INVALID, ...).
int guide_block_problem(const mpdx_guide_params* gp, int D, ChainInfo* chain_info, int H);

}  // namespace mpdx
