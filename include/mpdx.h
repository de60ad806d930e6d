/*
 * mpdx.h - C ABI of libmpdx.so: the MI355X (gfx950) guided reverse-diffusion trajectory sampler.
 *
 * The reference (jacarvalho/mpd-public) has NO native / FFI interface for this path: it is three Python callable
 * protocols.  Each entry point below states the reference Python interface it replaces
 * (file:line under /root/reference) - this is what a maintainer's ctypes stub binds.
 *
 * Conventions
 *   - every function returns int: 0 = ok, >0 = hipError_t, <0 = MPDX_E_* ; never throws across the ABI;
 *     mpdx_last_error() returns a thread-local human-readable message for the last non-zero return.
 *   - the CALLER owns every device buffer (PyTorch caching allocator in practice) and passes raw device pointers;
 *     the library never allocates caller-visible device memory and never synchronises: it only enqueues work on
 *     the hipStream_t it is given (void* here so that the header needs no HIP include).
 *   - tensors are contiguous fp32 row-major.  Trajectories are [B, H, D] exactly as the reference's x.
 *   - one handle per model; a handle is host-side metadata only (layer table, offsets); not thread-safe per handle.
 *   - the MPDX_* environment switches the library reads are listed in INTEGRATION.md section F (csrc/switches.hpp); none is needed.
 */
#ifndef MPDX_H
#define MPDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPDX_E_INVALID   (-1) /* bad argument / unsupported configuration */
#define MPDX_E_NOTFOUND  (-2) /* unknown parameter name */
#define MPDX_E_STATE     (-3) /* call order violated (e.g. forward before all parameters were packed) */
#define MPDX_E_DEVICE    (-4) /* a kernel gave up a bounded wait on the device; sticky on the handle (mpdx_unet_status) */

#define MPDX_MAX_LEVELS 8

typedef struct mpdx_unet mpdx_unet; /* opaque */

/* TemporalUnet.__init__ arguments that shape the network (mpd/models/diffusion_models/temporal_unet.py:22-35), for
 * conditioning_type=None (the only one the reference scripts build); self_attention is either value.
 *
 * self_attention = 1 puts a Residual(PreNorm(dim, LinearAttention(dim))) behind the second residual block of every down level, between
 * the two middle blocks and behind the second residual block of every up level (temporal_unet.py:82,93,104,146,153,162), five more
 * state-dict tensors each (<p>.fn.fn.to_qkv.weight [384,C,1], <p>.fn.fn.to_out.weight [C,128,1], <p>.fn.fn.to_out.bias [C],
 * <p>.fn.norm.g / .b [1,C,1]; <p> = downs.<i>.2, mid_attn, ups.<j>.2).  Per trajectory, x [C, L], all in fp32, one launch per block:
 *   xn  = (x - mean) / sqrt(var + 1e-5) * g + b      mean / biased variance over the C channels of each position (layers.py:194-204)
 *   qkv = W_qkv xn                                   no bias; q, k, v = 128 rows each = 4 heads x 32 channels (LinearAttention's own
 *                                                    defaults, layers.py:208; TemporalUnet passes only dim); q *= 32^-0.5 (layers.py:217-219)
 *   k   = softmax(k) over the L positions of each row, max-subtracted; q is not soft-maxed (layers.py:221)
 *   context[d][e] = sum_n k[d][n] v[e][n],  out[e][n] = sum_d context[d][e] q[d][n]     per head, 32 x 32 (layers.py:222-224)
 *   result = W_out out + b_out + x                   (layers.py:226, :180)
 * In a zero-padded container (H = 24, 40, 48, 96) the softmax and the context sum run over the valid positions and the pad rows stay zero.
 * Such a network runs every layer as its own launch (no whole-trajectory programs).  It is inference and evaluation only: the
 * mpdx_train_* entry points refuse its handle (the size functions return 0) - the training pass has no backward for these blocks. */
typedef struct mpdx_unet_cfg {
    int32_t state_dim;                  /* D */
    int32_t n_support_points;           /* H: 64 in every shipped configuration; 16 ... 128 with H % 2^(n_levels-1) == 0 (powers of two run as they are, 24 / 40 / 48 / 96 ... in the next power-of-two container, zero rows kept zero) */
    int32_t unet_input_dim;             /* 32 */
    int32_t n_levels;                   /* len(dim_mults) */
    int32_t dim_mults[MPDX_MAX_LEVELS]; /* (1,2,4,8) or (1,2,4): UNET_DIM_MULTS, temporal_unet.py:14-17 - the shipped ones.  Admitted: 2 ... 8 entries >= 1 with
                                           dim_mults[0] == 1, unet_input_dim a multiple of 16, every Conv1dBlock's GroupNorm region (group of 4 ... 32 channels x
                                           positions of its level) a power of two in 64 ... 2048 - e.g. (1,2), (1,8), (1,1,2), (1,2,2), (1,2,4,4), (1,2,8,8),
                                           (1,2,4,8,8), (1,1,2,2,4,8) on H = 128 (tests/shapes_ref.py holds the family the suite runs).  Refused with the layer
                                           named: a region outside that range ((1,2) on H = 16, (1,3), (1,16), width 16 ...), and dim_mults[i] == 2 * dim_mults[i+1]
                                           ((1,2,1), (1,4,2)): ups.<j>.0 would carry an identity residual over its whole concatenated input */
    int32_t time_emb_dim;               /* 32 */
    int32_t self_attention;             /* 0 / 1: TemporalUnet(self_attention=...), see above (appended: positional initialisers of the members above leave it 0) */
} mpdx_unet_cfg;

const char* mpdx_last_error(void);
int mpdx_version(void);

/* ---- model construction: replaces TemporalUnet(**unet_configs) + load_state_dict (inference.py:132-148) ---- */
int    mpdx_unet_create(const mpdx_unet_cfg* cfg, mpdx_unet** out);
void   mpdx_unet_destroy(mpdx_unet* u);
/* Handle option of mpdx_plan (default on).  The reference's reverse loop (p_sample_loop, diffusion_model_base.py:157-182) feeds the x_{t-1} of one
 * ddpm_sample_fn call (sample_functions.py:17-62) straight into the next call's model(x, t): on an unguided iteration that has a successor, mpdx_plan
 * runs the step's last program (up levels + final_conv + DDPM update) and the next step's first program (down levels) as ONE launch, one workgroup
 * per trajectory, where the standard four-level network on H = 64 runs and the batch is at most one workgroup per compute unit.  The results
 * are bit-identical with the option off; every other entry point runs the separate kernels.  mpdx_unet_plan_joined: how many joined launches the last
 * mpdx_plan call on this handle issued (0: the option is off or the network / batch does not admit it). */
int    mpdx_unet_set_plan_join(mpdx_unet* u, int on);
int    mpdx_unet_plan_joined(const mpdx_unet* u);
/* Paired form of the joined launch, a handle option of mpdx_plan.  The 128-channel level of the down part (downs.2: five ops of 8 channel tiles on one
 * position tile) runs on TWO compute units per trajectory: a helper workgroup on the same XCD takes channel tiles 4 - 7, the k-loops halve, and after
 * each of the level's first four ops the two workgroups trade their 4 KB halves of the output through a handle-owned exchange area (write-through
 * stores, one counter per trajectory, bounded polls - the runs' recipe, status word and 4 ms budget: see mpdx_unet_status below).  A wave still owns a
 * whole tile for the whole K and a GroupNorm group is one tile, so the results are bit-identical with the option off.  Admitted where a joined launch
 * is and both workgroups of every trajectory are resident at once (2 x 8 ceil(B / 8) <= compute units: B <= 128 on 256 CUs).
 * mpdx_unet_set_level_split(u, on): 0 never, 1 wherever admitted, negative automatic by batch (the default).  mpdx_unet_plan_split: paired launches of
 * the last mpdx_plan call (0 or mpdx_unet_plan_joined).
 * mpdx_level_split_block, without a device (tests): the workgroups of a paired launch for batch B (the return value; negative: an error), the trajectory
 * (-1: a surplus workgroup, it leaves at once) and the role (0 primary, 1 helper) of workgroup `block`.  Null outputs are skipped. */
int    mpdx_unet_set_level_split(mpdx_unet* u, int on);
int    mpdx_unet_plan_split(const mpdx_unet* u);
int    mpdx_level_split_block(int B, int block, int32_t* trajectory, int32_t* role);
/* Inner-level run, a handle option, default on.  mpdx_plan runs the seven consecutive 256 -> 256 Conv1dBlocks of the innermost level
 * (downs.3.0.blocks.1, downs.3.1, mid_block1, mid_block2) as ONE persistent launch where the standard four-level network on H = 64 runs without
 * self-attention and every workgroup of that launch is resident at once (8 x ceil(B / 4) workgroups, one per compute unit: B <= 128 on 256 CUs);
 * guided plans included.  The 8 workgroups of a position tile hand their output tiles to each other inside the launch; the arithmetic is the
 * per-layer kernels', the results are bit-identical with the option off, and every other entry point runs the separate kernels.
 * mpdx_unet_inner_runs: run launches of the last mpdx_plan call on this handle (0: option off, or network / batch do not admit it).
 * The device state of the run (arrival counters, status word) belongs to the handle: one mpdx_plan of a handle at a time.
 *
 * Every wait inside the run is bounded (4 ms of shader clock; a layer takes under 10 us).  A workgroup whose wait runs out sets a sticky status
 * word on the handle, makes the workgroups of its position tile leave as well, and writes NaN into its tile of the run's output, so the plan's
 * trajectories are NaN.  mpdx_unet_status returns MPDX_E_DEVICE while the word is set (0 otherwise) and mpdx_plan refuses to start; both read
 * host memory and never synchronise.  The window: the word is written while the plan's launches EXECUTE, so mpdx_plan's own return value only
 * covers launches that have already run when it returns; ask mpdx_unet_status after synchronising the stream to cover the whole plan.
 * mpdx_unet_set_status(u, 0) clears the word (the counters are re-zeroed before the next run); a non-zero word marks the handle failed as
 * a give-up would (bit 0 set, bits 8.. the layer of the run that waited).
 *
 * The tail run: under the same conditions the tail of up level 0 - the three 128 -> 128 Conv1dBlocks ups.0.0.blocks.1, ups.0.1.blocks.0,
 * ups.0.1.blocks.1 and Upsample1d(128) - is a second persistent launch of the same kind (same counters, status word, bounds and bit-identical results).
 * mpdx_unet_set_inner_run(u, 1) selects every run that is eligible, 0 none.  mpdx_unet_set_inner_run_parts selects them separately: bit 0 the seven
 * layers, bit 1 the tail (A/B runs and tests; other bits: MPDX_E_INVALID).  mpdx_unet_inner_runs counts the seven-layer launches only;
 * mpdx_unet_inner_run_layers: how many layers ran inside run launches of either kind in the last mpdx_plan call (11 per pass with both selected).
 *
 * The width of the runs: a position tile is 4 whole trajectories (32 positions, one workgroup per compute unit) or 2 (16 positions, 8 x ceil(B / 2)
 * workgroups, up to two per compute unit; B <= 128 on 256 CUs either way).  mpdx_unet_set_inner_run_width(u, w): w = 0 automatic by batch (the
 * default), 16 or 32 for both runs; anything else MPDX_E_INVALID.  It takes effect at the next mpdx_plan; the results are the same bits at every
 * width, and the two counts above keep their values. */
int    mpdx_unet_set_inner_run(mpdx_unet* u, int on);
int    mpdx_unet_set_inner_run_parts(mpdx_unet* u, int parts);
int    mpdx_unet_set_inner_run_width(mpdx_unet* u, int width);
/* The launch geometry of a run, without a device (tests): the workgroups of a launch for batch B at `width` (the return value; negative: an error),
 * the cluster (-1: a surplus workgroup of the placement, it leaves at once) and the channel tile 0..7 of workgroup `block`, and the counter lines a
 * handle keeps for that width on a device of `cus` compute units.  Null outputs are skipped. */
int    mpdx_inner_run_block(int B, int width, int cus, int block, int32_t* cluster, int32_t* tile, int32_t* counter_lines);
int    mpdx_unet_inner_runs(const mpdx_unet* u);
int    mpdx_unet_inner_run_layers(const mpdx_unet* u);
int    mpdx_unet_status(const mpdx_unet* u);
int    mpdx_unet_set_status(mpdx_unet* u, unsigned word);
/* number of state-dict tensors the model expects; their names/shapes (identical to the reference's keys) */
int    mpdx_unet_num_params(const mpdx_unet* u);
int    mpdx_unet_param_info(const mpdx_unet* u, int idx, const char** name, int32_t shape[3], int32_t* ndim);
/* sizes (in floats) of the caller-allocated device buffers */
size_t mpdx_unet_packed_floats(const mpdx_unet* u);             /* repacked weights (MFMA fragment order)       */
size_t mpdx_unet_timetab_floats(const mpdx_unet* u, int T);     /* per-timestep conditioning table [T, sum C_out] */
size_t mpdx_unet_workspace_floats(const mpdx_unet* u, int B);   /* activations for a batch of B trajectories    */
/* repack one state-dict tensor (device pointer, reference layout) into `packed` */
int    mpdx_unet_pack_param(mpdx_unet* u, const char* name, const float* src_dev, size_t n_floats,
                            float* packed_dev, void* stream);
/* TimeEncoder + every block's cond_mlp depend only on the integer t (layers.py:229-255,336-340): tabulate them.
 * freqs16 = the 16 sinusoid frequencies exp(-k*ln(1e4)/15) computed by the host exactly as layers.py:249-251. */
int    mpdx_unet_build_timetab(mpdx_unet* u, const float* packed_dev, const float* freqs16_dev, int T,
                               float* timetab_dev, void* stream);

/* ---- eps-model call: replaces model(x, t, context=None) (diffusion_model_base.py:147; temporal_unet.py:118) ----
 * x, eps: [B,H,D]; t: the (batch-constant) integer timestep, 0 <= t < T. */
int mpdx_unet_forward(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T,
                      const float* x, int t, float* eps, int B, float* ws, void* stream);

/* ---- one reverse step: replaces ddpm_sample_fn's arithmetic (sample_functions.py:17-62) together with
 * p_mean_variance / predict_start_from_noise / q_posterior (diffusion_model_base.py:121-155) and
 * apply_hard_conditioning (sample_functions.py:5-8).  Scalars are the t-th entries of the registered buffers. */
typedef struct mpdx_step_coefs {
    float sqrt_recip_alphas_cumprod;    /* diffusion_model_base.py:90  */
    float sqrt_recipm1_alphas_cumprod;  /* :91 */
    float posterior_mean_coef1;         /* :100 */
    float posterior_mean_coef2;         /* :102 */
    float noise_scale;                  /* exp(0.5*posterior_log_variance_clipped[t]) ; 0 when t == 0 */
    float noise_std_extra;              /* noise_std_extra_schedule_fn(t) (0.5 at inference.py:243), 1 if None */
    int32_t predict_epsilon;            /* :121-132 */
    int32_t clip_denoised;              /* :149-150 */
    float ddim_k1;                      /* ddim_sample (:184-259): sqrt(alphas_cumprod[t_next]), 1 on the last pair */
    float ddim_k2;                      /* sqrt(1 - alphas_cumprod[t_next] - sigma^2) with eta = 0, 0 on the last pair */
    float guide_scale;                  /* factor on every guide increment of this step: 1, or model_var = exp(posterior_log_variance_clipped[t])
                                         * when scale_grad_by_std (sample_functions.py:77-78) */
} mpdx_step_coefs;

/* x_io[B,H,D] is updated in place to  hard_cond( mean + noise_scale*noise*noise_std_extra ).
 * noise may be NULL (treated as 0).  hard_start/hard_goal: [B,D] values written at horizon index 0 / H-1
 * (NULL = no hard conditioning).  mean_only == 1: the posterior mean (before noise, before hard conditioning) is
 * written instead - the point where the reference inserts the guide (sample_functions.py:39-48).
 * mean_only == 2: the DDIM update of ddim_sample (diffusion_model_base.py:216-237, eta = 0):
 *   x <- hard_cond( ddim_k1 * x_start + ddim_k2 * pred_noise ), x_start NOT clamped (as the reference).
 * chain_out (optional): a second [B,H,D] destination that receives the same values (chain.append, :175-176).
 * absmax_out (optional, uint32 per context): atomicMax of the bit pattern of max|x| over each context's
 * n_per_ctx trajectories - the whole-tensor range test of LimitsNormalizer.unnormalize (normalization.py:160). */
int mpdx_ddpm_step(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T,
                   float* x_io, const float* noise, const float* hard_start, const float* hard_goal,
                   const mpdx_step_coefs* coefs, int t, int mean_only, float* chain_out,
                   uint32_t* absmax_out, int n_per_ctx, int B, float* ws, void* stream);

/* finish a guided step: x = hard_cond(x + noise_scale*noise*noise_std_extra), optional chain copy */
int mpdx_add_noise(float* x_io, const float* noise, const float* hard_start, const float* hard_goal,
                   float noise_scale, float noise_std_extra, float* chain_out, int B, int H, int D, void* stream);

/* apply_hard_conditioning (sample_functions.py:5-8) for ARBITRARY horizon indices:  x[:, horizon_idx[k], :] = values[k]  ([B,D] device tables) for
 * k < n <= 16, in order (python semantics: negative indices count from the end, a later entry wins on a repeated index); chain_out (optional) receives
 * the same writes.  horizon_idx / values are HOST arrays.  The step kernels fold indices 0 and H-1 into their epilogue (hard_start / hard_goal above);
 * this is the step-by-step loop's path for every other index (the fused mpdx_plan takes 0 and H-1 only). */
int mpdx_hard_conds(float* x_io, float* chain_out, int n, const int32_t* horizon_idx, const float* const* values, int B, int H, int D, void* stream);

/* ---- forward loss (what the reference's validation loop evaluates under no_grad; the pass WITH its gradient is mpdx_train_loss_backward below).
 * q_sample (diffusion_model_base.py:320-330) followed by apply_hard_conditioning (:335): per-trajectory timesteps t_dev[B]
 * (int64, clamped to [0,T)), schedule buffers on the device. */
int mpdx_q_sample(const float* x_start, const float* noise, const long long* t_dev, const float* sqrt_alphas_cumprod_dev,
                  const float* sqrt_one_minus_alphas_cumprod_dev, const float* hard_start, const float* hard_goal, float* out, int B, int H,
                  int D, int T, void* stream);
/* WeightedL2 (l1 = 0) / WeightedL1 (l1 = 1) of helpers.py:71-99 applied to apply_hard_conditioning(pred) vs targ
 * (diffusion_model_base.py:343-350): out1[0] = mean over B*H*D of the (optionally weights_hd[H*D]-weighted) error. */
int mpdx_weighted_loss(const float* pred, const float* targ, const float* weights_hd, const float* hard_start, const float* hard_goal,
                       int l1, float* out1, int B, int H, int D, void* stream);

/* ---- training step: replaces  loss = model.loss(x, context, hard_conds); loss.backward();
 * clip_grad_norm_; optimizer.step(); EMA.update_model_average   of mpd/trainer/trainer.py:186-283 with
 * GaussianDiffusionModel.p_losses (diffusion_model_base.py:331-352) and WeightedL1/L2 (helpers.py:71-99).
 * Parameters, gradients, Adam moments and the EMA copy are FLAT fp32 vectors in reference (state-dict) layout: parameter idx
 * (mpdx_unet_param_info order) lives at [off, off + n) with (off, n) from mpdx_train_param_offset, gaps are zero.  A host
 * framework can alias its parameter tensors onto the vector (mpd_public_amd/trainer.py does, so torch optimisers keep working). */
size_t mpdx_train_flat_floats(mpdx_unet* u);
size_t mpdx_train_dgrad_pack_floats(mpdx_unet* u);              /* transposed / tap-flipped packs for the input-gradient convolutions */
size_t mpdx_train_workspace_floats(mpdx_unet* u, int B);     /* every activation of a batch of B + gradient buffers */
int    mpdx_train_param_offset(mpdx_unet* u, int idx, size_t* off, size_t* n);
/* flat parameters -> forward pack (what mpdx_unet_pack_param builds, all parameters, one launch) and, if packedT != NULL,
 * the dgrad pack.  Call after every optimiser step. */
int    mpdx_train_pack(mpdx_unet* u, const float* flat, float* packed, float* packedT, void* stream);
/* one p_losses evaluation and its gradient wrt every parameter:
 *   x_start, noise [B,H,D]; t_dev [B] int64 timesteps; sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod [T] device tables;
 *   freqs16 the SinusoidalPosEmb frequencies (as mpdx_unet_build_timetab); hard_start / hard_goal [B,D] or NULL;
 *   weights_hd [H,D] loss weights or NULL; l1: 1 = WeightedL1, 0 = WeightedL2; loss_scale multiplies the gradient;
 *   loss_out: one device float <- the loss; grads_flat <- d(loss_scale * loss)/d(parameters), every parameter entry written. */
int    mpdx_train_loss_backward(mpdx_unet* u, const float* flat, const float* packed, const float* packedT, float* grads_flat,
                                const float* x_start, const float* noise, const long long* t_dev, const float* sqrt_alphas_cumprod_dev,
                                const float* sqrt_one_minus_alphas_cumprod_dev, const float* freqs16, const float* hard_start,
                                const float* hard_goal, const float* weights_hd, int T, int B, int predict_epsilon, int l1, float loss_scale,
                                float* loss_out, float* ws, void* stream);
/* torch.nn.utils.clip_grad_norm_(max_norm) if max_norm > 0, then torch.optim.Adam.step() (no weight decay, no amsgrad);
 * step counts from 1; scratch: >= 1032 floats (scratch[0] <- the gradient norm before clipping, scratch[1] <- the clip factor).
 * step < 0: the count lives on the device - the int at scratch + 4 holds the number of steps taken so far and this call advances it (the form a
 * training step captured into a hipGraph needs: kernel arguments are frozen at capture, trainer.TrainStep.step); with step < 0, lr < 0 takes the
 * learning rate from the float at scratch + 5 as well (an LR schedule then neither re-captures nor re-keys anything) */
int    mpdx_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                      float eps, int step, float max_norm, float* scratch, void* stream);
/* EMA.update_model_average (trainer.py:67-85): ema = beta * ema + (1 - beta) * params */
/* draw mode of mpdx_train_loss_backward (replaces `t = torch.randint(...)`, `noise = torch.randn_like(x)` of diffusion_model_base.py:356 / :337 when an
 * iteration is replayed as a hipGraph): with a non-null step_counter_dev - the device int mpdx_adam_step(step < 0) advances - the following loss passes
 * treat t_dev and noise as OUTPUTS drawn on the device (Philox4x32-10 keyed by seed, stream position step * B + sample); NULL disarms */
int    mpdx_train_draw(mpdx_unet* u, unsigned long long seed, const int* step_counter_dev);
int    mpdx_ema_update(float* ema, const float* params, size_t n, float beta, void* stream);

/* standard-normal generator for the production path (Philox4x32-10 + Box-Muller); replaces torch.randn /
 * torch.randn_like (diffusion_model_base.py:165, sample_functions.py:51).  Parity runs inject noise instead. */
int mpdx_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);

/* ---- cost guidance: replaces guide(x) = GuideManagerTrajectoriesWithVelocity.forward (guides.py:173-211) and one
 * iteration of guide_gradient_steps (sample_functions.py:74-81).  The cost terms are the ones inference.py:188-225
 * builds: one CostCollision per collision field of the task + CostGPTrajectory, weights as at :204,213.
 * Their arithmetic is un-vendored in the reference (empty submodules): restated, see oracle/costs.py. */
#define MPDX_MAX_FIELDS 4
#define MPDX_FIELD_OBJECTS   0 /* sdf to sphere/box primitives (task.df_collision_objects / extra objects) */
#define MPDX_FIELD_WORKSPACE 1 /* workspace-boundary planes */
#define MPDX_FIELD_SELF      2 /* robot self collision (Panda) */
#define MPDX_FIELD_GRID      3 /* precomputed signed-distance grid in global memory (guide and metrics kernels only; see below) */
#define MPDX_ROBOT_POINTMASS 0
#define MPDX_ROBOT_PANDA     1
#define MPDX_ROBOT_CHAIN     2 /* a serial kinematic chain given at run time as a table (mpdx_guide_params.chain, layout below); guide, metrics, mpdx_plan */

typedef struct mpdx_field {
    int32_t kind;                       /* MPDX_FIELD_* */
    float   weight;                     /* weight_grad_cost_collision (inference.py:55) */
    int32_t sphere_off, n_spheres;      /* float offset into prims, 4 floats each: cx,cy,cz,r (cz unused in 2-D); with several scenes: offset into the
                                         * staged image of a scene and the table's CAPACITY (mpdx_guide_params.n_scenes) */
    int32_t box_off, n_boxes;           /* 6 floats each: cx,cy,cz,hx,hy,hz */
    float   ws_min[3], ws_max[3];       /* MPDX_FIELD_WORKSPACE */
    /* --- MPDX_FIELD_GRID: a sampled signed-distance field (torch_robotics' GridMapSDF; un-vendored, restated: PARITY UNPINNED).
     * Planes live in mpdx_guide_params.grids (global memory, NOT in prims: every kernel copies prims into LDS):
     *   sdf plane       [nz][ny][nx] fp32, x fastest
     *   gradient plane  [nz][ny][nx][4] fp32 (gx, gy, gz, 0): one 16-byte load per node (grids 16-byte aligned, grid_grad_off % 4 == 0)
     * Lookup of a point p (all in fp32; inv = 1.0f / cell, taken ONCE on the host):
     *   u_j = (p_j - origin_j) * inv        (one rounded subtraction, one rounded product)
     *   c_j = min(max(u_j, 0), n_j - 1)     (the point is clamped into the grid box)
     *   MPDX_GRID_LINEAR : i_j = min((int)floor(c_j), n_j - 2), w_j = c_j - i_j; sdf = bi-/trilinear interpolant of the 4 / 8 nodes around the cell,
     *                      a + w (b - a) along x, then y, then z; gradient = the analytic derivative of that interpolant (what autograd gives on the
     *                      same formula: along j the interpolated node difference times inv); an axis on which the point was clamped
     *                      (c_j != u_j) contributes ZERO gradient.  Needs no gradient plane.
     *   MPDX_GRID_NEAREST: GridMapSDF AS RECALLED - node i_j = rint(c_j) (half to even, as torch.round / rintf); sdf = the node's value, gradient =
     *                      the node's STORED gradient (first-order surrogate), the edge node's for a clamped point.
     * The guide applies the hinge relu(margin - sdf) to it exactly as to an OBJECTS field. */
    /* --- MPDX_FIELD_OBJECTS: moving obstacles, time-indexed translation tracks (an extension: the reference's collision fields are static).  Both
     * members zero: the field does not move - the block behaves exactly as before the members existed (they lie where an OBJECTS field never
     * carried anything: the words a GRID field uses for its plane offsets; the caller zeroes the block as for every appended member).
     * An MPDX_FIELD_OBJECTS field may carry a track: track_len = H rows of 4 floats (ox, oy, oz, 0) at prims + track_off, behind the primitive
     * tables (the kernels stage it into LDS with them; n_prim_floats covers it).  Row h is the rigid translation of ALL the field's primitives at
     * the time of support point h (h * dt), relative to the positions in the primitive table.  In 2-D oz is ignored.
     * On point i of a trajectory - the guide's n_interp interpolated points, the metrics' n_check points, the supports themselves with
     * interpolation off - the kernels form the interpolation pair (i0, i1, l0, l1) of q_i = l0 * x[i0] + l1 * x[i1]; the field's offset there is
     *     o_i = l0 * track[i0] + l1 * track[i1]        (the same pair, the same arithmetic, fp32 throughout)
     * and every link point p of that trajectory point is tested as p' = p - o_i: from there on the field's arithmetic is unchanged (hinge,
     * arg-min primitive, gradient, all on p').  The force on the link point is the one computed at p' (a translation has an identity Jacobian; for
     * the Panda the moment of the force is taken about the link point p itself).  No velocity of the obstacle enters the cost.
     * A NaN or infinite track entry cannot fault: no index is formed from p'.  What the field then reports is NOT defined: against a sphere every
     * comparison with NaN is false (no hit, no force), but the box distance goes through fmaxf, which drops a NaN operand - a box whose p' is NaN on
     * every axis reads as deep inside (a hit, an active hinge), and one that is NaN on some axes acts as a slab along the others.  Keep tracks finite
     * (the Python side refuses a non-finite track; the C ABI does not read the table and cannot).
     * Checked on the host before any launch, on members only (MPDX_E_INVALID, message naming the member): track_len neither 0 nor H of the launch;
     * a track_len != 0 on a MPDX_FIELD_WORKSPACE or MPDX_FIELD_SELF field; track_off negative, not a multiple of 4, or the track not ending inside
     * n_prim_floats; a track overlapping a primitive table of any field or another track; n_scenes > 1; robot == MPDX_ROBOT_CHAIN.  Tracks next to a
     * MPDX_FIELD_GRID field are allowed (a grid itself does not move: its two words are its plane offsets).  Fields at and beyond n_fields are not
     * looked at.
     * Entry points that take tracks: mpdx_guide_step, mpdx_guide_step_scaled, mpdx_guide_time, mpdx_guide_variant, mpdx_traj_metrics,
     * mpdx_traj_metrics_mask, mpdx_plan; mpdx_gpmp_step, mpdx_rrt_connect, mpdx_rrt_paths and mpdx_sdf_grid_bake refuse any OBJECTS field with
     * track_len != 0 (the baseline planners would silently plan among the obstacles' positions at time 0). */
    /* The two words below are read by the field's kind: a MPDX_FIELD_GRID field has no primitives that could move and a MPDX_FIELD_OBJECTS field
     * no planes, so the track members of an OBJECTS field (moving obstacles, below) share their storage - mpdx_field and mpdx_guide_params keep
     * their size and every member its offset.  Two consequences.  (1) These words used to be ignored for every kind but MPDX_FIELD_GRID: a caller that
     * wrote something into them on an OBJECTS, WORKSPACE or SELF field (grid_grad_off = -1 on every field, say) now states a track, and the host
     * checks refuse the block (a track_len that is not H, or a track on a WORKSPACE / SELF field) rather than ignore it - zero them, as every appended
     * member of the block asks.  (2) Anonymous unions need C11 (or C++); a C99 caller compiles the header with its compiler's extension
     * (gcc and clang accept them in every mode). */
    union { int32_t grid_sdf_off;       /* MPDX_FIELD_GRID: float offset of the sdf plane in grids */
            int32_t track_len; };       /* MPDX_FIELD_OBJECTS: 0: the field does not move; otherwise it must equal H of the launch */
    union { int32_t grid_grad_off;      /* MPDX_FIELD_GRID: float offset of the gradient plane in grids, or -1: none (LINEAR only) */
            int32_t track_off; };       /* MPDX_FIELD_OBJECTS: float offset of the field's track in prims: track_len rows of 4 floats, offset a multiple of 4 */
    int32_t n[3];                       /* nodes along x, y, z (>= 2 along a used axis; n[2] = 1 in 2-D) */
    float   origin[3];                  /* position of node (0, 0, 0) */
    float   cell;                       /* edge of the cubic cell (> 0) */
    int32_t mode;                       /* MPDX_GRID_LINEAR | MPDX_GRID_NEAREST */
} mpdx_field;
#define MPDX_GRID_LINEAR  0
#define MPDX_GRID_NEAREST 1

typedef struct mpdx_guide_params {
    int32_t robot;                      /* MPDX_ROBOT_* */
    int32_t q_dim;                      /* 2, 3 (point mass), 7 (Panda) or the chain's n_joints (1 ... 8); state dim D = 2*q_dim (pos + vel) */
    int32_t ws_dim;                     /* workspace dimension 2 or 3 */
    int32_t interpolate;                /* interpolate_trajectories_for_collision (guides.py:152) */
    int32_t n_interp;                   /* num_interpolated_points_for_collision; effective reference value 128 */
    int32_t clip_grad;                  /* clip_grad (guides.py:151), rule 'norm' */
    float   max_grad_norm;              /* 1.0 */
    float   mins[16], maxs[16];         /* LimitsNormalizer limits of the trajectory field (normalization.py:92-93) */
    float   cutoff_margin;              /* obstacle_cutoff_margin (inference.py:110) */
    float   link_margin;                /* point-mass collision radius */
    int32_t n_fields;
    mpdx_field fields[MPDX_MAX_FIELDS];
    int32_t use_gp;                     /* CostGPTrajectory present */
    float   gp_weight;                  /* weight_grad_cost_smoothness (inference.py:56) */
    float   dt;                         /* trajectory_duration / n_support_points (inference.py:120) */
    float   sigma_gp;                   /* 1.0 */
    const float* prims;                 /* device pointer: primitive table (n_scenes > 1: the scene blocks + the shared tail, see the scene members below) */
    int32_t n_prim_floats;
    /* --- switches for what the reference's empty submodules leave undecidable / for options of guides.py --- */
    int32_t clip_rule;                  /* 0: clip_grad_rule 'norm' (guides.py:224-230); 1: 'value' (guides.py:232-236) */
    float   max_grad_value;             /* 0.1 (guides.py:151) */
    int32_t gp_half_factor;             /* 0: cost_GP = sum e^T Qinv e (default);  1: 1/2 sum e^T Qinv e (GPMP2's convention) */
    int32_t identity_normalizer;        /* 0: LimitsNormalizer (mins / maxs above, whole-tensor range test; normalization.py:156-167);
                                         * 1: x is ALREADY in robot units (Identity :111-116; no range test): the trajectory optimiser of
                                         *    generate_trajectories (scripts/generate_data/generate_trajectories.py:94-117) works on raw trajectories;
                                         * 2: GaussianNormalizer (:140-141): x * stds + means with means in `mins`, stds in `maxs`, no range test */
    const float* grids;                 /* device pointer: the planes of the MPDX_FIELD_GRID fields (NULL when there is none); stays in global memory */
    int32_t n_grid_floats;              /* floats in grids (every plane must lie inside) */
    /* --- several obstacle scenes in one batch (an extension: the reference plans one task per call).  All four members zero (or n_scenes = 1):
     * one scene, prims as described above - the block behaves exactly as before these members existed.
     * n_scenes > 1: the trajectories of one launch see different primitive tables.  prims then holds
     *     [ scene block 0 | scene block 1 | ... | scene block n_scenes-1 | shared tail ]
     *   scene block s   scene_stride floats at prims + s * scene_stride:
     *                     words 0 .. 2*MPDX_MAX_FIELDS-1 (int32 bit patterns, the block header): n_spheres of field 0 .. MPDX_MAX_FIELDS-1 IN THIS
     *                     SCENE, then n_boxes of field 0 .. MPDX_MAX_FIELDS-1 in this scene (entries of fields that are not OBJECTS fields: ignored);
     *                     then the sphere (4 floats each) and box (6 floats each) tables of the per-scene fields, unused capacity zero
     *   shared tail     the n_prim_floats - n_scenes * scene_stride floats behind the last block: tables every scene sees (may be empty)
     * A workgroup (= one trajectory) of scene s stages block s and, directly behind it, the shared tail: scene_stride + tail floats.  sphere_off /
     * box_off of an OBJECTS field are offsets into THAT image, the same for every scene: a table at an offset < scene_stride lies in the scene
     * block (it must start behind the header and end inside the block) and differs per scene; a table at an offset >= scene_stride lies in the
     * shared tail.  n_spheres / n_boxes of the field are the CAPACITY of its table (the maximum over the scenes); a scene scans
     * min(header count, capacity) primitives, in table order - the result is, bit for bit, that of a single-scene block holding those primitives.
     * WORKSPACE, SELF and GRID fields are the same for every scene (a grid stands for the fixed environment).
     * Trajectory b uses scene scene_of_ctx[b / scene_n_per_ctx], clamped into [0, n_scenes) by the kernels: a bad entry reads another scene, never
     * out of bounds.  The caller sizes scene_of_ctx: ceil(B / scene_n_per_ctx) entries for a batch of B.
     * Entry points that take scenes: mpdx_guide_step, mpdx_guide_step_scaled, mpdx_guide_time, mpdx_traj_metrics, mpdx_traj_metrics_mask, mpdx_plan
     * (checked on the host before any launch: MPDX_E_INVALID, message naming the scene member at fault); mpdx_gpmp_step, mpdx_rrt_connect,
     * mpdx_rrt_paths and mpdx_sdf_grid_bake refuse n_scenes > 1. */
    int32_t n_scenes;                   /* 0 or 1: one scene */
    int32_t scene_stride;               /* floats per scene block: a multiple of 4, >= 2*MPDX_MAX_FIELDS + the per-scene tables */
    const int32_t* scene_of_ctx;        /* device array: scene index per group of scene_n_per_ctx consecutive trajectories */
    int32_t scene_n_per_ctx;            /* trajectories per entry of scene_of_ctx (a member: the metrics entry points have no n_per_ctx argument) */
    /* --- MPDX_ROBOT_CHAIN: a serial kinematic chain described by a table (an extension: the reference builds one of its own robots by name).
     * Both members zero: the block behaves exactly as before they existed (they are looked at for robot == MPDX_ROBOT_CHAIN only).
     * The table is fp32 words; integer entries are int32 bit patterns (as the scene header); sizes in floats:
     *   header   4 floats                       n_joints (1 ... MPDX_ROBOT_CHAIN_MAX_JOINTS), n_spheres (1 ... MPDX_ROBOT_CHAIN_MAX_SPHERES),
     *                                           n_pairs (0 ... MPDX_ROBOT_CHAIN_MAX_PAIRS), 0                                          [int32]
     *   joint j  MPDX_ROBOT_CHAIN_JOINT_FLOATS  R[9] row-major rotation, parent frame from joint frame at q = 0 | t[3] translation |
     *                                           type [int32]: MPDX_ROBOT_CHAIN_REVOLUTE about the joint frame's z, MPDX_ROBOT_CHAIN_PRISMATIC
     *                                           along it | 3 pad floats
     *   sphere s MPDX_ROBOT_CHAIN_SPHERE_FLOATS frame [int32]: 0 = the fixed base, k = moves with joint k (1-based) | offset[3] in that frame |
     *                                           radius | 3 pad floats
     *   pair     2 floats                       sphere indices (a, b) of a self-collision pair                                          [int32]
     * Forward kinematics:  T_0 = I;  T_j = T_{j-1} [R_j | t_j] M_j(q_j),  M = Rot_z(q) (revolute) or Trans_z(q) (prismatic);  z_j = third column
     * of T_j's rotation, O_j its origin;  sphere centre P_s = O_f + Rot_f offset_s  (f = frame of s; frame 0: P_s = offset_s).  An arbitrary joint
     * axis or a base pose is folded into R and t by the caller.  The Panda's modified-DH frame [Rot_x(alpha) Trans_x(a) Trans_z(d)] Rot_z(theta) is
     * of this form (Rot_z and Trans_z commute).  Joint gradients of a force F_s on sphere s:  revolute g_j = z_j . sum_s (P_s - O_j) x F_s,
     * prismatic g_j = z_j . sum_s F_s, over the spheres with frame(s) >= j; a base-frame sphere feels forces and gives no gradient.
     * Hinges: objects / workspace relu(r_s + cutoff_margin - sdf), self relu(r_a + r_b - |P_a - P_b|); link_margin is not used.
     * A chain robot takes MPDX_FIELD_OBJECTS, MPDX_FIELD_WORKSPACE and MPDX_FIELD_SELF fields (scene batches included); a MPDX_FIELD_GRID field
     * is refused, and so is ws_dim != 3 (a planar arm is a chain whose axes are all z, among 3-D primitives).
     * Checked on the host before any launch (MPDX_E_INVALID, message naming the member at fault): counts inside the caps, n_chain_floats covers
     * the table, q_dim == n_joints, ws_dim == 3, every frame <= n_joints, pair indices < n_spheres, radii > 0, every R orthonormal to 1e-4, type
     * 0 or 1, a MPDX_FIELD_SELF field only with n_pairs > 0, no MPDX_FIELD_GRID field.  The table is read for this check (a device table is
     * copied to the host once per (pointer, size) and the verdict remembered; the kernels clamp every index they take from the table, so a
     * table rewritten in place afterwards reads other entries, never memory outside it).
     * Entry points that take a chain: mpdx_guide_step, mpdx_guide_step_scaled, mpdx_guide_time, mpdx_traj_metrics, mpdx_traj_metrics_mask,
     * mpdx_plan, and mpdx_ik_solve (a chain only); mpdx_gpmp_step, mpdx_rrt_connect, mpdx_rrt_paths and mpdx_sdf_grid_bake know the built-in robots only. */
    const float* chain;                 /* device pointer: the chain table (NULL unless robot == MPDX_ROBOT_CHAIN) */
    int32_t n_chain_floats;             /* floats in chain: >= 4 + 16 n_joints + 8 n_spheres + 2 n_pairs */
    /* --- tool-axis constraint of a chain robot ("carry it upright"; an extension: the reference has no task-space cost).  All members zero
     * (tool_frame == 0): no tool term - the block behaves exactly as before these members existed.
     * Fixed per guide: a frame f = tool_frame (1 ... n_joints), a unit axis a = tool_axis in that frame, a unit axis u = tool_world in the world and
     * c* = tool_cos_min = cos(max_tilt).  On every interpolated point i of a trajectory (the points the collision terms use), all in fp32:
     *   1. Rot_f(q_i) by the forward-kinematics recurrence of the chain table above (sinf / cosf);  w_i = Rot_f(q_i) a
     *   2. d_i = u . w_i;   c_i = relu(c* - d_i);   cost = sum_i c_i
     *   3. d c_i / d q_j = -[c_i > 0] z_j . (w_i x u)   for a revolute joint j <= f (1-based; z_j as above: the geometric Jacobian's angular part);
     *      0 for a prismatic joint and for every joint j > f; the velocity dims get 0
     *   4. the term is a cost of its own in the composite, handled as each collision cost is (guides.py:192-207): its point gradients are gathered to
     *      the supports by the transpose of the interpolation (fixed order), clipped by the guide's clip rule over all D dims, the endpoints
     *      zeroed, multiplied by tool_weight and summed with the collision terms (behind them) before the GP prior is added.
     * At d_i = -1 (the tool axis exactly opposite) w_i x u = 0 and the gradient vanishes although the hinge is active: a saddle of the cost, as
     * it is in exact arithmetic.  It is not worked around.
     * Checked on the host before any launch (MPDX_E_INVALID, message naming the member): robot != MPDX_ROBOT_CHAIN (the Panda takes the term as
     * RobotChain.panda()), tool_frame outside 1 ... n_joints, an axis that is not finite or not unit to 1e-4, tool_cos_min outside [-1, 1], a
     * tool_weight that is not finite.
     * Entry points that take the term: mpdx_guide_step, mpdx_guide_step_scaled, mpdx_guide_time, mpdx_plan (scene batches included) and
     * mpdx_traj_tool_metrics; mpdx_traj_metrics / mpdx_traj_metrics_mask check the members and report collisions as before; mpdx_gpmp_step,
     * mpdx_rrt_connect, mpdx_rrt_paths and mpdx_sdf_grid_bake refuse tool_frame != 0 (the baseline planners do not honour the constraint). */
    int32_t tool_frame;                 /* 0: no tool term; 1 ... n_joints: the frame that carries the axis */
    float   tool_axis[3];               /* a: unit axis in that frame */
    float   tool_world[3];              /* u: unit axis in the world */
    float   tool_cos_min;               /* cos(max_tilt), in [-1, 1] */
    float   tool_weight;                /* weight of the term (the weight_grad_cost_* of the collision terms) */
} mpdx_guide_params;
#define MPDX_ROBOT_CHAIN_MAX_JOINTS    8
#define MPDX_ROBOT_CHAIN_MAX_SPHERES   16
#define MPDX_ROBOT_CHAIN_MAX_PAIRS     24
#define MPDX_ROBOT_CHAIN_HEADER_FLOATS 4
#define MPDX_ROBOT_CHAIN_JOINT_FLOATS  16
#define MPDX_ROBOT_CHAIN_SPHERE_FLOATS 8
#define MPDX_ROBOT_CHAIN_REVOLUTE      0
#define MPDX_ROBOT_CHAIN_PRISMATIC     1
#define MPDX_SCENE_HEADER_WORDS 8            /* 2 * MPDX_MAX_FIELDS */
#define MPDX_SCENE_MAX_STAGED_FLOATS 12288   /* scene_stride + shared tail: the kernels' LDS budget for one staged table */

/* one guide iteration on x[B,H,D] (normalised).  grad_out == NULL: x <- hard_cond(x + guide(x)) in place and
 * absmax_out[ctx] <- atomicMax(max|x_new|) ; grad_out != NULL: grad_out <- guide(x), x untouched.
 * absmax_in[ctx] holds the bit pattern of max|x| over the context's n_per_ctx trajectories (the whole-tensor range
 * test of LimitsNormalizer.unnormalize, normalization.py:160). */
int mpdx_guide_step(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hard_start, const float* hard_goal,
                    const uint32_t* absmax_in, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, void* stream);
/* the same with the increment multiplied by guide_scale before it is added (scale_grad_by_std, sample_functions.py:77-78) */
int mpdx_guide_step_scaled(const mpdx_guide_params* gp, float* x, float* grad_out, const float* hard_start, const float* hard_goal,
                           const uint32_t* absmax_in, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, float guide_scale,
                           void* stream);
/* measurement helper (bench.py `guided` sub-record): `reps` back-to-back guide launches in gradient-only mode (grad_out
 * <- guide(x); x and the flags untouched, so every launch does the same work) bracketed by ONE HIP-event pair on `stream`;
 * *ms_avg = average time per launch.  Replaces nothing in the reference: guides.py:173-211 is what one launch computes.  Synchronises. */
int mpdx_guide_time(const mpdx_guide_params* gp, float* x, float* grad_out, const uint32_t* absmax_in, int n_per_ctx, int B, int H, int D,
                    int reps, void* stream, float* ms_avg);
/* dev tool: cycle stamps (16 slots per wave x 8 waves, workgroup 0) of one guide launch (gradient-only mode).
 * The three *_trace entry points and the ablation masks of mpdx_bench_layer work only in a library built with -DMPDX_DEV_HOOKS
 * (the production kernels carry no hooks); otherwise they return MPDX_E_STATE. */
int mpdx_guide_trace(const mpdx_guide_params* gp, float* x, const uint32_t* absmax_in, int B, int H, int D, void* stream,
                     long long* stamps128);
/* Which kernel variant mpdx_guide_step takes for this block at batch B: 1 = the Panda's dense variant (large batches, or MPDX_GUIDE_DENSE=1, where
 * its LDS layout fits 80 KB), 0 = every other kernel (the Panda's table variant, point mass, chain); negative: the block is refused.  No launch. */
int mpdx_guide_variant(const mpdx_guide_params* gp, int B, int H, int D);
/* absmax_out[ctx] <- atomicMax over the context's trajectories (caller zeroes absmax_out first) */
int mpdx_absmax(const float* x, uint32_t* absmax_out, int n_per_ctx, int B, int H, int D, void* stream);

/* ---- post-loop metrics: the arithmetic behind task.get_trajs_collision_and_free / compute_fraction_free_trajs /
 * compute_collision_intensity_trajs and compute_smoothness / compute_path_length (inference.py:288-297,311-316;
 * un-vendored, restated).  x_unnormalised [B,H,D]; out4 [B,4] = {#colliding interpolated waypoints, path length,
 * smoothness, #waypoints checked}; n_check = interpolated waypoints per trajectory used for collision checking. */
int mpdx_traj_metrics(const mpdx_guide_params* gp, const float* x_unnormalised, float* out4, int n_check, int B, int H, int D,
                      void* stream);
/* the same, plus the per-waypoint collision flags the count is made of: mask [B, n_check] bytes (1 = the interpolated waypoint
 * collides), or NULL.  compute_collision_intensity_trajs (inference.py:295-297) is the mean of these flags; the parity tests use them to
 * compare the kernel's decisions with an fp64 evaluation waypoint by waypoint. */
int mpdx_traj_metrics_mask(const mpdx_guide_params* gp, const float* x_unnormalised, float* out4, uint8_t* mask, int n_check, int B,
                           int H, int D, void* stream);

/* ---- tool-axis metrics of a chain robot (the tool members of mpdx_guide_params, which must be set: tool_frame != 0; tool_weight is not used).
 * x_unnormalised [B,H,D]; over n_check interpolated points per trajectory (n_check < 2: H), d_i = tool_world . Rot_f(q_i) tool_axis:
 * out2 [B,2] = {min_i d_i, number of checked points with d_i < tool_cos_min}; mask [B, n_check] bytes (1 = d_i < tool_cos_min) or NULL.
 * The largest tilt of a trajectory is acos(min_i d_i).  mpdx_traj_metrics* and their out4 are unchanged.  Replaces nothing in the reference. */
int mpdx_traj_tool_metrics(const mpdx_guide_params* gp, const float* x_unnormalised, float* out2, uint8_t* mask, int n_check, int B, int H, int D,
                           void* stream);

/* ---- bake a signed-distance grid from primitives: replaces GridMapSDF.__init__ (torch_robotics, un-vendored: restated, PARITY UNPINNED), which
 * samples the fixed objects' SDF (and its gradient) on a regular grid once per environment.  One thread per node: node (ix, iy, iz) sits at
 * origin_j + (float)i_j * cell (fp32: one rounded product, one rounded sum); sdf_out[iz][iy][ix] = minimum signed distance to the sphere / box tables
 * of the OBJECTS field gp->fields[field] (the arithmetic of the metrics kernel: IEEE sqrtf); grad_out (or NULL) [iz][iy][ix][4] = the analytic
 * gradient of the arg-min primitive (gx, gy, gz, 0).  n[2] = 1 in 2-D (gp->ws_dim == 2).  The outputs may be planes of a grids buffer. */
int mpdx_sdf_grid_bake(const mpdx_guide_params* gp, int field, float* sdf_out, float* grad_out, const int n[3], const float origin[3], float cell,
                       void* stream);

/* ---- a signed-distance grid from an occupancy grid or a point cloud: an exact Euclidean distance transform on the device (csrc/edt.hpp).  Replaces
 * nothing in the reference (its environments are primitives); it produces the planes the MPDX_FIELD_GRID lookups read from what a depth camera or an
 * occupancy map gives.  Every step is exactly reproducible in numpy (tests/edt_ref.py).
 *
 * Nodes are voxel centres: node (ix, iy, iz) sits at origin + i * cell, as for every grid; occ[iz][iy][ix] is one byte, x fastest, non-zero = occupied;
 * n[2] = 1 in 2-D (there is no ws_dim here: n[2] == 1 IS the 2-D case), else 2 ... 4096 nodes along every axis, at most 2^29 nodes.
 *   d2    free node n: min |n - m|^2 over OCCUPIED nodes m; occupied node: min over FREE nodes m - in cells, exact integers (int32).  Without any
 *         such m (all free / all occupied): d2 = (n[0] + n[1] + n[2])^2, which exceeds every distance inside the grid (and fits int32 with every
 *         intermediate of the separable passes at 4096 nodes per axis).
 *   s     fp32, every operation rounded (no contraction), IEEE sqrtf:  free  s =   cell * (sqrtf((float)d2) - 0.5f)  - inflate
 *                                                                     occupied  s = -(cell * (sqrtf((float)d2) - 0.5f)) - inflate
 *         the half cell puts the surface on the voxel FACE (a free node beside an occupied one: +cell / 2); inflate >= 0 thickens every obstacle.
 *   grad  [nz][ny][nx][4] or NULL (MPDX_GRID_NEAREST needs it, LINEAR does not): along each used axis (s[i+1] - s[i-1]) * k2 at an interior node,
 *         (s[i+1] - s[i]) * k1 / (s[i] - s[i-1]) * k1 at a face node, k1 = 1.0f / cell, k2 = 0.5f / cell (fp32, taken once on the host); one rounded
 *         subtraction and one rounded product each; the unused axis and the fourth word are 0.
 *   d2_out (or NULL, for tests): the d2 above per node.
 * ws: mpdx_sdf_grid_edt_ws_bytes(n) bytes of device memory (4-byte aligned; the library allocates nothing and never synchronises); the size function
 * returns 0 for a refused n.  sdf_out / grad_out may be planes of a grids buffer (grad_out 16-byte aligned).
 *
 * mpdx_occupancy_from_points: points [P][3] fp32 (z ignored in 2-D); u_j = (p_j - origin_j) * inv, inv = 1.0f / cell (the two rounded operations of the
 * lookups' cell coordinate), i_j = rintf(u_j) (half to even).  A point with a non-finite used coordinate or an i_j outside [0, n_j - 1] is DROPPED (not
 * clamped); otherwise occ[node] = 1.  Bytes are only ever set, so several clouds accumulate into one map; clear it yourself.  n_points == 0: no-op.
 *
 * Refused on the host, before any launch (MPDX_E_INVALID, the message names the argument): a null pointer (grad_out, d2_out may be null), n outside
 * the ranges above, cell not positive and finite, inflate negative or non-finite, a misaligned grad_out, ws_bytes too small, n_points < 0. */
size_t mpdx_sdf_grid_edt_ws_bytes(const int n[3]);
int mpdx_sdf_grid_from_occupancy(const uint8_t* occ, float* sdf_out, float* grad_out, int32_t* d2_out, const int n[3], float cell, float inflate, void* ws,
                                 size_t ws_bytes, void* stream);
int mpdx_occupancy_from_points(const float* points, int n_points, uint8_t* occ, const int n[3], const float origin[3], float cell, void* stream);

/* ---- a signed-distance grid from a triangle mesh: every grid node against every triangle, on the device (csrc/mesh_sdf.hpp).  Replaces nothing in the
 * reference; it produces the planes the MPDX_FIELD_GRID lookups read from what a CAD export, a scanned fixture or URDF collision geometry gives, with
 * the surface where the mesh has it (no half-cell quantisation).  Restated in fp64 numpy in tests/mesh_ref.py; the device is held to it within bounds.
 * All pointers are device pointers: vertices [V][3] fp32, faces [F][3] int32 (counter-clockwise seen from outside), sdf_out [nz][ny][nx], x fastest.
 * 3-D only: 2 ... 4096 nodes along every axis, at most 2^29 nodes, 1 ... 2^20 faces.
 *   p     node (ix, iy, iz) sits at origin_j + (float)i_j * cell (fp32: one rounded product, one rounded sum, as for mpdx_sdf_grid_bake).
 *   d     min over faces f of |p - cp_f(p)|, cp_f = the closest point of the closed triangle (Ericson's region test: a vertex, an edge or the face),
 *         evaluated on the vertices relative to the node (A = a - p, B = b - p, C = c - p) and measured FROM THE CLOSEST POINT (r = p - cp, d2 = r . r;
 *         no projected-distance formula: the error in d stays linear in the rounding even for a node in a triangle's plane).  The best d2 is kept with
 *         fminf (a NaN from a degenerate face never wins); one IEEE sqrtf per node at the end.
 *   w     the generalised winding number (1 / 4 pi) sum_f Omega_f, Omega = 2 atan2f(det[A B C], |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|) (Van Oosterom
 *         and Strackee), summed in fp32 in face order per node: the same bits from run to run.  A node is inside where w > 0.5.
 *   s     MPDX_MESH_SIGN_WINDING:  s = (w > 0.5 ? -d : d) - inflate;  MPDX_MESH_SIGN_NONE:  s = d - inflate, w is not evaluated (open sheets and scans:
 *         inflate >= 0 gives them thickness).
 *   grad  [nz][ny][nx][4] or NULL (MPDX_GRID_NEAREST needs it, LINEAR does not): the differences of s stated for mpdx_sdf_grid_from_occupancy, by
 *         the same kernel (k1 = 1.0f / cell, k2 = 0.5f / cell).
 *   wind_out (or NULL, for tests): w per node; refused with MPDX_MESH_SIGN_NONE.
 * A face with an index outside [0, n_vertices) or a non-finite vertex is skipped on the device (d2 = +inf, Omega = 0): it is never read out of bounds.
 * The library allocates nothing, takes no workspace and never synchronises.  The work is nodes x faces pair tests (rates: profiles/mesh_sdf_probe.md):
 * the host splits the node range into launches of at most 2^33 pairs and refuses a call of more than 2^38 (use a coarser grid or a decimated mesh).
 *
 * Refused on the host, before any launch (MPDX_E_INVALID, the message names the argument): a null vertices, faces, sdf_out, n or origin; n_vertices < 3;
 * n_faces outside 1 ... 2^20; n outside the ranges above (n[2] = 1: "3-D only"); more than 2^29 nodes; cell not positive and finite; inflate negative or
 * non-finite; a non-finite origin; an unknown sign_mode; wind_out with MPDX_MESH_SIGN_NONE; vertices, faces, sdf_out or wind_out not 4-byte aligned,
 * grad_out not 16-byte aligned; nodes x n_faces > 2^38. */
#define MPDX_MESH_SIGN_WINDING 0
#define MPDX_MESH_SIGN_NONE    1
int mpdx_sdf_grid_from_mesh(const float* vertices, int n_vertices, const int32_t* faces, int n_faces, float* sdf_out, float* grad_out /* or NULL */,
                            float* wind_out /* or NULL: w per node, for tests */, const int n[3], const float origin[3], float cell, float inflate,
                            int sign_mode, void* stream);

/* ---- depth-camera fusion: projective TSDF integration (KinectFusion-style truncated signed distance) into per-node planes on the device
 * (csrc/tsdf.hpp).  Replaces nothing in the reference; it fuses depth frames into the occupancy bytes mpdx_sdf_grid_from_occupancy turns into the
 * sdf and gradient planes.  Every step is exactly reproducible in numpy (tests/tsdf_ref.py): tsdf, weight and occ are held to it bit for bit.
 * Every fp32 operation below is one rounded operation (the library builds with -ffp-contract=on; the kernel spells them out).
 *   camera  pinhole, no distortion (undistort first); OpenCV frame: x right, y down, z forward; depth [height][width] fp32 on the device, metres
 *           along z; pixel (iu, iv) has its centre at image coordinate (iu, iv).  cam_from_world and world_from_cam are row-major 3x4 [R | t], formed
 *           in float64 by the caller and rounded to fp32 (one need not be the exact inverse of the other in fp32).
 *   p       node (ix, iy, iz) sits at origin_j + (float)i_j * cell (one rounded product, one rounded sum, as for mpdx_sdf_grid_bake).
 * Per node, for each camera in the order given (A = cam_from_world, B = world_from_cam):
 *   1. x_j = ((A[j][0] p0 + A[j][1] p1) + A[j][2] p2) + A[j][3]; the camera is skipped unless x2 > 0 (false for NaN).
 *   2. u = fx * (x0 / x2) + cx, v = fy * (x1 / x2) + cy; ru = rintf(u), rv = rintf(v) (half to even); the pixel must satisfy 0 <= ru <= width - 1
 *      and 0 <= rv <= height - 1, tested on the floats before any conversion (a non-finite u or v is no measurement); iu = (int)ru, iv = (int)rv.
 *   3. d = depth[iv * width + iu] is a measurement only if min_depth <= d <= max_depth (NaN, +-inf, 0 and negative values are rejected).
 *   4. robot mask (n_spheres > 0): P_cam = (((float)iu - cx) / fx * d, ((float)iv - cy) / fy * d, d), P_j = ((B[j][0] P0 + B[j][1] P1) + B[j][2] P2)
 *      + B[j][3]; the measurement is skipped (it neither carves nor occupies) if (dx * dx + dy * dy) + dz * dz < r * r for any sphere (c, r),
 *      d = P - c.  r is the padded radius.
 *   5. s = d - x2; skipped if s < -trunc (the node is occluded); o = fminf(s, trunc) / trunc.
 *   6. T = (T * W + o) / (W + 1), then W = fminf(W + 1, max_weight).
 * After all cameras, occ = (W > 0 && T < 0) for EVERY node, nodes no camera saw in this call included.  So an unobserved node (W == 0) is free: a
 * solid's unseen interior is free behind an occupied shell about trunc thick, and the inflate of the transform still applies.  Start a map with
 * tsdf = weight = 0 (a NaN tsdf at W = 0 would stay NaN: 0 * NaN).
 *
 * One thread per node (256 per workgroup, x fastest: the plane reads and writes are coalesced); the camera records and the spheres are kernel
 * arguments (uniform: scalar loads, no copy).  No atomics, no workspace, no scratch; the library allocates nothing and never synchronises.
 * tsdf, weight [nz][ny][nx] fp32 and occ [nz][ny][nx] bytes are device pointers, read and written in place; spheres is a HOST array [n][4]
 * (centre, radius), copied into the launch.  3-D grids only.
 *
 * Refused on the host, before any launch (MPDX_E_INVALID, the message names the argument): n outside 2 ... 4096 along every axis or more than 2^29
 * nodes (n[2] = 1: "3-D only"); n_cams outside 1 ... 8 or cams null; a null or not 4-byte aligned depth, width or height outside 1 ... 8192; fx or
 * fy not positive and finite; a non-finite cx, cy or matrix entry; min_depth < 0, max_depth <= min_depth or a non-finite bound; n_spheres outside
 * 0 ... 64, spheres null with n_spheres > 0, a non-finite sphere value or a negative radius; cell not positive and finite; a non-finite origin; trunc
 * not positive and finite; max_weight outside 1 ... 2^24; a null or misaligned tsdf, weight (4 bytes) or occ. */
#define MPDX_TSDF_MAX_CAMS     8
#define MPDX_TSDF_MAX_SPHERES 64
typedef struct mpdx_depth_camera {
    const float* depth;                 /* device pointer: [height][width] fp32, metres */
    int32_t width, height;
    float fx, fy, cx, cy;
    float cam_from_world[12];           /* row-major 3x4 */
    float world_from_cam[12];           /* row-major 3x4 */
    float min_depth, max_depth;
} mpdx_depth_camera;
int mpdx_tsdf_integrate(const mpdx_depth_camera* cams, int n_cams, const float* spheres /* host [n][4]: centre, radius */, int n_spheres,
                        float* tsdf, float* weight, uint8_t* occ, const int n[3], const float origin[3], float cell, float trunc, float max_weight,
                        void* stream);

/* ---- baseline planners of the dataset-generation script: replaces `HybridPlanner(RRTConnect x n via
 * MultiSampleBasedPlanner, GPMP2).optimize()` of scripts/generate_data/generate_trajectories.py:68-120.  The planners are
 * un-vendored in the reference (mp_baselines submodule empty: PARITY UNPINNED); the published algorithms are restated
 * (oracle/gpmp.py).  Trajectories and configurations are in RAW robot units (gp->identity_normalizer semantics).
 *
 * GPMP2 (Mukadam et al. 2018) - one Levenberg-Marquardt iteration per call for B trajectories:
 *   F = 1/2 sum e_i^T Q^-1 e_i / sigma_gp^2 + 1/2 sum c^2 / sigma_obs^2   (constant-velocity GP prior of gp->dt / gp->sigma_gp between the
 *   supports; hinge collision factors of gp->fields on the gp->n_interp interpolated points; start and goal states fixed).
 *   state[b] = {F(x_b), lambda_b, accepted steps, F(last candidate)}: initialise to {3e38, lambda_init, 0, 0} and delta to 0.
 *   Each call judges the pending candidate x + delta (accept if it lowers F: x <- x + delta, lambda *= lambda_down; else lambda *= lambda_up),
 *   then (solve != 0) linearises at x and writes the next proposal  delta = -step (K^-1 + J^T J / sigma_obs^2 + lambda diag)^-1 grad F
 *   (block-tridiagonal system, banded LDL^T in LDS).  Call iters times with solve = 1 and once more with solve = 0.
 *   A trajectory whose accepted step no longer lowers F (relative 1e-7) or whose lambda reached lambda_max is CONVERGED: its lambda is
 *   stored negated and further calls return at once for it.
 *   adaptive == 0: every candidate is accepted and lambda stays fixed (damped Gauss-Newton with a fixed step).
 * The three planner entry points know primitive fields only: a MPDX_FIELD_GRID field is refused with MPDX_E_INVALID (grid fields: guide and metrics only). */
typedef struct mpdx_gpmp_opts {
    float   sigma_obs;
    float   lambda_up, lambda_down, lambda_min, lambda_max;
    float   step;
    int32_t adaptive;
} mpdx_gpmp_opts;
int mpdx_gpmp_step(const mpdx_guide_params* gp, const mpdx_gpmp_opts* opts, float* x, float* delta, float* state, int B, int H, int D,
                   int solve, void* stream);

/* RRT-Connect (Kuffner & LaValle 2000) for n independent problems, the WHOLE search in one launch (one workgroup per problem):
 *   start, goal [n, q]; nodes [n, 2, max_nodes, q] / parent [n, 2, max_nodes] the two trees (tree 0 from the start, tree 1 from the goal);
 *   count [n, 2] nodes per tree; link [n, 2] the node indices where the trees met (-1: not solved within max_iters / max_nodes);
 *   iters [n] iterations used.  Samples are uniform in [q_lo, q_hi] (Philox keyed by seed, problem, iteration); an edge is checked on
 *   n_edge_checks interpolated configurations with the link radius only (as mpdx_traj_metrics). */
typedef struct mpdx_rrt_opts {
    float    q_lo[8], q_hi[8];
    float    step;
    int32_t  max_nodes, max_iters, max_connect_steps, n_edge_checks;
    uint64_t seed;
} mpdx_rrt_opts;
int mpdx_rrt_connect(const mpdx_guide_params* gp, const mpdx_rrt_opts* opts, const float* start, const float* goal, float* nodes,
                     int32_t* parent, int32_t* count, int32_t* link, int32_t* iters, int n, void* stream);

/* RRT-Connect post-processing on the device: per problem the path start ... goal is extracted from the two trees mpdx_rrt_connect grew, shortcut
 * greedily (`rounds` passes, edges checked on n_edge_checks interpolated configurations) and resampled uniformly in arc length to H support
 * points with central-difference velocities -> trajs_out[n][H][2 q_dim]; path_len[n] (or NULL) = nodes of the shortcut path.  An unsolved problem
 * becomes the straight line.  Replaces the path extraction / smoothing that MultiSampleBasedPlanner + HybridPlanner do between RRTConnect and GPMP2
 * (scripts/generate_data/generate_trajectories.py:68-105; un-vendored: the published algorithms, parity unpinned).
 *   path        start ... link[b][0] along tree 0's parents (root first), then link[b][1] ... goal along tree 1's parents.  A NEGATIVE entry in
 *               either link means unsolved.  A path of more than 1024 nodes is treated as unsolved too: both give the straight line
 *               [start[b], goal[b]] and path_len 2 (start / goal are read for these problems only; the roots of the trees otherwise).
 *   shortcut    per round, from node i to the LAST later node whose edge is free, else to the next node; it ends when a round removes nothing
 *               (one round of this rule already leaves a fixed point) or 2 nodes are left; rounds = 0: none.  An edge is checked on the
 *               configurations (1 - w) qa + w qb, w = c / (n_edge_checks - 1), end points included, link radius only.
 *   resample    u_h = total arc length * h / (H - 1); segment = first node with cumulative length > u_h, clamped to [1, m - 1]; linear
 *               interpolation (segment length clamped to 1e-12: start == goal gives H copies of it); supports 0 and H - 1 are exactly the
 *               first and the last node; velocities (x[h + 1] - x[h - 1]) / (2 dt), zero at both ends.
 *   refused with MPDX_E_INVALID before any launch: a null pointer (path_len may be null), n < 1, max_nodes < 2, H outside [2, 1024], dt <= 0,
 *               n_edge_checks outside [2, 256], rounds < 0, and a max_nodes whose LDS need
 *               4 (1024 q_dim + H q_dim + 2048 + 2 max_nodes + 16 + n_prim_floats) bytes exceeds 160 KB. */
int mpdx_rrt_paths(const mpdx_guide_params* gp, const float* start, const float* goal, const float* nodes, const int32_t* parent, const int32_t* link,
                   float* trajs_out, int32_t* path_len, int n, int max_nodes, int H, float dt, int n_edge_checks, int rounds, void* stream);

/* ---- inverse kinematics of a chain robot: n end-effector targets x `restarts` seeds in one launch.  Replaces nothing in the reference: it takes
 * every goal as a joint configuration (inference.py:161 draws one with task.random_coll_free_q); a task-space goal for a table-driven robot is
 * this package's extension.  A redundant arm has a set of configurations for one pose: the restarts that converge are
 * samples of it (collision filtering stays with mpdx_traj_metrics).
 *
 * Damped least squares (Levenberg-Marquardt), all in fp32, one independent problem per (target, restart).  Per iteration, in this order:
 *   FK         of frame f = opts->frame (1 ... n_joints; frame 0 is the fixed base and is refused) by the recurrence of the chain table above,
 *              T_j = T_{j-1} [R_j | t_j] M_j(q_j) with sinf / cosf, keeping O_j and z_j for j <= f; tool point p = O_f + Rot_f offset.
 *   residual   e = [p - p*; w_r e_R],  e_R = 1/2 sum_i Rot_f[:, i] x R*[:, i]  (it points from the current to the target orientation);
 *              w_r = rot_weight; w_r = 0: position only, the rotation rows are skipped (R* is not read into the result; err_out[..][1] = 0).
 *   Jacobian   joint j <= f contributes one column: revolute Jv = z_j x (p - O_j), Jw = z_j; prismatic Jv = z_j, Jw = 0; joints j > f: zero columns.
 *              The residual's Jacobian is J = [Jv; -w_r Jw]: the rotation block is the usual geometric-Jacobian Gauss-Newton approximation
 *              (d e_R / dq = -Jw to first order in e_R, exact at e_R = 0).
 *   solve      (J^T J + lambda I) dq = -J^T e  by a Cholesky factorisation of the n_joints x n_joints system; a zero column gives dq_j = 0 exactly.
 *              Every squared pivot is >= lambda in exact arithmetic and is floored there (max(d, lambda)): rounding cannot make dq non-finite.
 *   candidate  q_c = min(max(q + dq, q_lo), q_hi),  F = 1/2 |e(q)|^2,  F_c = 1/2 |e(q_c)|^2.
 *              adaptive = 1: accept (q <- q_c) iff F_c < F, then lambda <- max(lambda * lambda_down, lambda_min); else lambda <- min(lambda * lambda_up,
 *              lambda_max).  adaptive = 0: every candidate is accepted and lambda stays lambda_init (the semantics of mpdx_gpmp_opts.adaptive).
 *   stop       before every iteration (and once behind the last): converged when |p - p*| <= pos_tol and, with w_r > 0, |e_R| <= rot_tol and
 *              trace(Rot_f^T R*) > 1 (e_R also vanishes at a rotation error of 180 degrees: the trace rules that zero out); a restart also
 *              stops after max_iters iterations.  A converged restart is left as it is.
 * Seeds: q_init [n][restarts][n_joints], clamped into [q_lo, q_hi] (a seed inside the limits is used bit for bit); or NULL: restart r of target i draws
 *   u = philox_uniform4(seed, (i << 32) | (2 r + k)), k = 0 for joints 0 ... 3 and k = 1 for joints 4 ... 7 (the uniforms of mpdx_rrt_connect: Philox4x32-10,
 *   u = ((word >> 8) + 0.5) / 2^24) and starts at fmaf(q_hi - q_lo, u, q_lo), clamped into [q_lo, q_hi].
 * Outputs per restart: q_out [n][restarts][n_joints], always inside the limits; err_out [n][restarts][2] = |p - p*| and |e_R| at
 *   q_out; status [n][restarts]: bit 0 = converged, bits 8 ... = iterations used.  max_iters = 0 returns the (clamped) seeds with their errors.
 * Of gp only the chain members count: robot (MPDX_ROBOT_CHAIN), q_dim, chain, n_chain_floats, checked as for the guide; the fields, the primitive
 * table and the scene members are ignored.  target [n][12]: p*, then R* row-major (an orthonormal matrix; the identity will do with w_r = 0).
 * Refused with MPDX_E_INVALID before any launch, the message naming the argument: a null pointer (q_init may be null), n outside 1 ... 65535,
 *   restarts outside 1 ... 4096, a built-in robot id, a bad chain table, frame outside 1 ... n_joints, a non-finite offset, q_lo > q_hi or
 *   non-finite limits, rot_weight < 0, non-positive pos_tol / rot_tol / lambda_init, max_iters < 0, and with adaptive = 1 lambda_up < 1,
 *   lambda_down outside (0, 1], lambda_min <= 0 or lambda_max < lambda_min. */
typedef struct mpdx_ik_opts {
    int32_t  frame;                     /* 1 ... n_joints: the frame whose tool point is placed */
    float    offset[3];                 /* tool point in that frame */
    float    q_lo[8], q_hi[8];          /* joint limits (entries past n_joints are not read) */
    float    rot_weight;                /* w_r (metres per radian); 0: position only */
    float    pos_tol, rot_tol;
    float    lambda_init, lambda_up, lambda_down, lambda_min, lambda_max;
    int32_t  adaptive;
    int32_t  max_iters;
    uint64_t seed;
} mpdx_ik_opts;
int mpdx_ik_solve(const mpdx_guide_params* gp, const mpdx_ik_opts* opts, const float* target, const float* q_init, float* q_out, float* err_out,
                  int32_t* status, int n, int restarts, void* stream);

/* ---- the whole planning loop: replaces GaussianDiffusionModel.p_sample_loop driven by run_inference
 * (diffusion_model_base.py:157-182,285-316) with sample_fn=ddpm_sample_fn.  Everything is enqueued on `stream`
 * without a single host synchronisation: the t-dependent branches of the reference (`t_single < 0`,
 * `t_single < t_start_guide`, sample_functions.py:28-29,39) depend only on the integer loop index.
 *   coefs  : host array [T], entry t = the scalars of timestep t (see mpdx_step_coefs)
 *   x      : [B,H,D]; in: x_T ~ N(0,I) (hard conditioning is applied here, :165-166); out: the final trajectories
 *   noise  : [T + n_without_noise, B,H,D] the randn_like draw of each loop iteration, in loop order; or NULL: every iteration
 *            draws its noise in place from the Philox stream (rng_seed, rng_offset) - iteration k takes elements
 *            [(k+1) n, (k+2) n), n = B*H*D, of the stream whose first n elements are x_T as written by
 *            mpdx_randn(x, n, rng_seed, rng_offset): bit-identical to passing the pre-generated tensor, without its
 *            (T + n_without_noise) * n * 4 bytes (2.4 GB for a 6400-trajectory Panda shard)
 *   chain  : NULL or [T + n_without_noise + 1, B,H,D] <- x after every iteration, index 0 = conditioned x_T
 *            (the 'diffsteps b h d' layout run_inference returns, :310)
 *   guide  : NULL (planner_alg 'diffusion_prior') or the cost guide; applied n_guide_steps times on the posterior
 *            mean of every iteration whose loop index i < t_start_guide (sample_functions.py:39-48), each increment times
 *            coefs[t].guide_scale; n_guide_steps == 0 skips guidance (the reference's empty range(0) loop)
 *   guide_flags : device scratch, (T + n_without_noise) * (n_guide_steps + 1) * ceil(B / n_per_ctx) uint32
 *   n_per_ctx   : trajectories per start/goal context (n_samples); contexts are consecutive blocks of the batch   */
int mpdx_plan(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T, const mpdx_step_coefs* coefs,
              int n_without_noise, float* x, const float* noise, const float* hard_start, const float* hard_goal,
              float* chain, int B, float* ws, const mpdx_guide_params* guide, int n_guide_steps, int t_start_guide,
              uint32_t* guide_flags, int n_per_ctx, uint64_t rng_seed, uint64_t rng_offset, void* stream);

/* ---- measurement helpers (bench.py's roofline leg; not used by the planning path) ----
 * One U-Net pass with a hipEvent pair around every kernel launch, on `stream`.  This call DOES synchronise the
 * stream (it reads the events).  ms_out[i] = duration of launch i; flops_out[i] = its algorithmic FLOPs
 * (2*C_out*B*L_out*C_in*taps summed over the layers of the launch, 0 for the final 1x1+step kernel); names_out[i] ->
 * layer name, or "fused[...]" for a whole-trajectory fused segment (disable fusion with MPDX_FUSED=0).
 * Returns the number of launches written (<= cap) in *n_out. */
int mpdx_unet_profile(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T, const float* x, int t,
                      int B, float* ws, void* stream, int cap, float* ms_out, double* flops_out,
                      const char** names_out, int* n_out);
/* dev tool: per-phase s_memtime stamps (7 each) of the first and the last workgroup of one launch of layer `layer` */
int mpdx_layer_trace(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, const float* x, int layer, int B, float* ws,
                     void* stream, long long* stamps32);
/* dev tool: per-phase s_memtime stamps (workgroup 0; 8 waves x 128 slots) of one launch of fused segment `seg`; seg == number of segments: the
 * joined launch; + 1 / + 2: the seven-layer run / the tail run of mpdx_plan - 32 slots per layer, ten stamps of workgroup 0 / thread 0 each (entry,
 * requests issued, predecessor published, staging issued, staged, k-loop, all waves, partials visible, epilogue, published); *nops_out = its layers */
int mpdx_fused_trace(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, const float* x, int seg, int B,
                     float* ws, void* stream, long long* stamps_out, int cap, int* n_out, int* nops_out);
/* in-situ timing of launch units [unit_first, unit_last] inside `reps` real U-Net passes (one event pair per pass around the
 * run: real predecessors and cold weights, event cost amortised over the run); *ms_avg = bracketed time per pass. */
int mpdx_unet_time_units(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T, const float* x, int t, int B,
                         float* ws, void* stream, int unit_first, int unit_last, int reps, float* ms_avg);
/* the DIFFERENTIAL form: `reps` back-to-back U-Net passes WITHOUT the launch units whose bit is set in skip_mask (0: nothing skipped)
 * between ONE event pair -> *ms_avg per pass.  A launch class costs (pass with everything) - (pass without the class): no event sits next to the
 * measured launches.  Timing only: the skipped units' consumers read whatever the workspace holds. */
int mpdx_unet_time_without(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, int T, const float* x, int t, int B,
                           float* ws, void* stream, unsigned long long skip_mask, int reps, float* ms_avg);
/* layer index behind launch unit i of mpdx_unet_profile at batch B (-1: fused whole-trajectory segment or the final kernel) */
int mpdx_unet_unit_layer(const mpdx_unet* u, int B, int i);
/* introspection: the kernel that runs fused segment `seg` of this network - 0..6: a static whole-trajectory program (0, 3, 5, 6 with
 * compile-time LDS geometry, csrc/fused_geom.hpp; four levels: 5 + 3, three levels: 0 + 6 + 3), -1: the generic op-list kernel, -2: no such segment.  Replaces nothing in the reference. */
int mpdx_unet_fused_program(const mpdx_unet* u, int seg);
/* measurement helper: ALGORITHMIC bytes of launch unit i of a U-Net pass at batch B - its weights / parameters once plus the activations
 * that cross its boundary once (bench.py: roofline.traffic_over_algorithmic).  Replaces nothing in the reference. */
double mpdx_unet_unit_bytes(const mpdx_unet* u, int B, int i);
/* 1 when launch unit i is a paired launch (blocks[0] + the same block's residual 1x1 conv in one conv_pair_kernel) */
int mpdx_unet_unit_is_pair(const mpdx_unet* u, int B, int i);
/* `reps` back-to-back launches of layer `layer` between two events; dbg = ablation mask (1 skip staging, 2 skip
 * MFMA loop, 4 skip epilogue, 8 skip weight loads: -DMPDX_DEV_HOOKS builds only), 16 = replay from a hipGraph; synchronises. */
int mpdx_bench_layer(mpdx_unet* u, const float* packed_dev, const float* timetab_dev, const float* x, int layer, int B,
                     float* ws, void* stream, int reps, int dbg, float* ms_per_launch);
/* tile the dispatcher picks for launch i at batch B: writes "MTxNT/WNxWK" into buf */
int mpdx_unet_layer_tile(const mpdx_unet* u, int i, int B, char* buf, size_t buflen);
/* dev / test entry: ONE Residual(PreNorm(C, LinearAttention(C))) block (layers.py:174-226) outside a network, in place on x [B][L][C]
 * (channel-last; rows Lv..L-1 of each trajectory zero on entry and on return: a horizon of Lv positions in its power-of-two container L).
 * Parameters in state-dict layout: to_qkv.weight [384,C,1], to_out.weight [C,128,1], to_out.bias [C], norm.g / norm.b [1,C,1].  Runs what a
 * network runs (the same weight packing, layer description and launch); MPDX_E_INVALID, before any launch, for every (C, L) that
 * mpdx_unet_create refuses for a self-attention level.  Synchronises the stream. */
int mpdx_attention_block(float* x, const float* to_qkv_w, const float* to_out_w, const float* to_out_b, const float* norm_g, const float* norm_b,
                         int B, int L, int Lv, int C, void* stream);

/* ---- cost values and clearance per trajectory: the VALUES of the terms whose gradients mpdx_guide_step applies.  Replaces the forward half of
 * guides.py:190, cost(x, x_interpolated=..., return_invidual_costs_and_weights=True) -> ([B] per term, [weights]), for a composite compiled into
 * mpdx_guide_params (cost arithmetic un-vendored in the reference, restated from the published formulas: PARITY UNPINNED); the clearance replaces
 * nothing (the reference counts colliding waypoints).  One 64-lane workgroup per trajectory, sums and minima by a fixed butterfly (no atomics:
 * two calls on the same input give the same bits).  x_unnormalised [B,H,D] is in robot units, as for mpdx_traj_metrics: clip_grad, the normaliser
 * members and identity_normalizer are ignored.  The weights of the block (fields[f].weight, gp_weight, tool_weight) are NOT applied.
 * All in fp32, on the same device functions as mpdx_traj_metrics_mask (a negative clearance and a collision flag come from the same signed distance):
 *   1. the evaluated points: N = n_points (2 ... 8192), or for n_points == 0 what the block says (interpolate ? n_interp : H); point i is the guide's
 *      linear interpolation q_i = l0 x[i0] + l1 x[i1], u = i (H - 1) / (N - 1), i0 = (int)u, l1 = u - i0 (N == H: the supports themselves)
 *   2. the link spheres of q_i: the point itself with r = link_margin (point mass); the Panda's 11 spheres; the chain table's spheres (sinf / cosf)
 *   3. slot f < n_fields, cost_out[b][f] = sum over points and factors, with m = r + cutoff_margin:
 *        MPDX_FIELD_OBJECTS / MPDX_FIELD_GRID  one relu(m - sdf(p)) per sphere; a field with a track is tested at p - o_i, o_i = l0 track[i0] + l1 track[i1]
 *        MPDX_FIELD_WORKSPACE                  one relu(m - (p_j - ws_min_j)) and one relu(m - (ws_max_j - p_j)) per sphere and axis j < ws_dim
 *        MPDX_FIELD_SELF                       one relu(r_a + r_b - |P_a - P_b|) per pair (Panda: its 12 pairs; chain: the table's); point mass: none
 *      a slot at or beyond n_fields is 0
 *   4. slot MPDX_MAX_FIELDS, the GP prior over the SUPPORTS: with eq = q_{h+1} - q_h - dt v_h, ev = v_{h+1} - v_h,
 *        sum_{h < H-1} 12/dt^3 |eq|^2 - 12/dt^2 eq.ev + 4/dt |ev|^2, times 0.5 under gp_half_factor, divided by sigma_gp^2; 0 when use_gp == 0
 *   5. slot MPDX_MAX_FIELDS + 1, the tool axis (chain, tool_frame != 0; arithmetic of the tool members above): sum_i relu(tool_cos_min - tool_world .
 *      Rot_f(q_i) tool_axis); 0 when tool_frame == 0
 *   6. clearance_out[b][f] (or NULL) = min over points and factors of: sdf - r (objects, grid), face distance - r (workspace), |P_a - P_b| - (r_a +
 *      r_b) (self); +3.0e38 for a slot without factors
 *   7. point_out[b][i][f] (or NULL) = the factor sum of field f at point i alone, point_out[b][i][MPDX_MAX_FIELDS] that of the tool term (the GP prior
 *      has no points)
 * Checked on the host before any launch (MPDX_E_INVALID, the message names the argument): gp, x_unnormalised or cost_out NULL; B <= 0; D != 2 q_dim;
 * H < 2; n_points outside {0} and 2 ... 8192 (or, for 0, an n_interp outside it); the LDS need (state, staged tables, 64 x 49 floats of sphere centres for
 * the Panda and a chain) above 160 KB; everything mpdx_traj_metrics refuses in the block: a bad chain table ("chain: ..."), grid, scene and track members
 * (track_len != H), chain + grid, chain + track, track + scenes, and the checks of the tool members.
 * Takes: the point mass (ws_dim 2 and 3), the Panda, a chain of 1 ... 8 joints; every field kind; tracks (point mass, Panda); scenes (all three). */
#define MPDX_COST_SLOTS (MPDX_MAX_FIELDS + 2)   /* fields 0 ... 3 | GP prior | tool axis */
int mpdx_traj_costs(const mpdx_guide_params* gp, const float* x_unnormalised, float* cost_out /* [B][MPDX_COST_SLOTS] */,
                    float* clearance_out /* [B][MPDX_MAX_FIELDS] or NULL */, float* point_out /* [B][n_points][MPDX_MAX_FIELDS + 1] or NULL */,
                    int n_points, int B, int H, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPDX_H */
