// mpdx.hip - libmpdx.so: host-side layer plan, the launch units of a U-Net pass, the planning loop, the C ABI (include/mpdx.h) + the small streaming
// kernels.  Two host headers are this file's alone: fused_build.hpp (the whole-trajectory programs' descriptors), unet_measure.hpp (timing / trace entries).
//
// gfx950 only.  No CUDA shims, no dual paths.  All device memory is caller-owned; nothing here synchronises.
#include "host.hpp"
#include "attn.hpp"
#include "inner_run.hpp"
#include "loss.hpp"
#include "scene_table.hpp"
#include "motion.hpp"

namespace mpdx {

// ------------------------------------------------------------------------------------------------ error plumbing
static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) must be applied once per (device, kernel): guarded by a mutex and keyed by
// the current device, so that several host threads / several GPUs in one process are safe.
int raise_lds_limit(const void* kern) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kern})) return 0;
    HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done.insert({dev, kern});
    return 0;
}

static long long* g_conv_trace = nullptr;   // dev tool (mpdx_layer_trace)

// ------------------------------------------------------------------------------------------------ small kernels

// TimeEncoder (layers.py:229-255) and every ResidualTemporalBlock.cond_mlp (layers.py:336-340) depend only on the
// integer timestep: tabulate row t = [ cond_mlp_0(temb_t) | cond_mlp_1(temb_t) | ... ] once per model.
struct TimeTabArgs {
    const float* packed;
    const float* freqs;  // [16]
    float* tab;          // [T][row]
    int w1, b1, w2, b2;  // offsets of time_mlp.encoder.{1,3}.{weight,bias}
    int row;             // sum of C_out over blocks
    int nblk;
    int woff[40], boff[40], cout[40], toff[40];
};

__global__ __launch_bounds__(128) void timetab_kernel(const TimeTabArgs a) {
    __shared__ float emb[32], h1[128], te[32];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (tid < 16) {
        const float arg = (float)t * a.freqs[tid];  // x[:, None] * emb[None, :]  layers.py:252
        emb[tid] = sinf(arg);
        emb[tid + 16] = cosf(arg);
    }
    __syncthreads();
    {   // Linear(32,128) + Mish
        const float* w = a.packed + a.w1 + tid * 32;
        float s = a.packed[a.b1 + tid];
        for (int k = 0; k < 32; ++k) s = fmaf(w[k], emb[k], s);
        h1[tid] = mish(s);
    }
    __syncthreads();
    if (tid < 32) {  // Linear(128,32), then the Mish that opens every cond_mlp
        const float* w = a.packed + a.w2 + tid * 128;
        float s = a.packed[a.b2 + tid];
        for (int k = 0; k < 128; ++k) s = fmaf(w[k], h1[k], s);
        te[tid] = mish(s);
    }
    __syncthreads();
    for (int blk = 0; blk < a.nblk; ++blk) {
        for (int c = tid; c < a.cout[blk]; c += 128) {
            const float* w = a.packed + a.woff[blk] + c * 32;
            float s = a.packed[a.boff[blk] + c];
            for (int k = 0; k < 32; ++k) s = fmaf(w[k], te[k], s);
            a.tab[(size_t)t * a.row + a.toff[blk] + c] = s;
        }
    }
}


__global__ __launch_bounds__(256) void final_step_kernel(const FinalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* w = sm;                 // [D][C]
    float* bs = sm + a.D * a.C;    // [D]
    for (int i = threadIdx.x; i < a.D * a.C; i += blockDim.x) w[i] = a.w[i];
    for (int i = threadIdx.x; i < a.D; i += blockDim.x) bs[i] = a.bias[i];
    __syncthreads();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;  // b*H + l
    const bool live = p < a.B * a.H;
    const int b = live ? p / a.H : 0, l = live ? p - b * a.H : 0;
    float vmax = 0.f;
    if (live) {
        const float* hp = a.h + ((size_t)b * (a.Hc > 0 ? a.Hc : a.H) + l) * a.C;
        for (int d = 0; d < a.D; ++d) {
            float s = bs[d];
            for (int c = 0; c < a.C; c += 4) {
                const f32x4 hv = *(const f32x4*)(hp + c);
                const f32x4 wv = *(const f32x4*)(w + d * a.C + c);
                s = fmaf(hv[0], wv[0], s); s = fmaf(hv[1], wv[1], s);
                s = fmaf(hv[2], wv[2], s); s = fmaf(hv[3], wv[3], s);
            }
            const size_t o = (size_t)p * a.D + d;
            float r;
            if (a.mode == 0) {
                r = s;
            } else {
                const float xv = a.x_in[o];
                float x0;
                if (a.k.predict_epsilon)
                    x0 = __fsub_rn(__fmul_rn(a.k.sqrt_recip_alphas_cumprod, xv), __fmul_rn(a.k.sqrt_recipm1_alphas_cumprod, s));
                else
                    x0 = s;
                if (a.mode == 3) {  // ddim_sample (diffusion_model_base.py:216-237): x_start is not clamped there
                    const float pn = a.k.predict_epsilon
                                         ? s
                                         : __fdiv_rn(__fsub_rn(__fmul_rn(a.k.sqrt_recip_alphas_cumprod, xv), s), a.k.sqrt_recipm1_alphas_cumprod);
                    r = __fadd_rn(__fmul_rn(x0, a.k.ddim_k1), __fmul_rn(a.k.ddim_k2, pn));
                    if (a.hs && l == 0) r = a.hs[(size_t)b * a.D + d];
                    if (a.hg && l == a.H - 1) r = a.hg[(size_t)b * a.D + d];
                } else {
                    if (a.k.clip_denoised) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
                    r = __fadd_rn(__fmul_rn(a.k.posterior_mean_coef1, x0), __fmul_rn(a.k.posterior_mean_coef2, xv));
                    if (a.mode == 1) {
                        if (a.rng.on) r = __fadd_rn(r, __fmul_rn(__fmul_rn(a.k.noise_scale, philox_normal_at(a.rng.seed, a.rng.offset, a.rng.elem0 + o)), a.k.noise_std_extra));
                        else if (a.noise) r = __fadd_rn(r, __fmul_rn(__fmul_rn(a.k.noise_scale, a.noise[o]), a.k.noise_std_extra));
                        if (a.hs && l == 0) r = a.hs[(size_t)b * a.D + d];
                        if (a.hg && l == a.H - 1) r = a.hg[(size_t)b * a.D + d];
                    }
                }
            }
            a.out[o] = r;
            if (a.chain) a.chain[o] = r;
            vmax = fmaxf(vmax, fabsf(r));
        }
    }
    if (a.absmax) {
        // one wave == one trajectory when H == 64: reduce in-wave, one atomic per wave
        const int ctx = b / a.n_per_ctx;
        const int ctx0 = __builtin_amdgcn_readfirstlane(ctx);
        if (__all(ctx == ctx0)) {
            float m = vmax;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
            if ((threadIdx.x & 63) == 0) atomicMax(a.absmax + ctx0, __float_as_uint(m));
        } else if (live) {
            atomicMax(a.absmax + ctx, __float_as_uint(vmax));
        }
    }
}

__global__ __launch_bounds__(256) void add_noise_kernel(float* x, const float* noise, const float* hs, const float* hg,
                                                         float scale, float extra, float* chain, int B, int H, int D) {
    const size_t n = (size_t)B * H * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int d = i % D;
        const size_t p = i / D;
        const int l = p % H;
        const size_t b = p / H;
        float r = x[i];
        if (noise) r = __fadd_rn(r, __fmul_rn(__fmul_rn(scale, noise[i]), extra));
        if (hs && l == 0) r = hs[b * D + d];
        if (hg && l == H - 1) r = hg[b * D + d];
        x[i] = r;
        if (chain) chain[i] = r;
    }
}

// apply_hard_conditioning (sample_functions.py:5-8) for ARBITRARY horizon indices: x[:, idx[k], :] = vals[k][:, :] for k < n, in the dict's
// order (a later entry wins on a repeated index, as successive indexed writes do).  One thread per (entry, trajectory, dimension).
constexpr int kMaxHardConds = 16;
struct HardCondArgs { int idx[kMaxHardConds]; const float* vals[kMaxHardConds]; int n; };
__global__ __launch_bounds__(256) void hard_conds_kernel(float* x, float* chain, const HardCondArgs a, int B, int H, int D) {
    const size_t per = (size_t)B * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / D;
        const int d = (int)(i - b * D);
        for (int k = 0; k < a.n; ++k) {   // in order: every thread owns its (b, d) column of all entries, so a repeated index resolves as in the reference
            const float v = a.vals[k][i];
            const size_t o = (b * H + a.idx[k]) * D + d;
            x[o] = v;
            if (chain) chain[o] = v;
        }
    }
}

// q_sample (diffusion_model_base.py:320-330) + apply_hard_conditioning (:335): per-trajectory timestep, schedule rows
// looked up on the device.  x_t = sqrt(acp[t_b]) * x0 + sqrt(1 - acp[t_b]) * noise
__global__ __launch_bounds__(256) void q_sample_kernel(const float* x0, const float* noise, const long long* t, const float* sqrt_ac,
                                                        const float* sqrt_1mac, const float* hs, const float* hg, float* out, int B, int H,
                                                        int D, int T) {
    const size_t n = (size_t)B * H * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int d = i % D;
        const size_t p = i / D;
        const int l = p % H;
        const size_t b = p / H;
        long long tb = t[b];
        tb = tb < 0 ? 0 : (tb >= T ? T - 1 : tb);
        float r = __fadd_rn(__fmul_rn(sqrt_ac[tb], x0[i]), __fmul_rn(sqrt_1mac[tb], noise[i]));
        if (hs && l == 0) r = hs[b * D + d];
        if (hg && l == H - 1) r = hg[b * D + d];
        out[i] = r;
    }
}

// WeightedL1 / WeightedL2 (helpers.py:71-99) of apply_hard_conditioning(pred) against targ: mean over all B*H*D elements
// of |.| or (.)^2, optionally times weights[H*D].  One workgroup, fixed summation order (deterministic); validation-sized
// inputs (B*H*D ~ 1e5 - 1e7).
__global__ __launch_bounds__(1024) void weighted_loss_kernel(const float* pred, const float* targ, const float* weights, const float* hs,
                                                             const float* hg, int l1, float* out, int B, int H, int D) {
    __shared__ double part[16];
    weighted_loss_body(pred, targ, weights, hs, hg, l1, out, B, H, D, part);
}

// standard-normal generator (Philox4x32-10 + Box-Muller, conv_block.hpp): 4 normals per counter.
__global__ __launch_bounds__(256) void randn_kernel(float* out, size_t n, uint64_t seed, uint64_t offset) {
    const size_t nquad = (n + 3) / 4;
    for (size_t qd = (size_t)blockIdx.x * blockDim.x + threadIdx.x; qd < nquad; qd += (size_t)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal4(seed, qd + offset, z);
        const size_t base = qd * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (base + e < n) out[base + e] = z[e];
    }
}

// network input [B][H][D] -> container [B][Hc][D] with zero rows behind the H real ones (horizons that are not powers of two)
__global__ __launch_bounds__(256) void pad_input_kernel(const float* __restrict__ x, float* __restrict__ xc, int B, int H, int Hc, int D) {
    const size_t n = (size_t)B * Hc * D;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const size_t p = i / D;
        const int l = (int)(p % Hc);
        const size_t b = p / Hc;
        xc[i] = l < H ? x[(b * H + l) * D + d] : 0.f;
    }
}

__global__ void copy_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------
// weight repacking: reference layout -> MFMA A-fragment order  Wp[m16][c16][slot][lane][4]
//   conv:   src [C_out][C_in][k]        (nn.Conv1d)
//   convT:  src [C_in][C_out][k]        (nn.ConvTranspose1d)
__global__ void pack_conv_weights_kernel(const float* __restrict__ src, float* __restrict__ dst, int C_out, int C_in,
                                         int ksz, int cin_pad, int nslot, int transposed) {
    const int nc16 = cin_pad >> 4;
    const size_t total = (size_t)(C_out >> 4) * nc16 * nslot * 256;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i & 3, lane = (i >> 2) & 63;
        size_t r = i >> 8;
        const int slot = r % nslot; r /= nslot;
        const int c16 = r % nc16; const int m16 = r / nc16;
        const int co = m16 * 16 + (lane & 15);
        const int ci = c16 * 16 + (lane >> 4) * 4 + e;
        float v = 0.f;
        if (ci < C_in) {
            if (transposed) v = src[((size_t)ci * C_out + co) * ksz + upt_slot_to_k(slot)];
            else v = src[((size_t)co * C_in + ci) * ksz + slot];
        }
        dst[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host-side model

static int gn_groups(int c) {  // layers.py:389-395
    if (c < 8) return 1;
    for (int g = 8; g < 18; ++g)
        if (c % g == 0) return g;
    return 1;
}

// input channels as the kernels see them: a multiple of 16 (one MFMA k-group) that is also a power of two (channel indices are shifts) - 33 ... 48
// real channels run in a 64-channel container whose extra channels are zero in the staged input AND in the packed weights
static int pad_cin(int c) {
    int p = (c + 15) / 16 * 16;
    while (p & (p - 1)) p += 16;
    return p;
}

static int add_param(mpdx_unet* u, const std::string& name, std::initializer_list<int> shape, int kind = PK_VEC) {
    Param p;
    p.name = name;
    p.ndim = (int)shape.size();
    p.n = 1;
    int i = 0;
    for (int s : shape) { p.shape[i++] = s; p.n *= (size_t)s; }
    p.kind = kind;
    if (kind == PK_CONV) {
        p.cout = p.shape[0]; p.cin = p.shape[1]; p.ksz = p.shape[2];
        p.nslot = p.ksz;
    } else if (kind == PK_CONVT) {
        p.cin = p.shape[0]; p.cout = p.shape[1]; p.ksz = p.shape[2];
        p.nslot = 4;
    }
    if (kind != PK_VEC) {
        p.cin_pad = pad_cin(p.cin);
        p.pn = (size_t)(p.cout / 16) * (p.cin_pad / 16) * p.nslot * 256;
    } else {
        p.pn = (p.n + 3) / 4 * 4;
    }
    p.off = u->packed_floats;
    u->packed_floats += p.pn;
    u->pidx[name] = (int)u->params.size();
    u->params.push_back(p);
    return (int)u->params.size() - 1;
}

// LDS row stride (floats) for the staged window: smallest pad that minimises ds_read_b128 bank conflicts of the
// B-fragment gather (lane (j,q) reads 16 B at row(j)*rs + 4q; ds_read_b128 is served in the four 16-lane groups
// listed in MI355X_MICROARCH.md section LDS; bank = dword address mod 64).
int pick_row_stride(int cin_pad, int mode, int L_in, int L_out, int LP) {
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int best_rs = cin_pad, best = 1 << 30;
    for (int pad = 0; pad <= 64; pad += 4) {
        const int rs = cin_pad + pad;
        int score = 0;
        for (int g = 0; g < 4; ++g) {
            int cnt[16] = {0};
            int worst = 0;
            for (int i = 0; i < 16; ++i) {
                const int lane = groups[g][i], j = lane & 15, q = lane >> 4;
                int row;
                if (mode == CONV_UPT) { const int s = j / L_in, m = j % L_in; row = s * LP + m; }
                else { const int s = j / L_out, l = j % L_out; row = s * LP + (mode == CONV_DOWN ? 2 * l : l); }
                const int slot16 = ((row * rs + q * 4) & 63) >> 2;
                worst = std::max(worst, ++cnt[slot16]);
            }
            score += worst;
        }
        if (score < best) { best = score; best_rs = rs; }
        if (best == 4) break;
    }
    return best_rs;
}

static void build_model(mpdx_unet* u) {
    const mpdx_unet_cfg& c = u->cfg;
    const int nl = c.n_levels, D = c.state_dim, te = c.time_emb_dim;
    const int Hv = c.n_support_points;   // the horizon; H below = its power-of-two container (== Hv for 16 / 32 / 64 / 128)
    int H = 1;
    while (H < Hv) H <<= 1;
    u->Hc = H;
    std::vector<int> dims(nl + 1);
    dims[0] = D;
    for (int i = 0; i < nl; ++i) dims[i + 1] = c.unet_input_dim * c.dim_mults[i];

    add_param(u, "time_mlp.encoder.1.weight", {128, 32});
    add_param(u, "time_mlp.encoder.1.bias", {128});
    add_param(u, "time_mlp.encoder.3.weight", {te, 128});
    add_param(u, "time_mlp.encoder.3.bias", {te});

    const int P0 = 0, P1 = 1, HB = 2, RB = 3, S0 = 4;
    u->n_slots = S0 + nl;
    auto other = [&](int s) { return s == P0 ? P1 : P0; };
    size_t slot = 0;

    auto conv_layer = [&](const std::string& wname, const std::string& bname, int mode, int ks, int epi, int src1, int c1,
                          int src2, int c2, int cout, int L_in, int L_out, int dst) -> Layer& {
        Layer l;
        l.name = wname; l.mode = mode; l.ks = ks; l.epi = epi;
        l.src1 = src1; l.c1 = c1; l.src2 = src2; l.c2 = c2; l.cout = cout; l.L_in = L_in; l.L_out = L_out; l.dst = dst;
        l.Lv_out = (H != Hv) ? (int)((long)L_out * Hv / H) : 0;   // (levels halve container and horizon alike: Hv % 2^(levels-1) == 0)
        l.pin_nt = c.self_attention != 0;
        if (mode == CONV_UPT) l.w = add_param(u, wname, {c1 + c2, cout, ks}, PK_CONVT);
        else l.w = add_param(u, wname, {cout, c1 + c2, ks}, PK_CONV);
        l.b = add_param(u, bname, {cout});
        l.cin_pad = pad_cin(c1 + c2);
        const int pad = (mode == CONV_S1) ? ks / 2 : 1;
        l.rs = pick_row_stride(l.cin_pad, mode, L_in, L_out, L_in + 2 * pad);
        slot = std::max(slot, (size_t)cout * L_out);
        u->layers.push_back(l);
        return u->layers.back();
    };
    auto cblock = [&](const std::string& p, int src1, int c1, int src2, int c2, int cout, int L, int dst) -> Layer& {
        Layer& l = conv_layer(p + ".block.0.weight", p + ".block.0.bias", CONV_S1, 5, EPI_GN_MISH, src1, c1, src2, c2, cout, L, L, dst);
        const int idx = (int)u->layers.size() - 1;
        const int ga = add_param(u, p + ".block.2.weight", {cout});
        const int be = add_param(u, p + ".block.2.bias", {cout});
        Layer& ll = u->layers[idx];
        ll.gamma = ga; ll.beta = be;
        ll.gs = cout / gn_groups(cout);
        (void)l;
        return ll;
    };
    auto rtb = [&](const std::string& p, int src1, int c1, int src2, int c2, int cout, int L, int dst) {
        {
            Layer& b0 = cblock(p + ".blocks.0", src1, c1, src2, c2, cout, L, HB);
            b0.tb_off = u->tt_row;
        }
        const int i1 = (int)u->layers.size();
        cblock(p + ".blocks.1", HB, cout, SRC_NONE, 0, cout, L, dst);
        const int tw = add_param(u, p + ".cond_mlp.1.weight", {cout, te});
        const int tbp = add_param(u, p + ".cond_mlp.1.bias", {cout});
        u->tt_w.push_back(tw); u->tt_b.push_back(tbp); u->tt_cout.push_back(cout); u->tt_off.push_back(u->tt_row);
        u->tt_row += cout;
        int res = src1;
        if (c1 + c2 != cout) {
            // residual 1x1 conv runs BEFORE blocks.1 in launch order: insert it ahead of that layer
            Layer keep = u->layers[i1];
            u->layers.pop_back();
            conv_layer(p + ".residual_conv.weight", p + ".residual_conv.bias", CONV_S1, 1, EPI_BIAS, src1, c1, src2, c2, cout, L, L, RB);
            u->layers.push_back(keep);
            res = RB;
        }
        u->layers.back().res = res;
    };

    // Residual(PreNorm(dim, LinearAttention(dim))) (temporal_unet.py:82,93,104; layers.py:174-226) in place on `slot_id`: one launch (attn.hpp).
    // to_qkv / to_out are 1x1 convolutions: packed into the A-fragment order of the convolutions, one tap
    auto attention = [&](const std::string& p, int slot_id, int C, int Lc) {
        if (!c.self_attention) return;
        Layer l;
        l.name = p + ".fn.fn.to_qkv.weight"; l.attn = true; l.mode = CONV_S1; l.ks = 0; l.epi = EPI_BIAS;
        l.src1 = slot_id; l.dst = slot_id; l.c1 = C; l.cout = C; l.L_in = Lc; l.L_out = Lc;
        l.Lv_out = (H != Hv) ? (int)((long)Lc * Hv / H) : 0;
        l.w = add_param(u, p + ".fn.fn.to_qkv.weight", {3 * kAttnHid, C, 1}, PK_CONV);
        l.w2 = add_param(u, p + ".fn.fn.to_out.weight", {C, kAttnHid, 1}, PK_CONV);
        l.b2 = add_param(u, p + ".fn.fn.to_out.bias", {C});
        l.gamma = add_param(u, p + ".fn.norm.g", {1, C, 1});
        l.beta = add_param(u, p + ".fn.norm.b", {1, C, 1});
        l.cin_pad = pad_cin(C);
        l.rs = pick_row_stride(l.cin_pad, CONV_S1, Lc, Lc, Lc);
        u->layers.push_back(l);
    };

    int L = H, cur = SRC_X, curC = D;
    for (int i = 0; i < nl; ++i) {
        const int co = dims[i + 1];
        const std::string p = "downs." + std::to_string(i);
        const int a = other(cur);
        rtb(p + ".0", cur, curC, SRC_NONE, 0, co, L, a);
        rtb(p + ".1", a, co, SRC_NONE, 0, co, L, S0 + i);
        attention(p + ".2", S0 + i, co, L);   // (the skip tensor the level pushes is the block's output: temporal_unet.py:146-149)
        cur = S0 + i; curC = co;
        if (i < nl - 1) {
            conv_layer(p + ".4.conv.weight", p + ".4.conv.bias", CONV_DOWN, 3, EPI_BIAS, cur, co, SRC_NONE, 0, co, L, L / 2, P0);
            cur = P0; L /= 2;
        }
    }
    rtb("mid_block1", cur, curC, SRC_NONE, 0, curC, L, P0);
    attention("mid_attn", P0, curC, L);
    rtb("mid_block2", P0, curC, SRC_NONE, 0, curC, L, P1);
    cur = P1;
    for (int j = 0; j < nl - 1; ++j) {
        const int lv = nl - 1 - j;            // level whose skip is popped
        const int dout = dims[lv + 1], din = dims[lv];
        const std::string p = "ups." + std::to_string(j);
        const int a = other(cur);
        rtb(p + ".0", cur, dout, S0 + lv, dout, din, L, a);
        const int b = other(a);
        rtb(p + ".1", a, din, SRC_NONE, 0, din, L, b);
        attention(p + ".2", b, din, L);
        const int d = other(b);
        conv_layer(p + ".4.conv.weight", p + ".4.conv.bias", CONV_UPT, 4, EPI_BIAS, b, din, SRC_NONE, 0, din, L, 2 * L, d);
        cur = d; L *= 2; curC = din;
    }
    cblock("final_conv.0", cur, curC, SRC_NONE, 0, c.unet_input_dim, L, HB);
    u->final_slot = HB;
    add_param(u, "final_conv.1.weight", {D, c.unet_input_dim, 1});
    add_param(u, "final_conv.1.bias", {D});
    u->slot_floats = std::max(slot, (size_t)c.unet_input_dim * H);
    if (H != Hv) u->xpad_slot = u->n_slots++;   // one more workspace slot: the padded copy of the network input
}

}  // namespace mpdx

#include "fused_build.hpp"   // build_units: which layer ranges run as whole-trajectory programs, and their descriptors

namespace mpdx {

// tile choice.  Measured on MI355X at B=100 (tools/ablate_layers.py): per-launch time is dominated by fixed costs
// (launch boundary ~3 us, epilogue ~1.9 us), halving the tile to co-schedule two workgroups per CU does NOT pay
// (the MFMA phase gets slower: every output column re-streams the weights), so: the largest tile that still
// gives >= `target` workgroups (default 160 of the 256 CUs), growing with the batch for weight reuse.
// MPDX_TILE=MTxNT / MPDX_TARGET_WGS override (development).
void choose_tile(const Layer& l, int B, int& MT, int& NT) {
    const int min_mt = (l.epi == EPI_GN_MISH && l.gs > 16) ? 32 : 16;
    const int min_nt = std::max(l.mode == CONV_UPT ? 32 : 16, l.L_out);
    const long npos = (long)B * l.L_out;
    if (const char* ov = sw::tile()) {
        int mt = 0, nt = 0;
        if (sscanf(ov, "%dx%d", &mt, &nt) == 2 && mt >= min_mt && nt >= min_nt && l.cout % mt == 0 && nt % l.L_out == 0) { MT = mt; NT = nt; return; }
    }
    if (min_nt > 64) {   // a level with more than 64 positions (n_support_points = 128): one trajectory per tile
        NT = min_nt;
        MT = (min_mt <= 16 && l.cout % 16 == 0) ? 16 : 32;
        return;
    }
    const int target = std::max(1, sw::target_wgs());
    auto wgs = [&](int mt, int nt) { return (long)(l.cout / mt) * ((npos + nt - 1) / nt); };
    const int pad = (l.mode == CONV_S1) ? l.ks / 2 : 1;
    auto lds = [&](int mt, int nt) {  // max(staged windows, K-partial buffer), as conv_block_lds_bytes
        const size_t stage = (size_t)(nt / l.L_out) * (l.L_in + 2 * pad) * l.rs * sizeof(float);
        const size_t red = (size_t)8 * nt * (mt + 4) * sizeof(float);
        return std::max(stage, red);
    };
    const int mts[2] = {32, 16}, nts[3] = {64, 32, 16};
    if (l.pin_nt && !layer_ksplit(l)) {   // (Layer::pin_nt) the narrowest legal width at every batch; the channel tile by the usual rule
        NT = min_nt;
        for (int mt : mts)
            if (mt >= min_mt && l.cout % mt == 0 && lds(mt, NT) <= (size_t)sw::lds_cap_kb() * 1024 && wgs(mt, NT) >= target) { MT = mt; return; }
        MT = (min_mt <= 16 && l.cout % 16 == 0) ? 16 : 32;
        return;
    }
    // largest tile that fits LDS (<= 96 KiB so that a second workgroup can co-reside; MPDX_LDS_CAP_KB overrides) and still
    // yields >= target workgroups; else the smallest legal tile
    const size_t cap = (size_t)sw::lds_cap_kb() * 1024;
    for (int nt : nts)
        for (int mt : mts) {
            if (mt < min_mt || nt < min_nt || l.cout % mt || lds(mt, nt) > cap) continue;
            if (wgs(mt, nt) >= target) { MT = mt; NT = nt; return; }
        }
    MT = (min_mt <= 16 && l.cout % 16 == 0) ? 16 : 32;
    NT = min_nt;
}

static int layer_ntap(const Layer& l) { return l.mode == CONV_UPT ? 2 : l.ks; }
bool layer_ksplit(const Layer& l) {
    if (!(l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH)) return true;
    if (const int forced = sw::ksplit(); forced >= 0) return forced != 0;
    return (l.cin_pad / 16) * layer_ntap(l) >= 16;  // enough K to feed 8 K-split waves
}
static double layer_flops(const Layer& l, int B) {
    // attention block: to_qkv 2 * 384 * C + to_out 2 * C * 128 = 1024 C per position, context and out 2 * 2 * 32 * 32 per head and position = 16384
    if (l.attn) return (double)B * l.L_out * (1024.0 * l.cout + 16384.0);
    return 2.0 * l.cout * (double)B * l.L_out * (l.c1 + l.c2) * layer_ntap(l);
}


static int make_conv_args(const mpdx_unet* u, const Layer& l, const float* packed, const float* tt_row, const float* x, float* ws, int B,
                          int dbg, ConvArgs& a) {
    const size_t slot = u->slot_floats * (size_t)B;
    auto src = [&](int s) -> const float* { return s == SRC_X ? x : (s == SRC_NONE ? nullptr : ws + slot * s); };
    memset(&a, 0, sizeof(a));
    a.src1 = src(l.src1); a.src2 = src(l.src2);
    a.c1 = l.c1; a.c2 = l.c2;
    a.wp = packed + u->params[l.w].off;
    a.bias = packed + u->params[l.b].off;
    a.gamma = l.gamma >= 0 ? packed + u->params[l.gamma].off : nullptr;
    a.beta = l.beta >= 0 ? packed + u->params[l.beta].off : nullptr;
    a.tbias = (l.tb_off >= 0 && tt_row) ? tt_row + l.tb_off : nullptr;
    a.res = src(l.res);
    a.dst = ws + slot * l.dst;
    a.B = B; a.L_in = l.L_in; a.L_out = l.L_out; a.C_out = l.cout;
    a.cin_pad = l.cin_pad; a.rs = l.rs; a.gs = l.gs; a.dbg = dbg;
    a.Lv_out = l.Lv_out;
    a.trace = g_conv_trace;
    auto lg2 = [](int v) { int k = 0; while ((1 << k) < v) ++k; return k; };
    a.lg_c4n = lg2(l.cin_pad / 4); a.lg_Lin = lg2(l.L_in); a.lg_Lout = lg2(l.L_out); a.lg_gs = l.gs > 0 ? lg2(l.gs) : 0;
    if ((1 << a.lg_c4n) != l.cin_pad / 4 || (1 << a.lg_Lin) != l.L_in || (1 << a.lg_Lout) != l.L_out || (l.gs > 0 && (1 << a.lg_gs) != l.gs))
        return fail(MPDX_E_INVALID, "layer %s: channel/length/group sizes must be powers of two", l.name.c_str());
    return 0;
}

// Large batches: the Conv1dBlocks of the inner levels (L = 8) run on the weight-stationary persistent kernels (conv_ws.hpp;
// bit-identical outputs).  From 8 position tiles per workgroup on (B >= 512 at L = 8); MPDX_WS=0 switches them off (read per call: A/B
// runs and the bit-identity test flip it inside one process).  Returns the variant: 0 none, 1 <16,32> (256 -> 256); with a paired
// residual 1x1 conv l2: 3 <32,16,R1> (512 -> 128 on a channel concat).  Measured and NOT used (rocprofv3, B = 6400, us per launch,
// weight-stationary vs per-layer kernels): 128 -> 128 <8,16>: 142.7 vs 95.9; 128 -> 256 + 1x1 <8,32,R1>: 268 vs 234 - with 5 k-groups per
// wave a tile's 20-40 MFMAs per wave do not cover its barrier and window hand-over; kept: 256 -> 256: 319 vs 332, 512 -> 128 + 1x1: 387 vs 468.
static int weight_stationary_variant(const Layer& l, const Layer* l2, const ConvArgs& a, int B, int dbg) {
    const int ws_env = sw::ws();   // 0: off, 2: single layers only
    // conv_wsn / conv_wsp load a wave's WHOLE weight slice in their prologue (40-48 KB per wave, ~10 us per launch): they pay from a few tiles per
    // wave on - batch thresholds (512, MPDX_WSN_MIN_B / MPDX_WSP_MIN_B) from tools/wsn_threshold_sweep.py (profiles/r05_wsn_threshold_sweep.txt)
    const int wsn_min_b = sw::wsn_min_b(), wsp_min_b = sw::wsp_min_b();
    const bool wsn_on = sw::wsn() && ws_env != 0 && B >= wsn_min_b;
    const bool wsp_on = ws_env != 0 && B >= wsp_min_b && sw::wsp();
    // Upsample1d(128) of the innermost up level, 8 -> 16 positions: conv_wsn_kernel<CONV_UPT> (round 5)
    if (l.mode == CONV_UPT && l.ks == 4 && l.epi == EPI_BIAS && !l2 && l.L_in == 8 && l.L_out == 16 && !l.Lv_out && l.c1 == 128 && l.c2 == 0 &&
        l.cin_pad == 128 && l.cout == 128 && !dbg && !a.pre && !a.accum && !a.dst2 && wsn_on && (long)B * 8 >= 16L * kWsGroups * 8)
        return 5;
    if (!(l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH && l.L_out == 8 && l.L_in == 8) || l.Lv_out) return 0;
    if (dbg || a.pre || (l.c1 & 3) || (l.c2 & 3) || l.cin_pad != l.c1 + l.c2) return 0;
    if ((long)B * l.L_out < 16L * kWsGroups * 8) return 0;
    if (ws_env == 0 || (l2 && ws_env == 2)) return 0;
    if (l2) {
        if (!(l2->mode == CONV_S1 && l2->ks == 1 && l2->epi == EPI_BIAS && l2->cout == l.cout && l2->L_out == 8 && l2->c1 == l.c1 && l2->c2 == l.c2)) return 0;
        if (l.cout == 128 && l.gs == 16 && l.cin_pad == 512) return 3;
        if (l.cout == 256 && l.gs == 32 && l.cin_pad == 128 && l.c2 == 0 && wsp_on && !a.res)
            return 6;   // conv_wsp_kernel: 128 -> 256 k5 + 1x1, a pair of waves per tile, whole K per wave (round 5)
        return 0;
    }
    if (l.cout == 256 && l.gs == 32 && l.cin_pad == 256) return 1;
    if (l.cout == 128 && l.gs == 16 && l.cin_pad == 128 && l.c2 == 0 && wsn_on) return 4;   // conv_wsn_kernel<CONV_S1>: no K split (round 5)
    return 0;
}


static int run_layer(const mpdx_unet* u, const Layer& l, const float* packed, const float* tt_row, const float* x,
                     float* ws, int B, hipStream_t st, int dbg = 0) {
    if (l.attn) {
        AttnArgs aa;
        memset(&aa, 0, sizeof(aa));
        aa.x = ws + u->slot_floats * (size_t)B * l.dst;
        aa.wqkv = packed + u->params[l.w].off; aa.wout = packed + u->params[l.w2].off; aa.bout = packed + u->params[l.b2].off;
        aa.g = packed + u->params[l.gamma].off; aa.b = packed + u->params[l.beta].off;
        return launch_attention(l, aa, B, st);
    }
    ConvArgs a;
    if (int rc = make_conv_args(u, l, packed, tt_row, x, ws, B, dbg, a)) return rc;
    if (const int v = weight_stationary_variant(l, nullptr, a, B, dbg)) return launch_weight_stationary(v, l, a, a, B, st);
    return launch_conv_layer(l, a, B, st);
}

// blocks[0] + residual 1x1 conv of one ResidualTemporalBlock qualify for ONE launch (conv_pair_kernel)?  On success the tile.
bool pair_tile(const Layer& l1, const Layer& l2, int B, int& MT, int& NT) {
    if (!sw::pair()) return false;
    if (!(l1.mode == CONV_S1 && l1.ks == 5 && l1.epi == EPI_GN_MISH && l2.mode == CONV_S1 && l2.ks == 1 && l2.epi == EPI_BIAS)) return false;
    if ((l1.gs * l1.L_out != 128 && l1.gs * l1.L_out != 256) || l1.Lv_out) return false;   // general / masked GroupNorm regions: no paired instantiations
    if (l1.src1 != l2.src1 || l1.src2 != l2.src2 || l1.cout != l2.cout || l1.L_out != l2.L_out || !layer_ksplit(l1)) return false;
    choose_tile(l1, B, MT, NT);   // the k5 block decides the tile; the 1x1 conv has no constraint beyond it
    if (l1.cout % MT) MT = 16;
    if (l1.cout % MT || NT % l1.L_out) return false;
    const size_t lds = std::max({(size_t)(NT / l1.L_out) * (l1.L_in + 4) * l1.rs * sizeof(float), (size_t)(NT / l2.L_out) * l2.L_in * l2.rs * sizeof(float),
                                 (size_t)8 * NT * (MT + 4) * sizeof(float)});   // as launch_pair computes it
    return lds <= 160 * 1024;
}

static int run_pair(const mpdx_unet* u, const Layer& l1, const Layer& l2, const float* packed, const float* tt_row, const float* x, float* ws,
                    int B, hipStream_t st) {
    int MT, NT;
    if (!pair_tile(l1, l2, B, MT, NT)) return fail(MPDX_E_STATE, "layers %s / %s do not pair", l1.name.c_str(), l2.name.c_str());
    ConvArgs a1, a2;
    if (int rc = make_conv_args(u, l1, packed, tt_row, x, ws, B, 0, a1)) return rc;
    if (int rc = make_conv_args(u, l2, packed, tt_row, x, ws, B, 0, a2)) return rc;
    if (const int v = weight_stationary_variant(l1, &l2, a1, B, 0)) return launch_weight_stationary(v, l1, a1, a2, B, st);
    a1.n_tiles_n = a2.n_tiles_n = (int)(((long)B * l1.L_out + NT - 1) / NT);
    return launch_conv_pair(MT, NT, a1, a2, l1, l2, st) == 1 ? 0 : fail(MPDX_E_INVALID, "pair launch failed (tile %dx%d)", MT, NT);
}

int check_ready(const mpdx_unet* u) {
    if (u->n_done != (int)u->params.size())
        return fail(MPDX_E_STATE, "%d of %zu parameters packed; call mpdx_unet_pack_param for every state-dict tensor first",
                    u->n_done, u->params.size());
    return 0;
}

// bit k enables fused segment k.  Default: all segments at every batch size.  A fused program streams the segment's weights once
// per TRAJECTORY (from the L2, warm within a launch) where the per-layer kernels stream them once per tile of 4-8 trajectories and
// round-trip every activation through HBM; with the static programs (136-170 VGPRs: two workgroups per CU) the fused path wins
// everywhere.  Measured on MI355X: U-Net pass D=14, round-2 generic kernel: B=800 1.305 vs 1.337 ms (fused vs per-layer), 1600: 2.04 vs
// 2.16, 3200: 3.52 vs 3.57, 6400 equal; static programs at B=6400 (cfg5 plan): 644 vs 726 ms.  (Round 1's kernel crossed over at
// B~600.)  MPDX_FUSED=0/1 forces none/all, MPDX_FUSED_MASK=<bits> selects segments.
unsigned fused_mask(int B) {
    (void)B;
    return sw::fused() ? sw::fused_mask() : 0u;   // both live: tests and A/B runs switch the path inside one process
}
// launch units for batch B, one per program / pair / single layer (the form the timing entries and the unit queries index)
static std::vector<mpdx_unet::Unit> current_units(const mpdx_unet* u, int B, bool* final_in_fused) {
    std::vector<mpdx_unet::Unit> out;
    const unsigned m = fused_mask(B);
    bool fin = false;
    const int nlay = (int)u->layers.size();
    auto fused_on = [&](int i) { const int o = u->owner[i]; return o >= 0 && ((m >> o) & 1u); };
    for (int i = 0; i < nlay; ++i) {
        const int o = u->owner[i];
        if (fused_on(i)) {
            if (i == u->fused[o].first) { out.push_back({mpdx_unet::kProgram, o, i, u->fused[o].count}); fin |= u->fused[o].has_final; }
            continue;
        }
        int MT, NT;
        if (i + 1 < nlay && !fused_on(i + 1) && pair_tile(u->layers[i], u->layers[i + 1], B, MT, NT)) {
            out.push_back({mpdx_unet::kPair, -1, i, 2});   // blocks[0] followed by the same block's residual 1x1 conv: one launch
            ++i;
            continue;
        }
        out.push_back({mpdx_unet::kLayer, -1, i, 1});
    }
    if (final_in_fused) *final_in_fused = fin;
    return out;
}

static int run_final(mpdx_unet* u, const float* packed, FinalArgs& fa, int B, float* ws, hipStream_t st) {
    const mpdx_unet_cfg& c = u->cfg;
    fa.h = ws + u->slot_floats * (size_t)B * u->final_slot;
    fa.w = packed + u->params[u->pidx.at("final_conv.1.weight")].off;
    fa.bias = packed + u->params[u->pidx.at("final_conv.1.bias")].off;
    fa.B = B; fa.H = c.n_support_points; fa.D = c.state_dim; fa.C = c.unet_input_dim;
    fa.Hc = u->Hc;
    return launch_final_step(fa, st);
}
int launch_final_step(const FinalArgs& fa, hipStream_t st) {
    const int n = fa.B * fa.H;
    const size_t lds = (size_t)(fa.D * fa.C + fa.D) * sizeof(float);
    hipLaunchKernelGGL(final_step_kernel, dim3((n + 255) / 256), dim3(256), lds, st, fa);
    return 0;
}

static long long* g_fused_trace = nullptr;  // dev tool (mpdx_fused_trace)
static int g_fused_trace_seg = -1;

// all strided copies of every fused segment in ONE launch (blockIdx.y = job; the table lives in device memory; CopyJobDev, restream_job: train_types.hpp)
__global__ __launch_bounds__(256) void restream_all_kernel(float* __restrict__ packed, const CopyJobDev* __restrict__ jobs) {
    restream_job(packed, jobs[blockIdx.y], blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

static int ensure_stream_jobs(mpdx_unet* u) {
    if (!u->jobs_dev) {   // the job table never changes after build_units
        std::vector<CopyJobDev> all;
        for (const auto& f : u->fused)
            for (const auto& j : f.jobs) all.push_back({(unsigned long long)j.src, (unsigned long long)j.dst, j.n0, j.ss0, j.ds0, j.n1, j.ss1, j.ds1, j.n_inner});
        u->n_jobs = (int)all.size();
        if (u->n_jobs) {
            HIP_TRY(hipMalloc(&u->jobs_dev, all.size() * sizeof(CopyJobDev)));
            HIP_TRY(hipMemcpy(u->jobs_dev, all.data(), all.size() * sizeof(CopyJobDev), hipMemcpyHostToDevice));
        }
    }
    return 0;
}
// The fused segments read stream-ordered copies of their weights and one contiguous parameter block (fused_level.hpp);
// (re)assemble them in `packed` after the state dict was (re)packed.  Enqueues copies on `st`; no synchronisation.
int ensure_fused_streams(mpdx_unet* u, const float* packed, hipStream_t st) {
    if (u->streams_for == packed && u->streams_version == u->pack_version) return 0;
    if (int rc = ensure_stream_jobs(u)) return rc;
    if (u->n_jobs)
        hipLaunchKernelGGL(restream_all_kernel, dim3(64, (unsigned)u->n_jobs), dim3(256), 0, st, const_cast<float*>(packed), (const CopyJobDev*)u->jobs_dev);
    HIP_TRY(hipGetLastError());
    u->streams_for = packed; u->streams_version = u->pack_version;
    return 0;
}
// training: the caller runs the copies itself, as side blocks of its next launch (time_train_fwd_kernel) - hands out the device job table (null / 0:
// the streams are current) and marks the streams of `packed` current
int claim_fused_stream_jobs(mpdx_unet* u, const float* packed, const void** jobs, int* n) {
    *jobs = nullptr; *n = 0;
    if (u->streams_for == packed && u->streams_version == u->pack_version) return 0;
    if (int rc = ensure_stream_jobs(u)) return rc;
    *jobs = u->jobs_dev; *n = u->n_jobs;
    u->streams_for = packed; u->streams_version = u->pack_version;
    return 0;
}

// programs that exist in the training-forward variant (the two of the standard 4-level network, and the generic op-list kernel)
bool fused_save_variant(const mpdx_unet::Fused& f) { return f.program == 0 || f.program == 3 || f.program == 5 || f.program == 6 || f.program < 0; }
// the argument block of one launch of segment f
static int fill_fused_args(mpdx_unet* u, const mpdx_unet::Fused& f, const float* packed, const float* tt_row, const float* x, float* ws,
                           int B, const FinalArgs* fa, FusedArgs& a) {
    const size_t slot = u->slot_floats * (size_t)B;
    auto src = [&](int s) -> const float* { return s == SRC_X ? x : (s == SRC_NONE ? nullptr : ws + slot * s); };
    a = f.tmpl;
    a.packed = packed; a.tt_row = tt_row;
    a.gsrc1 = src(f.in1); a.gsrc2 = src(f.in2);
    a.gsrc3 = f.in3 != SRC_NONE ? src(f.in3) : a.gsrc1;
    for (int k = 0; k < 3; ++k) a.gout[k] = f.gout_slot[k] >= 0 ? ws + slot * f.gout_slot[k] : nullptr;
    a.B = B;
    a.trace = (g_fused_trace && (g_fused_trace_seg < 0 || g_fused_trace_seg == (int)(&f - &u->fused[0]))) ? g_fused_trace : nullptr;
    if (f.has_final) {
        if (!fa) return fail(MPDX_E_STATE, "fused final segment needs the step arguments");
        a.x_in = fa->x_in; a.noise = fa->noise; a.hs = fa->hs; a.hg = fa->hg; a.out = fa->out; a.chain = fa->chain;
        a.absmax = fa->absmax; a.fmode = fa->mode; a.n_per_ctx = fa->n_per_ctx > 0 ? fa->n_per_ctx : B; a.k = fa->k;
        a.rng = fa->rng;
    }
    return 0;
}
static int run_fused(mpdx_unet* u, const mpdx_unet::Fused& f, const float* packed, const float* tt_row, const float* x, float* ws,
                     int B, const FinalArgs* fa, hipStream_t st) {
    if (int rc = ensure_fused_streams(u, packed, st)) return rc;
    FusedArgs a;
    if (int rc = fill_fused_args(u, f, packed, tt_row, x, ws, B, fa, a)) return rc;
    return launch_fused_args(f, a, B, st);
}
// ---- the device state of the inner-level run (mpdx_unet::InnerRunState, host.hpp)
// Workgroups of a run launch of `width` that are resident at once on `cus` compute units, given the occupancy answer for that instantiation: the
// wide form stays at one workgroup per compute unit (the batches the per-layer tiles were measured at), the narrow form takes up to two.
static int run_index(int width) { return width == kRunNarrow ? 1 : 0; }
static int inner_run_resident(int cus, int width, int wgs_per_cu) { return cus * std::min(width == kRunNarrow ? 2 : 1, wgs_per_cu); }
// Counter lines of one width: the largest cluster count an admitted (B, width) gives - an admitted grid is whole groups of 8 clusters x 8 workgroups
// and at most inner_run_resident() workgroups - plus the 8 lines of slack the area always had (40 lines at width 32, 72 at width 16 on 256 CUs).
static int inner_run_counter_lines(int cus, int width) { return inner_run_resident(cus, width, 2) / 8 + 8; }
static size_t inner_run_counter_bytes(int cus, int width) { return (size_t)inner_run_counter_lines(cus, width) * kInnerRunCounterStride * sizeof(unsigned); }
// One occupancy query per run kernel and width, then the cluster counters (one area per width) and the host-mapped status word.  A device that cannot
// be asked leaves capacity 0: no run on this handle.
static int inner_run_create(mpdx_unet::InnerRunState& r, int cus) {
    if (r.capacity >= 0) return 0;
    r.capacity = 0;
    int dev = 0, khz = 0;
    if (cus <= 0 || hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev) != hipSuccess)
        return (void)hipGetLastError(), 0;
    bool any = false;
    for (int width : {kRunWide, kRunNarrow}) {
        r.seven_wgs[run_index(width)] = inner_run_workgroups_per_cu(width);
        r.tail_wgs[run_index(width)] = tail_run_workgroups_per_cu(width);
        any = any || r.seven_wgs[run_index(width)] > 0 || r.tail_wgs[run_index(width)] > 0;
    }
    if (!any) return 0;
    const size_t bytes = inner_run_counter_bytes(cus, kRunWide) + inner_run_counter_bytes(cus, kRunNarrow);
    HIP_TRY(hipMalloc((void**)&r.counters, bytes));
    HIP_TRY(hipMemset(r.counters, 0, bytes));
    r.ctr[0].p = r.counters;
    r.ctr[1].p = r.counters + inner_run_counter_lines(cus, kRunWide) * kInnerRunCounterStride;
    HIP_TRY(hipHostMalloc((void**)&r.status, 64, hipHostMallocMapped));
    *r.status = r.status_host;
    HIP_TRY(hipHostGetDevicePointer((void**)&r.status_dev, r.status, 0));
    r.budget = 4LL * (khz > 0 ? khz : 2400000);   // 4 ms of shader-clock ticks (s_memtime); a lower actual clock only lengthens it
    r.capacity = cus;
    return 0;
}
// A launch of nc clusters of `width` starts.  It advances the counters of ITS clusters only, so a launch with more clusters than the launch of that
// width before (a larger batch; a give-up's poison likewise) zeroes that width's counters, stream-ordered, and starts from base 0 again: at most once
// per plan and width.  Layer i > 0 waits for *base_out + 8 i: 8 arrivals per layer.
// The handle's runs of one width share its counters: each launch of n_layers layers leaves its clusters' counters at its base + 8 n_layers, the base of
// the next launch of either kind at that width (launches of one plan are stream-ordered and cover the same clusters).  A change of width between plans
// - or between the two runs of one plan - changes the area, not the rule.
static int inner_run_begin(mpdx_unet::InnerRunState& r, int width, int nc, int n_layers, hipStream_t st, unsigned** counters_out, unsigned* base_out) {
    mpdx_unet::InnerRunState::Counters& k = r.ctr[run_index(width)];
    if (nc > inner_run_counter_lines(r.capacity, width)) return fail(MPDX_E_STATE, "run of width %d: %d clusters, %d counter lines", width, nc, inner_run_counter_lines(r.capacity, width));
    if (k.rezero || nc > k.live) {
        HIP_TRY(hipMemsetAsync(k.p, 0, inner_run_counter_bytes(r.capacity, width), st));
        k.base = 0; k.rezero = false;
    }
    k.live = nc;
    *counters_out = k.p;
    *base_out = k.base;
    k.base += 8u * (unsigned)n_layers;
    return 0;
}
static void inner_run_free(mpdx_unet::InnerRunState& r) {
    if (r.counters) (void)hipFree(r.counters);
    if (r.status) (void)hipHostFree(r.status);
}
static int handle_status_error(const mpdx_unet* u, const char* fn) {
    const unsigned w = u->run.status_word();
    if (!w) return 0;
    return fail(MPDX_E_DEVICE, "%s: a workgroup of an inner-level run or of the paired joined launch gave up its wait (status 0x%x: layer %u of the run, or down op %u of the paired launch); the outputs of that plan hold NaN. "
                "mpdx_unet_set_status(u, 0) clears the word", fn, w, w >> 8, w >> 8);
}
// ---- the device state of the paired joined launch (mpdx_unet::LevelSplitState, host.hpp; fused_join_split_kernel): one occupancy query, then the exchange
// area and the counters of kSplitMaxB trajectories.  The status word and the budget are the runs' (inner_run_create).  capacity 0: no paired launch here.
static int level_split_create(mpdx_unet* u, int cus) {
    mpdx_unet::LevelSplitState& s = u->split;
    if (s.capacity >= 0) return 0;
    s.capacity = 0;
    if (int rc = inner_run_create(u->run, cus)) return rc;
    if (u->run.capacity <= 0 || !u->run.status_dev) return 0;
    s.wgs = fused_join_split_workgroups_per_cu();
    if (s.wgs < 1) return 0;
    HIP_TRY(hipMalloc((void**)&s.xch, (size_t)kSplitMaxB * kSplitTrajFloats * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&s.counters, (size_t)kSplitMaxB * kInnerRunCounterStride * sizeof(unsigned)));
    HIP_TRY(hipMemset(s.counters, 0, (size_t)kSplitMaxB * kInnerRunCounterStride * sizeof(unsigned)));
    s.capacity = cus;
    return 0;
}
static void level_split_free(mpdx_unet::LevelSplitState& s) {
    if (s.xch) (void)hipFree(s.xch);
    if (s.counters) (void)hipFree(s.counters);
}
// A paired launch of B trajectories starts: every counter of its trajectories holds *base_out.  A launch advances the counters of ITS trajectories only, so a
// larger batch than the launch before (a give-up's poison likewise) zeroes them all, stream-ordered, and starts from base 0 again.
static int level_split_begin(mpdx_unet::LevelSplitState& s, int B, hipStream_t st, unsigned* base_out) {
    if (B > kSplitMaxB) return fail(MPDX_E_STATE, "paired joined launch of %d trajectories (at most %d)", B, kSplitMaxB);
    if (s.rezero || B > s.live) {
        HIP_TRY(hipMemsetAsync(s.counters, 0, (size_t)kSplitMaxB * kInnerRunCounterStride * sizeof(unsigned), st));
        s.base = 0; s.rezero = false;
    }
    s.live = B;
    *base_out = s.base;
    s.base += kSplitAdvance;
    return 0;
}
// mpdx_plan only: the up program `up` of a pass (row `tt_row`, step `fa`) and the down program `dn` of the NEXT pass (row `tt_next`) as one launch
// (fused_join_kernel; split: its paired form, fused_join_split_kernel).  The down part starts from the x_{t-1} the up part has just computed, so its global
// input pointer is not used.
static int run_fused_join(mpdx_unet* u, const mpdx_unet::Fused& up, const mpdx_unet::Fused& dn, const float* packed, const float* tt_row, const float* tt_next,
                          const float* x, float* ws, int B, const FinalArgs* fa, hipStream_t st, long long* trace = nullptr, bool split = false) {
    if (int rc = ensure_fused_streams(u, packed, st)) return rc;
    FusedJoinArgs ja;
    FusedArgs d;
    if (int rc = fill_fused_args(u, up, packed, tt_row, x, ws, B, fa, ja.up)) return rc;
    if (int rc = fill_fused_args(u, dn, packed, tt_next, x, ws, B, nullptr, d)) return rc;
    ja.up.trace = trace;   // dev tool (mpdx_fused_trace with seg == number of segments); null in the plan
    ja.dn.packed = d.packed; ja.dn.tt_row = d.tt_row;
    for (int k = 0; k < 3; ++k) ja.dn.gout[k] = d.gout[k];
    ja.dn.gpar_off = d.gpar_off; ja.dn.tt_lo = d.tt_lo;
    for (int k = 0; k < kMaxFusedOps; ++k) ja.dn.sbase[k] = k < d.nops ? d.ops[k].sbase : 0;
    if (!split) return launch_fused_join(ja, B, st);
    FusedSplitArgs sa;
    memset(&sa, 0, sizeof(sa));
    if (int rc = level_split_begin(u->split, B, st, &sa.base)) return rc;
    sa.xch = u->split.xch; sa.counters = u->split.counters; sa.status = u->run.status_dev; sa.budget = u->run.budget; sa.nb8 = split_nb8(B);
    return launch_fused_join_split(ja, sa, B, st);
}

// mpdx_plan only: the seven 256 -> 256 Conv1dBlocks of the innermost level, layers [first, first + kInnerRunLayers), as ONE persistent launch (inner_run.hpp)
static long long* g_run_trace = nullptr;   // dev tool (mpdx_fused_trace on a run): kRunTraceSlots stamps per layer of the run kind g_run_trace_kind
static int g_run_trace_kind = -1;
constexpr int kRunTraceSlots = 32;
template <int N>
static int fill_run_args(mpdx_unet* u, int kind, int first, int width, const float* packed, const float* row, const float* x, float* ws, int B, hipStream_t st, RunArgs<N>& ra) {
    memset(&ra, 0, sizeof(ra));
    if (!inner_run_width_ok(width)) return fail(MPDX_E_STATE, "run unit of width %d", width);
    const int nc = inner_run_clusters(B, width);
    for (int k = 0; k < N; ++k) {
        if (int rc = make_conv_args(u, u->layers[first + k], packed, row, x, ws, B, 0, ra.layer[k])) return rc;
        ra.layer[k].n_tiles_n = nc;
        ra.layer[k].trace = g_run_trace && g_run_trace_kind == kind ? g_run_trace + k * kRunTraceSlots : nullptr;
    }
    ra.n_layers = N; ra.nc = nc;
    if (int rc = inner_run_begin(u->run, width, nc, N, st, &ra.counters, &ra.base)) return rc;
    ra.status = u->run.status_dev; ra.budget = u->run.budget;
    u->inner_run_layers += N;
    return 0;
}
static int run_inner_run(mpdx_unet* u, int first, int width, const float* packed, const float* row, const float* x, float* ws, int B, hipStream_t st) {
    InnerRunArgs ra;
    if (int rc = fill_run_args(u, mpdx_unet::kInnerRun, first, width, packed, row, x, ws, B, st, ra)) return rc;
    u->inner_runs++;
    return launch_inner_run(ra, B, width, st);
}
// mpdx_plan only: the tail of up level 0 - three 128 -> 128 Conv1dBlocks and Upsample1d(128), layers [first, first + kTailRunLayers) - as ONE persistent
// launch (inner_run.hpp).  It does not count in mpdx_unet_inner_runs.
static int run_tail_run(mpdx_unet* u, int first, int spare, int width, const float* packed, const float* row, const float* x, float* ws, int B, hipStream_t st) {
    TailRunArgs ra;
    if (spare < 0 || spare >= u->n_slots) return fail(MPDX_E_STATE, "tail run without a spare slot");
    if (int rc = fill_run_args(u, mpdx_unet::kTailRun, first, width, packed, row, x, ws, B, st, ra)) return rc;
    // layer 0's output, private to the run (layer 1's input, layer 2's residual), lives in the spare slot: tail_run_first says why
    float* const sp = ws + u->slot_floats * (size_t)B * spare;
    ra.layer[0].dst = sp; ra.layer[1].src1 = sp; ra.layer[2].res = sp;
    return launch_tail_run(ra, B, width, st);
}

// one launch unit of the pass (the SAME function serves the planning path, the profiler and the in-situ timer)
static int run_unit(mpdx_unet* u, const mpdx_unet::Unit& un, const float* packed, const float* row, const float* x, float* ws, int B,
                    const FinalArgs* fa, hipStream_t st) {
    if (un.kind == mpdx_unet::kProgram) return run_fused(u, u->fused[un.fused], packed, row, x, ws, B, fa, st);
    if (un.kind == mpdx_unet::kPair) return run_pair(u, u->layers[un.layer], u->layers[un.layer + 1], packed, row, x, ws, B, st);
    if (un.kind == mpdx_unet::kInnerRun) return run_inner_run(u, un.layer, un.width, packed, row, x, ws, B, st);
    if (un.kind == mpdx_unet::kTailRun) return run_tail_run(u, un.layer, un.fused, un.width, packed, row, x, ws, B, st);
    return run_layer(u, u->layers[un.layer], packed, row, x, ws, B, st);
}
static double unit_flops(const mpdx_unet* u, const mpdx_unet::Unit& un, int B) {
    double fl = 0.0;
    for (int k = un.layer; k < un.layer + un.count; ++k) fl += layer_flops(u->layers[k], B);
    return fl;
}

// ALGORITHMIC bytes of a launch unit: every weight / parameter it needs once + the activations that cross its boundary once (inputs,
// residual, outputs; what stays in LDS inside a fused program does not count) - the denominator of bench.py's traffic_over_algorithmic
static double layer_param_bytes(const mpdx_unet* u, const Layer& l) {
    if (l.attn) return 4.0 * ((double)u->params[l.w].n + (double)u->params[l.w2].n + 3.0 * l.cout);
    double n = (double)u->params[l.w].n + l.cout;
    if (l.gamma >= 0) n += 2.0 * l.cout;
    if (l.tb_off >= 0) n += l.cout;
    return 4.0 * n;
}
static double unit_bytes(const mpdx_unet* u, const mpdx_unet::Unit& un, int B) {
    auto act = [&](int L, int C) { return 4.0 * B * (double)L * C; };
    if (un.kind == mpdx_unet::kProgram) {
        const auto& f = u->fused[un.fused];
        const Layer& l0 = u->layers[f.first];
        double b = act(l0.L_in, l0.c1 + l0.c2);
        if (f.in3_consumer >= 0) b += act(u->layers[f.in3_consumer].L_in, u->layers[f.in3_consumer].c2);
        for (int k = f.first; k < f.first + f.count; ++k) b += layer_param_bytes(u, u->layers[k]);
        for (int k = 0; k < f.tmpl.nops; ++k)
            if (f.tmpl.ops[k].shape != kFusedShapeFinal && f.tmpl.ops[k].gdst >= 0) {
                const Layer& l = u->layers[f.op_layer[k]];
                b += act(l.L_out, l.cout);
            }
        if (f.has_final) b += 3.0 * act(u->cfg.n_support_points, u->cfg.state_dim);   // x_t in, noise in, x_{t-1} out
        return b;
    }
    double b = 0.0;
    for (int k = un.layer; k < un.layer + un.count; ++k) {
        const Layer& l = u->layers[k];
        b += layer_param_bytes(u, l) + act(l.L_out, l.cout) + (l.res != SRC_NONE ? act(l.L_out, l.cout) : 0.0);
        if (k == un.layer || un.kind != mpdx_unet::kPair) b += act(l.L_in, l.c1 + l.c2);   // a paired launch reads its input once
    }
    return b;
}

// One pass over the launch units, then the final kernel unless a program had it - the ONE loop over launch units: mpdx_plan, the single-pass entry
// points and the timing / trace entries (unet_measure.hpp) all come through here.  hook(kSkipUnit, i) != 0 leaves unit i out; hook(kBeforeLaunch /
// kAfterLaunch, i) runs around every launch and returns an error code; the final kernel counts as launch units.size().  A skipped program that holds
// the final op still stands for it: no separate final kernel either.  The two facts a pass of mpdx_plan adds (PlanSchedule::join holds for both):
// first_done - the first unit, the down program, has already run as the tail of the pass before; next_row != null - the last unit, the up program,
// runs joined with the NEXT pass's down program on that time-table row (join_trace: mpdx_fused_trace's stamps of that launch).
enum PassEvent { kSkipUnit, kBeforeLaunch, kAfterLaunch };
static int no_hook(PassEvent, int) { return 0; }
template <class Hook>
static int walk_pass(mpdx_unet* u, const std::vector<mpdx_unet::Unit>& units, const float* packed, const float* row, const float* x, float* ws,
                     int B, FinalArgs& fa, hipStream_t st, Hook&& hook, bool first_done = false, const float* next_row = nullptr,
                     long long* join_trace = nullptr, bool split = false) {
    const int n = (int)units.size();
    bool final_done = false;
    for (int i = first_done ? 1 : 0; i < n; ++i) {
        const mpdx_unet::Unit& un = units[i];
        if (un.kind == mpdx_unet::kProgram) final_done |= u->fused[un.fused].has_final;
        if (hook(kSkipUnit, i)) continue;
        if (int rc = hook(kBeforeLaunch, i)) return rc;
        const int rc = next_row && i == n - 1 ? run_fused_join(u, u->fused[un.fused], u->fused[units[0].fused], packed, row, next_row, x, ws, B, &fa, st, join_trace, split)
                                              : run_unit(u, un, packed, row, x, ws, B, &fa, st);
        if (rc) return rc;
        if (int rc = hook(kAfterLaunch, i)) return rc;
    }
    if (final_done) return 0;
    if (int rc = hook(kBeforeLaunch, n)) return rc;
    if (int rc = run_final(u, packed, fa, B, ws, st)) return rc;
    return hook(kAfterLaunch, n);
}

// the input a pass reads: x, or - a horizon in a container - the zero-padded copy of it this makes in the workspace
static const float* padded_input(const mpdx_unet* u, const float* x, float* ws, int B, hipStream_t st) {
    if (!u->masked()) return x;
    float* xc = ws + u->slot_floats * (size_t)B * u->xpad_slot;
    const size_t nx = (size_t)B * u->Hc * u->cfg.state_dim;
    hipLaunchKernelGGL(pad_input_kernel, dim3((unsigned)std::min<size_t>((nx + 255) / 256, 2048)), dim3(256), 0, st, x, xc, B, u->cfg.n_support_points, u->Hc,
                       u->cfg.state_dim);
    return xc;
}
// one U-Net pass + the final 1x1 conv / DDPM step described by `fa` (fa.mode 0: eps only)
static int run_unet_and_final(mpdx_unet* u, const float* packed, const float* timetab, int T, const float* x, int t, int B,
                              float* ws, FinalArgs& fa, hipStream_t st) {
    if (int rc = check_ready(u)) return rc;
    if (t < 0 || t >= T) return fail(MPDX_E_INVALID, "timestep %d outside [0,%d)", t, T);
    if (B <= 0) return fail(MPDX_E_INVALID, "B must be positive");
    return walk_pass(u, current_units(u, B, nullptr), packed, timetab + (size_t)t * u->tt_row, padded_input(u, x, ws, B, st), ws, B, fa, st, no_hook);
}

// ---- mpdx_plan's launch schedule
// First of kInnerRunLayers consecutive single-layer units that the inner-level run (inner_run.hpp) can stand for, or -1: every one a K-split
// 256 -> 256 Conv1dBlock on 8 positions with compile-time geometry.
static int inner_run_first(const mpdx_unet* u, const std::vector<mpdx_unet::Unit>& units) {
    auto fits = [&](const mpdx_unet::Unit& un) {
        if (un.kind != mpdx_unet::kLayer) return false;
        const Layer& l = u->layers[un.layer];
        if (l.attn || !(l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH) || l.Lv_out) return false;
        if (!(l.c1 == 256 && l.c2 == 0 && l.src2 == SRC_NONE && l.cout == 256 && l.L_in == 8 && l.L_out == 8 && l.gs == 32 && l.cin_pad == 256 && l.rs == 264)) return false;
        if ((l.tb_off >= 0) == (l.res != SRC_NONE)) return false;   // exactly one of time bias / residual
        // (the per-layer launch may pick a narrower position tile at small batch: the 8-wave K split and the GroupNorm regions - the arithmetic - do
        //  not depend on the tile's width)
        return layer_ksplit(l);
    };
    const int n = (int)units.size();
    for (int i = 0; i + kInnerRunLayers <= n; ++i) {
        int k = 0;
        while (k < kInnerRunLayers && fits(units[i + k])) ++k;
        if (k == kInnerRunLayers) return i;
    }
    return -1;
}
// First of the kTailRunLayers consecutive single-layer units the tail run (inner_run.hpp) can stand for, or -1: three K-split 128 -> 128 Conv1dBlocks
// on 8 positions (one GroupNorm group per 16-channel tile, one source, exactly one of time bias / residual), then Upsample1d(128) on 8 -> 16 positions
// over the whole horizon.  (make_conv_args leaves pre / accum / dst2 / c_split / decim / stuff zero on the planning path: what the GeoUp8 launch asks.)
// *spare: the workspace slot layer 0's output goes to inside the run (below).
static int tail_run_first(const mpdx_unet* u, const std::vector<mpdx_unet::Unit>& units, int* spare) {
    *spare = -1;
    auto layer_of = [&](const mpdx_unet::Unit& un) -> const Layer* {
        if (un.kind != mpdx_unet::kLayer) return nullptr;
        const Layer& l = u->layers[un.layer];
        if (l.attn || l.Lv_out || !(l.c1 == 128 && l.c2 == 0 && l.src2 == SRC_NONE && l.cout == 128 && l.L_in == 8 && l.cin_pad == 128)) return nullptr;
        return &l;
    };
    auto fits_gn = [&](const mpdx_unet::Unit& un) {
        const Layer* l = layer_of(un);
        if (!l || !(l->mode == CONV_S1 && l->ks == 5 && l->epi == EPI_GN_MISH && l->L_out == 8 && l->gs == 16 && l->rs == 136)) return false;
        if ((l->tb_off >= 0) == (l->res != SRC_NONE)) return false;   // exactly one of time bias / residual
        return layer_ksplit(*l);
    };
    auto fits_up = [&](const mpdx_unet::Unit& un) {
        const Layer* l = layer_of(un);
        return l && l->mode == CONV_UPT && l->ks == 4 && l->epi == EPI_BIAS && l->L_out == 16 && l->rs == 132 && l->res == SRC_NONE && l->tb_off < 0;
    };
    const int n = (int)units.size();
    for (int i = 0; i + kTailRunLayers <= n; ++i) {
        int k = 0;
        while (k < kTailRunLayers - 1 && fits_gn(units[i + k])) ++k;
        if (!(k == kTailRunLayers - 1 && fits_up(units[i + k]))) continue;
        // The three GroupNorm outputs are handed over tile-major inside the launch (RunCtx::tiled, RunSeqTail::tiled): the dataflow must be the one that
        // pattern is written for - a chain, layer 2's residual layer 0's output, layer 0 fed from earlier launches - and no layer behind the run may
        // read one of those three slots before it is written again.
        const int f = units[i].layer;
        const Layer &l0 = u->layers[f], &l1 = u->layers[f + 1], &l2 = u->layers[f + 2], &l3 = u->layers[f + 3];
        if (units[i + 1].layer != f + 1 || units[i + 2].layer != f + 2 || units[i + 3].layer != f + 3) continue;
        if (!(l1.src1 == l0.dst && l2.src1 == l1.dst && l2.res == l0.dst && l3.src1 == l2.dst && l0.res != SRC_NONE && l1.res == SRC_NONE)) continue;
        std::vector<int> kept = {l0.dst, l1.dst, l2.dst};   // slots that hold tile-major bytes when the run ends
        auto drop = [&](int s) { kept.erase(std::remove(kept.begin(), kept.end(), s), kept.end()); };
        auto held = [&](int s) { return std::find(kept.begin(), kept.end(), s) != kept.end(); };
        // (layer 0's own inputs come from earlier launches in [B][L][C]; a later layer of the run may reuse their slots, as between per-layer launches)
        if (l0.dst == l1.dst || l1.dst == l2.dst || l0.dst == l2.dst) continue;
        drop(l3.dst);
        bool read_later = false;
        for (int j = f + kTailRunLayers; j < (int)u->layers.size() && !read_later; ++j) {
            const Layer& l = u->layers[j];
            read_later = held(l.src1) || held(l.src2) || held(l.res);
            drop(l.dst);
        }
        if (read_later || held(u->final_slot)) continue;
        // Upsample1d's output is twice a trajectory's size of the other tensors: in its slot, trajectory b lies where trajectories 2 b and 2 b + 1 of a
        // [B][8][128] tensor lie, and those belong to ANOTHER cluster, which may still be reading them (the slot plan gives it layer 0's output slot: safe
        // only where layer 3 starts after ALL of layer 2).  So layer 0's output - private to the run - goes to a spare slot instead: one that none of
        // the four layers names and that is dead here (written before it is read again, if at all), e.g. the skip tensor the block before consumed.
        // (The rule is per trajectory and per slot, so it holds at either cluster width: with layer 0's output moved, NO other layer of the run names
        //  layer 3's destination slot - the checks below -, so whichever cluster owns trajectories 2 b and 2 b + 1, and however many trajectories a
        //  cluster has, nothing of the run reads or writes the bytes trajectory b's upsampled rows land on; every other tensor of the run, the spare
        //  slot included, gives trajectory b the same bytes of its slot, private to b's cluster.)
        auto named = [&](const Layer& l, int s) { return l.src1 == s || l.src2 == s || l.res == s || l.dst == s; };
        for (int s = 0; s < u->n_slots && *spare < 0; ++s) {
            if (s == u->xpad_slot || named(l0, s) || named(l1, s) || named(l2, s) || named(l3, s)) continue;
            bool dead = s != u->final_slot;
            for (int j = f + kTailRunLayers; j < (int)u->layers.size() && dead; ++j) {
                const Layer& l = u->layers[j];
                if (l.src1 == s || l.src2 == s || l.res == s) dead = false;
                else if (l.dst == s) break;
            }
            if (dead) *spare = s;
        }
        // with layer 0's output moved, layer 3's destination must be a slot no other layer of the run touches
        if (*spare < 0 || l3.dst == l1.dst || l3.dst == l2.dst || l3.dst == l0.src1 || l3.dst == l0.res) { *spare = -1; continue; }
        return i;
    }
    return -1;
}
static int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) (void)hipGetLastError();
    return cus;
}
// The automatic width of each run: a function of the batch alone, read from profiles/inner_run_narrow_ab.md.  The sweep (cfg2-shaped plans, ms per
// plan, width 16 minus width 32, one run selected, five rounds with spreads of 0.01 - 0.09 ms):
//     B             16      32      64     100     128
//     seven alone  -1.36   -1.54   -1.59   -0.17   -0.26
//     tail alone   -0.21   -0.19   -0.22   -0.04   -0.00
// Up to B = 64 every narrow workgroup has a compute unit to itself (8 ceil(B / 2) <= 256) and a launch uses twice the compute units of the wide
// form; beyond, two share a compute unit and the gain is what their phases overlap, bounded by the weight traffic (twice the wide form's per FLOP).
// The seven-layer run is narrow at every batch it admits: at the headline batch of 100 it meets the interleaved criterion (-0.170 ms per plan
// against a parent spread of 0.041).  The tail run does not (-0.069), so it is narrow up to B = 64 and keeps the wide form beyond: the measured
// crossover lies between 64 and 100, where the narrow workgroups stop having a compute unit each.
static int inner_run_auto_width(int B) { return (void)B, kRunNarrow; }
static int tail_run_auto_width(int B) { return B <= 64 ? kRunNarrow : kRunWide; }
// What mpdx_plan enqueues per pass at batch B, made once per call (the switches and the device are read here, not per pass): the launch units with the
// seven run layers as ONE unit where the run is selected, and whether passes can be joined.
// The batches at which the paired joined launch is taken when the handle leaves the choice open: read from profiles/level_split_ab.md.
static bool level_split_auto(int B) { return B <= kSplitMaxB; }
struct PlanSchedule {
    std::vector<mpdx_unet::Unit> units;
    bool run = false;    // units holds a kInnerRun or a kTailRun unit
    bool join = false;   // an unguided pass that has a successor ends in fused_join_kernel; the successor starts at its second unit
    bool split = false;  // ... in its paired form, fused_join_split_kernel
    int build(mpdx_unet* u, int B, bool with_run = true) {   // with_run = false: the per-layer units whatever the handle says (mpdx_fused_trace)
        units = current_units(u, B, nullptr);
        const int cus = device_cus();
        // The runs: the standard four-level network on H = 64 without self-attention, unmasked, and every workgroup of the launch resident at once
        // (B <= 128 on 256 CUs).
        if (with_run && u->inner_run && !u->masked() && !u->cfg.self_attention && u->cfg.n_levels == 4 && u->cfg.n_support_points == 64) {
            if (int rc = inner_run_create(u->run, cus)) return rc;
            // The width of a run: the handle's (mpdx_unet_set_inner_run_width), or automatic by batch; a launch is admitted where its whole grid is
            // resident at once (inner_run_resident) - B <= 128 on 256 compute units at either width.  0: the run is not taken.
            const bool may = u->run.capacity > 0 && sw::geo() && !sw::debug();
            auto width_of = [&](const int (&wgs)[2], int automatic) {
                auto fits = [&](int w) { return may && inner_run_grid(B, w) <= inner_run_resident(u->run.capacity, w, wgs[run_index(w)]); };
                if (u->inner_run_width) return fits(u->inner_run_width) ? u->inner_run_width : 0;
                // (a device whose occupancy answer for a narrow kernel is below 2 does not admit B > 64 at width 16: the wide form then)
                return fits(automatic) ? automatic : fits(kRunWide) ? kRunWide : 0;
            };
            const int sw7 = width_of(u->run.seven_wgs, inner_run_auto_width(B)), swt = width_of(u->run.tail_wgs, tail_run_auto_width(B));
            const int rf = sw7 && (u->inner_run & mpdx_unet::kRunSeven) ? inner_run_first(u, units) : -1;
            if (rf >= 0) {
                units[rf] = {mpdx_unet::kInnerRun, -1, units[rf].layer, kInnerRunLayers, sw7};
                units.erase(units.begin() + rf + 1, units.begin() + rf + kInnerRunLayers);
                run = true;
            }
            // the tail of up level 0, under the same conditions and on its own: the seven layers need not have been taken
            int spare = -1;   // (Unit::fused of a kTailRun unit: the spare slot of layer 0's output)
            const int tf = swt && (u->inner_run & mpdx_unet::kRunTail) ? tail_run_first(u, units, &spare) : -1;
            if (tf >= 0) {
                units[tf] = {mpdx_unet::kTailRun, spare, units[tf].layer, kTailRunLayers, swt};
                units.erase(units.begin() + tf + 1, units.begin() + tf + kTailRunLayers);
                run = true;
            }
        }
        // The join: the pass starts with the three-level down program from the network input and ends with the two-level up program that holds the final op
        // (the standard four-level network on a power-of-two horizon of 64), and one workgroup per CU runs anyway: the joined kernel's 84 KB of LDS admit
        // one workgroup per CU where the separate programs (59.1 / 63.5 KB) admit two.
        if (!u->plan_join || u->masked() || units.size() < 2) return 0;
        const mpdx_unet::Unit &first = units.front(), &last = units.back();
        if (first.kind != mpdx_unet::kProgram || last.kind != mpdx_unet::kProgram || first.fused == last.fused) return 0;
        const mpdx_unet::Fused &dn = u->fused[first.fused], &up = u->fused[last.fused];
        join = dn.program == 5 && dn.in1 == SRC_X && dn.in2 == SRC_NONE && !dn.has_final && up.program == 3 && up.has_final && B <= cus;
        // The paired form: both workgroups of every trajectory resident at once - 2 nb8 <= compute units, B <= 128 on 256 - on a handle that has not
        // switched it off.  Automatic (level_split < 0): by batch, level_split_auto.
        const bool want = u->level_split > 0 || (u->level_split < 0 && level_split_auto(B));
        if (join && want && u->cfg.state_dim <= 16 && split_grid(B) <= cus && B <= kSplitMaxB && sw::geo() && !sw::debug()) {
            if (int rc = level_split_create(u, cus)) return rc;
            split = u->split.capacity > 0 && split_grid(B) <= u->split.capacity * std::min(1, u->split.wgs);
        }
        return 0;
    }
};

// the trace / ablation entry points exist in a development build only: 0 there, else the error that says how to make one
int dev_hooks_missing(const char* fn) {
#ifdef MPDX_DEV_HOOKS
    return (void)fn, 0;
#endif
    return fail(MPDX_E_STATE, "%s needs a development build of libmpdx.so (MPDX_BUILD_DEFS=-DMPDX_DEV_HOOKS MPDX_BUILD_OUT=build_ab/libmpdx_dev.so python -m mpd_public_amd.build, then MPDX_LIB=build_ab/libmpdx_dev.so): "
                "the production kernels carry no trace / ablation hooks", fn);
}

}  // namespace mpdx

using namespace mpdx;

#include "unet_measure.hpp"   // mpdx_unet_profile / _time_units / _time_without, mpdx_bench_layer, the trace entries, the launch-unit queries

extern "C" {

const char* mpdx_last_error(void) { return g_err; }
int mpdx_version(void) { return 1; }

int mpdx_unet_create(const mpdx_unet_cfg* cfg, mpdx_unet** out) {
    if (!cfg || !out) return fail(MPDX_E_INVALID, "null argument");
    if (cfg->n_levels < 2 || cfg->n_levels > MPDX_MAX_LEVELS) return fail(MPDX_E_INVALID, "n_levels %d unsupported", cfg->n_levels);
    if (cfg->state_dim < 1 || cfg->state_dim > 64) return fail(MPDX_E_INVALID, "state_dim %d unsupported", cfg->state_dim);
    if (cfg->time_emb_dim != 32) return fail(MPDX_E_INVALID, "time_emb_dim must be 32 (TimeEncoder(32, .), temporal_unet.py:66)");
    if (cfg->unet_input_dim % 16) return fail(MPDX_E_INVALID, "unet_input_dim must be a multiple of 16");
    // final_conv is Conv1dBlock(unet_input_dim, unet_input_dim) on the output of the last up level, which has unet_input_dim * dim_mults[0]
    // channels (temporal_unet.py:98-116): the reference's own forward fails for dim_mults[0] != 1
    if (cfg->self_attention != 0 && cfg->self_attention != 1) return fail(MPDX_E_INVALID, "self_attention must be 0 or 1");
    if (cfg->dim_mults[0] != 1) return fail(MPDX_E_INVALID, "dim_mults[0] must be 1: final_conv takes unet_input_dim channels (temporal_unet.py:113-116)");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->dim_mults[i] < 1) return fail(MPDX_E_INVALID, "dim_mults[%d] = %d", i, cfg->dim_mults[i]);
    const int H = cfg->n_support_points;
    // the reference's U-Net takes every horizon its stride-2 / transposed convolutions map back onto itself: H % 2^(levels - 1) == 0
    // (temporal_unet.py:24,80-103).  Powers of two run natively; the others (24, 40, 48, 96 ...) in the next power-of-two container
    // with zeroed, masked rows (ConvArgs::Lv_out), one launch per layer
    if (H < 16 || H > 128 || (H % (1 << (cfg->n_levels - 1))) || (H >> (cfg->n_levels - 1)) < 2)
        return fail(MPDX_E_INVALID, "n_support_points %d must be a multiple of 2^(levels-1) = %d in [16, 128] with >= 2 points at the coarsest level", H,
                    1 << (cfg->n_levels - 1));
    // ups.j.0 reads the concatenation of the level below and the skip, 2 * dim_mults[lv] channels wide, and writes dim_mults[lv - 1]: where the two are
    // equal the reference's block has no residual_conv and its residual is the WHOLE concatenation (layers.py:337-355).  A layer here names one residual
    // slot of cout channels (build_model's rtb, ConvArgs::res), so such a network is refused, not run with half a residual
    for (int lv = 1; lv < cfg->n_levels; ++lv)
        if (2 * cfg->dim_mults[lv] == cfg->dim_mults[lv - 1])
            return fail(MPDX_E_INVALID, "layer ups.%d.0: identity residual over a concatenation (dim_mults[%d] = %d is twice dim_mults[%d] = %d, so the block "
                        "has no residual_conv) unsupported", cfg->n_levels - 1 - lv, lv - 1, cfg->dim_mults[lv - 1], lv, cfg->dim_mults[lv]);
    mpdx_unet* u = new mpdx_unet();
    u->cfg = *cfg;
    build_model(u);
    // GroupNorm regions (group x horizon) of 64 ... 2048 elements: one wave per region, 1, 2 or 4 x {1, 2, 4, 8} elements per lane
    // (conv_block.hpp).  The whole-trajectory fused programs exist for the shapes of H = 64 only; other horizons run one launch per layer.
    for (const Layer& l : u->layers)
        if (l.epi == EPI_GN_MISH) {
            const int re = l.gs * l.L_out;
            if (re < 64 || re > 2048 || (re & (re - 1)) || l.gs < 4 || 32 % l.gs) {
                std::string nm = l.name;
                delete u;
                return fail(MPDX_E_INVALID, "layer %s: GroupNorm region of %d elements (group of %d) unsupported", nm.c_str(), re, l.gs);
            }
        }
    for (const Layer& l : u->layers)
        if (l.attn)
            if (const char* why = attn_unsupported(l.cout, l.L_out)) {
                const std::string nm = l.name;
                const int ch = l.cout, np = l.L_out;
                delete u;
                return fail(MPDX_E_INVALID, "self-attention block %s (%d channels on %d positions): %s", nm.c_str(), ch, np, why);
            }
    if ((int)u->tt_w.size() > 40) { delete u; return fail(MPDX_E_INVALID, "too many residual blocks"); }
    build_units(u);
    u->packed_floats += 64;   // tail padding
    *out = u;
    return 0;
}

int mpdx_unet_set_plan_join(mpdx_unet* u, int on) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    u->plan_join = on ? 1 : 0;
    return 0;
}
int mpdx_unet_plan_joined(const mpdx_unet* u) { return u ? u->plan_joined : 0; }
int mpdx_unet_set_level_split(mpdx_unet* u, int on) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    u->level_split = on < 0 ? -1 : on ? 1 : 0;
    return 0;
}
int mpdx_unet_plan_split(const mpdx_unet* u) { return u ? u->plan_split : 0; }
int mpdx_level_split_block(int B, int block, int32_t* trajectory, int32_t* role) {
    if (B <= 0 || B > kSplitMaxB) return fail(MPDX_E_INVALID, "mpdx_level_split_block: B=%d", B);
    const int grid = split_grid(B);
    if (block < 0 || block >= grid) return fail(MPDX_E_INVALID, "mpdx_level_split_block: block %d of %d", block, grid);
    const SplitSlot s = split_slot(block, split_nb8(B));
    if (trajectory) *trajectory = s.b < B ? s.b : -1;
    if (role) *role = s.role;
    return grid;
}

int mpdx_unet_set_inner_run(mpdx_unet* u, int on) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    u->inner_run = on ? (mpdx_unet::kRunSeven | mpdx_unet::kRunTail) : 0;   // everything that is eligible, or nothing
    return 0;
}
int mpdx_unet_set_inner_run_parts(mpdx_unet* u, int parts) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    if (parts & ~(mpdx_unet::kRunSeven | mpdx_unet::kRunTail)) return fail(MPDX_E_INVALID, "inner-run parts 0x%x: bit 0 the seven 256 -> 256 layers, bit 1 the tail of up level 0", parts);
    u->inner_run = parts;
    return 0;
}
int mpdx_unet_set_inner_run_width(mpdx_unet* u, int width) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    if (width != 0 && !inner_run_width_ok(width)) return fail(MPDX_E_INVALID, "inner-run width %d: 0 (automatic), 16 or 32 positions per cluster", width);
    u->inner_run_width = width;
    return 0;
}
int mpdx_inner_run_block(int B, int width, int cus, int block, int32_t* cluster, int32_t* tile, int32_t* counter_lines) {
    if (B <= 0 || cus <= 0 || !inner_run_width_ok(width)) return fail(MPDX_E_INVALID, "mpdx_inner_run_block: B=%d width=%d cus=%d", B, width, cus);
    const int grid = inner_run_grid(B, width);
    if (block < 0 || block >= grid) return fail(MPDX_E_INVALID, "mpdx_inner_run_block: block %d of %d", block, grid);
    int c = 0, m = 0;
    inner_run_slot(block, &c, &m);
    if (cluster) *cluster = c < inner_run_clusters(B, width) ? c : -1;
    if (tile) *tile = m;
    if (counter_lines) *counter_lines = inner_run_counter_lines(cus, width);
    return grid;
}
int mpdx_unet_inner_runs(const mpdx_unet* u) { return u ? u->inner_runs : 0; }
int mpdx_unet_inner_run_layers(const mpdx_unet* u) { return u ? u->inner_run_layers : 0; }
int mpdx_unet_status(const mpdx_unet* u) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    return handle_status_error(u, "mpdx_unet_status");
}
int mpdx_unet_set_status(mpdx_unet* u, unsigned word) {
    if (!u) return fail(MPDX_E_INVALID, "null argument");
    if (u->run.status) __atomic_store_n(u->run.status, word, __ATOMIC_RELAXED);
    u->run.status_host = word;
    if (!word && u->run.counters) u->run.ctr[0].rezero = u->run.ctr[1].rezero = true;   // whatever a give-up left in the counters goes before the next run
    if (!word) u->split.rezero = true;
    return 0;
}

void mpdx_unet_destroy(mpdx_unet* u) {
    if (u && u->pack_descs_dev) (void)hipFree(u->pack_descs_dev);
    if (u && u->pack_chunks_dev) (void)hipFree(u->pack_chunks_dev);
    if (u && u->jobs_dev) (void)hipFree(u->jobs_dev);
    if (u) inner_run_free(u->run);
    if (u) level_split_free(u->split);
    delete u;
}

int mpdx_unet_num_params(const mpdx_unet* u) { return u ? (int)u->params.size() : 0; }

int mpdx_unet_param_info(const mpdx_unet* u, int idx, const char** name, int32_t shape[3], int32_t* ndim) {
    if (!u || idx < 0 || idx >= (int)u->params.size()) return fail(MPDX_E_INVALID, "bad parameter index %d", idx);
    const Param& p = u->params[idx];
    if (name) *name = p.name.c_str();
    if (shape) { shape[0] = p.shape[0]; shape[1] = p.shape[1]; shape[2] = p.shape[2]; }
    if (ndim) *ndim = p.ndim;
    return 0;
}

size_t mpdx_unet_packed_floats(const mpdx_unet* u) { return u ? u->packed_floats : 0; }
size_t mpdx_unet_timetab_floats(const mpdx_unet* u, int T) { return u ? (size_t)T * u->tt_row : 0; }
size_t mpdx_unet_workspace_floats(const mpdx_unet* u, int B) { return u ? u->slot_floats * (size_t)B * u->n_slots : 0; }

int mpdx_unet_pack_param(mpdx_unet* u, const char* name, const float* src, size_t n, float* packed, void* stream) {
    if (!u || !name || !src || !packed) return fail(MPDX_E_INVALID, "null argument");
    auto it = u->pidx.find(name);
    if (it == u->pidx.end()) return fail(MPDX_E_NOTFOUND, "unexpected state-dict key '%s'", name);
    Param& p = u->params[it->second];
    if (n != p.n) return fail(MPDX_E_INVALID, "'%s': got %zu floats, expected %zu", name, n, p.n);
    hipStream_t st = (hipStream_t)stream;
    if (p.kind == PK_VEC) {
        hipLaunchKernelGGL(copy_kernel, dim3((unsigned)std::min<size_t>((p.n + 255) / 256, 1024)), dim3(256), 0, st, src, packed + p.off, p.n);
    } else {
        hipLaunchKernelGGL(pack_conv_weights_kernel, dim3((unsigned)std::min<size_t>((p.pn + 255) / 256, 2048)), dim3(256), 0, st, src,
                           packed + p.off, p.cout, p.cin, p.ksz, p.cin_pad, p.nslot, p.kind == PK_CONVT ? 1 : 0);
    }
    HIP_TRY(hipGetLastError());
    if (!p.done) { p.done = true; u->n_done++; }
    u->pack_version++;   // the stream-ordered copies of the fused segments are stale now
    return 0;
}

int mpdx_unet_build_timetab(mpdx_unet* u, const float* packed, const float* freqs16, int T, float* timetab, void* stream) {
    if (!u || !packed || !freqs16 || !timetab || T <= 0) return fail(MPDX_E_INVALID, "bad argument");
    if (int rc = check_ready(u)) return rc;
    TimeTabArgs a;
    memset(&a, 0, sizeof(a));
    a.packed = packed; a.freqs = freqs16; a.tab = timetab;
    a.w1 = (int)u->params[u->pidx.at("time_mlp.encoder.1.weight")].off;
    a.b1 = (int)u->params[u->pidx.at("time_mlp.encoder.1.bias")].off;
    a.w2 = (int)u->params[u->pidx.at("time_mlp.encoder.3.weight")].off;
    a.b2 = (int)u->params[u->pidx.at("time_mlp.encoder.3.bias")].off;
    a.row = u->tt_row;
    a.nblk = (int)u->tt_w.size();
    for (int i = 0; i < a.nblk; ++i) {
        a.woff[i] = (int)u->params[u->tt_w[i]].off;
        a.boff[i] = (int)u->params[u->tt_b[i]].off;
        a.cout[i] = u->tt_cout[i];
        a.toff[i] = u->tt_off[i];
    }
    hipLaunchKernelGGL(timetab_kernel, dim3(T), dim3(128), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_unet_forward(mpdx_unet* u, const float* packed, const float* timetab, int T, const float* x, int t, float* eps,
                      int B, float* ws, void* stream) {
    if (!u || !packed || !timetab || !x || !eps || !ws) return fail(MPDX_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    FinalArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.out = eps; fa.mode = 0; fa.n_per_ctx = 1;
    if (int rc = run_unet_and_final(u, packed, timetab, T, x, t, B, ws, fa, st)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_ddpm_step(mpdx_unet* u, const float* packed, const float* timetab, int T, float* x_io, const float* noise,
                   const float* hard_start, const float* hard_goal, const mpdx_step_coefs* coefs, int t, int mean_only,
                   float* chain_out, uint32_t* absmax_out, int n_per_ctx, int B, float* ws, void* stream) {
    if (!u || !packed || !timetab || !x_io || !coefs || !ws) return fail(MPDX_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    FinalArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.x_in = x_io; fa.out = x_io; fa.noise = noise; fa.hs = hard_start; fa.hg = hard_goal;
    fa.chain = chain_out; fa.absmax = absmax_out; fa.n_per_ctx = n_per_ctx > 0 ? n_per_ctx : B;
    fa.mode = mean_only == 2 ? 3 : (mean_only ? 2 : 1);
    fa.k = *coefs;
    if (int rc = run_unet_and_final(u, packed, timetab, T, x_io, t, B, ws, fa, st)) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_add_noise(float* x_io, const float* noise, const float* hard_start, const float* hard_goal, float noise_scale,
                   float noise_std_extra, float* chain_out, int B, int H, int D, void* stream) {
    if (!x_io || B <= 0) return fail(MPDX_E_INVALID, "bad argument");
    const size_t n = (size_t)B * H * D;
    hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                       x_io, noise, hard_start, hard_goal, noise_scale, noise_std_extra, chain_out, B, H, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_hard_conds(float* x_io, float* chain_out, int n, const int32_t* horizon_idx, const float* const* values, int B, int H, int D, void* stream) {
    if (!x_io || B <= 0 || H <= 0 || D <= 0 || n < 0 || (n && (!horizon_idx || !values))) return fail(MPDX_E_INVALID, "bad argument");
    if (n > kMaxHardConds) return fail(MPDX_E_INVALID, "at most 16 hard conditions per call");
    if (n == 0) return 0;
    HardCondArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    for (int k = 0; k < n; ++k) {
        int t = horizon_idx[k];
        if (t < 0) t += H;   // python indexing: x[:, -1, :]
        if (t < 0 || t >= H) return fail(MPDX_E_INVALID, "hard condition index out of range for this horizon");
        if (!values[k]) return fail(MPDX_E_INVALID, "null hard condition table");
        a.idx[k] = t; a.vals[k] = values[k];
    }
    const size_t per = (size_t)B * D;
    hipLaunchKernelGGL(hard_conds_kernel, dim3((unsigned)std::min<size_t>((per + 255) / 256, 1024)), dim3(256), 0, (hipStream_t)stream, x_io, chain_out, a, B, H, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_q_sample(const float* x_start, const float* noise, const long long* t_dev, const float* sqrt_alphas_cumprod_dev,
                  const float* sqrt_one_minus_alphas_cumprod_dev, const float* hard_start, const float* hard_goal, float* out, int B, int H,
                  int D, int T, void* stream) {
    if (!x_start || !noise || !t_dev || !sqrt_alphas_cumprod_dev || !sqrt_one_minus_alphas_cumprod_dev || !out || B <= 0 || T <= 0)
        return fail(MPDX_E_INVALID, "bad argument");
    const size_t n = (size_t)B * H * D;
    hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)stream, x_start, noise,
                       t_dev, sqrt_alphas_cumprod_dev, sqrt_one_minus_alphas_cumprod_dev, hard_start, hard_goal, out, B, H, D, T);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_weighted_loss(const float* pred, const float* targ, const float* weights_hd, const float* hard_start, const float* hard_goal,
                       int l1, float* out1, int B, int H, int D, void* stream) {
    if (!pred || !targ || !out1 || B <= 0) return fail(MPDX_E_INVALID, "bad argument");
    hipLaunchKernelGGL(weighted_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, targ, weights_hd, hard_start, hard_goal, l1, out1,
                       B, H, D);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_plan(mpdx_unet* u, const float* packed, const float* timetab, int T, const mpdx_step_coefs* coefs, int n_without_noise,
              float* x, const float* noise, const float* hard_start, const float* hard_goal, float* chain, int B, float* ws,
              const mpdx_guide_params* guide, int n_guide_steps, int t_start_guide, uint32_t* guide_flags, int n_per_ctx,
              uint64_t rng_seed, uint64_t rng_offset, void* stream) {
    if (!u || !packed || !timetab || !coefs || !x || !ws || T <= 0 || n_without_noise < 0 || B <= 0)
        return fail(MPDX_E_INVALID, "bad argument");
    if (int rc = handle_status_error(u, "mpdx_plan")) return rc;   // sticky: a run of an earlier plan on this handle gave up (no synchronisation: a host read)
    if (guide)   // the tracks of moving obstacles first, as guide_block_problem orders the checks (members only; H is the network's)
        if (const char* why = motion_params_problem(*guide, u->cfg.n_support_points)) return fail(MPDX_E_INVALID, "%s", why);
    if (guide)   // the scene members are checked here, before the first launch of the loop (launch_guide checks them again per launch)
        if (const char* why = scene_params_problem(*guide)) return fail(MPDX_E_INVALID, "%s", why);
    if (guide)   // ... and so is a chain robot's table (a device table is read here, once, outside the loop)
        if (const char* why = chain_params_problem(*guide)) return fail(MPDX_E_INVALID, "%s", why);
    if (guide)   // ... and the tool-axis members
        if (const char* why = tool_params_problem(*guide)) return fail(MPDX_E_INVALID, "%s", why);
    if (int rc = check_ready(u)) return rc;
    // An unguided iteration that has a successor runs its up program and the successor's down program as ONE launch (nothing modifies x between the
    // two); the successor then starts at its second unit.  Whether the successor is guided does not matter.  The seven 256 -> 256 layers of the
    // innermost level are one persistent launch in guided iterations too: the inner levels do not see the guide.
    PlanSchedule ps;
    if (int rc = ps.build(u, B)) return rc;
    u->inner_runs = u->inner_run_layers = u->plan_joined = u->plan_split = 0;
    hipStream_t st = (hipStream_t)stream;
    const int H = u->cfg.n_support_points, D = u->cfg.state_dim;
    const size_t n = (size_t)B * H * D;
    const int npc = n_per_ctx > 0 ? n_per_ctx : B;
    const int n_ctx = (B + npc - 1) / npc;
    const int steps = T + n_without_noise;
    if (n_guide_steps < 0) return fail(MPDX_E_INVALID, "n_guide_steps %d", n_guide_steps);
    if (n_guide_steps == 0) guide = nullptr;   // range(0): the reference runs no guide iteration (sample_functions.py:74)
    const int dbg = sw::debug();
    if (guide) {
        if (!guide_flags) return fail(MPDX_E_INVALID, "guide needs guide_flags");
        if (B % npc) return fail(MPDX_E_INVALID, "B=%d is not a multiple of n_per_ctx=%d", B, npc);
        HIP_TRY(hipMemsetAsync(guide_flags, 0, (size_t)steps * (n_guide_steps + 1) * n_ctx * sizeof(uint32_t), st));
    }
    // x_T with hard conditioning; chain[0]
    hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, st, x, (const float*)nullptr,
                       hard_start, hard_goal, 0.f, 0.f, chain, B, H, D);
    bool down_done = false;   // this iteration's down program ran as the tail of the iteration before
    int k = 0;
    for (int i = T - 1; i >= -n_without_noise; --i, ++k) {
        const int t = i < 0 ? 0 : i;
        const bool guided = guide && i < t_start_guide;  // sample_functions.py:39 compares the un-clamped index
        const bool join = ps.join && !guided && i > -n_without_noise;
        const float* tt_next = join ? timetab + (size_t)(i - 1 < 0 ? 0 : i - 1) * u->tt_row : nullptr;
        const float* nz = (t == 0 || !noise) ? nullptr : noise + (size_t)k * n;  // noise[t == 0] = 0  (sample_functions.py:52)
        // noise == NULL: the step's draw is generated in place; iteration k uses elements [(k+1) n, (k+2) n) of the stream whose
        // first n elements are x_T (what mpdx_randn(x, n, seed, offset) wrote): the same bits a pre-generated tensor would hold
        NoiseRng rng;
        memset(&rng, 0, sizeof(rng));
        if (!noise && t != 0) { rng.on = 1; rng.seed = rng_seed; rng.offset = rng_offset; rng.elem0 = (unsigned long long)(k + 1) * n; }
        float* ch = chain ? chain + (size_t)(k + 1) * n : nullptr;
        uint32_t* fl = guided ? guide_flags + (size_t)k * (n_guide_steps + 1) * n_ctx : nullptr;
        FinalArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.x_in = x; fa.out = x;
        fa.k = coefs[t];
        fa.n_per_ctx = npc;
        if (!guided) {
            fa.rng = rng; fa.noise = nz; fa.hs = hard_start; fa.hg = hard_goal;
            fa.chain = ch; fa.mode = 1;
        } else {
            fa.mode = 2; fa.absmax = fl;  // posterior mean + its max|.| per context
        }
        if (int rc = walk_pass(u, ps.units, packed, timetab + (size_t)t * u->tt_row, padded_input(u, x, ws, B, st), ws, B, fa, st, no_hook, down_done, tt_next, nullptr, ps.split))
            return rc;
        down_done = join;
        u->plan_joined += join ? 1 : 0;
        u->plan_split += join && ps.split ? 1 : 0;
        if (guided) {
            for (int j = 0; j < n_guide_steps; ++j) {
                const bool last = j == n_guide_steps - 1;  // the last iteration also adds the noise term and appends to the chain
                if (int rc = launch_guide(guide, x, nullptr, hard_start, hard_goal, fl + (size_t)j * n_ctx, fl + (size_t)(j + 1) * n_ctx, npc, B, H,
                                          D, st, last ? nz : nullptr, coefs[t].noise_scale, coefs[t].noise_std_extra, last ? ch : nullptr,
                                          coefs[t].guide_scale, last ? &rng : nullptr))
                    return rc;
            }
        }
        if (dbg) {   // MPDX_DEBUG: attribute launch / execution errors to the loop iteration that caused them
            if (dbg >= 2) {
                const hipError_t e = hipStreamSynchronize(st);
                if (e != hipSuccess) return fail((int)e, "mpdx_plan: loop iteration %d (t=%d%s) faulted: %s", k, t, guided ? ", guided" : "", hipGetErrorString(e));
            }
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail((int)e, "mpdx_plan: launch in loop iteration %d (t=%d%s) failed: %s", k, t, guided ? ", guided" : "", hipGetErrorString(e));
        }
    }
    HIP_TRY(hipGetLastError());
    return ps.run || ps.split ? handle_status_error(u, "mpdx_plan") : 0;   // (what has already given up by now; the rest shows at the next call or in mpdx_unet_status)
}

int mpdx_randn(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
    if (!out) return fail(MPDX_E_INVALID, "null argument");
    if (n == 0) return 0;
    const size_t nquad = (n + 3) / 4;
    hipLaunchKernelGGL(randn_kernel, dim3((unsigned)std::min<size_t>((nquad + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, out, n,
                       seed, offset);
    HIP_TRY(hipGetLastError());
    return 0;
}

// dev entry: ONE Residual(PreNorm(LinearAttention)) block on a caller-owned activation, through the code a network runs (pack_conv_weights_kernel,
// a Layer filled as build_model's `attention` lambda fills it, launch_attention).  Synchronises the stream (it frees its packed weights).
int mpdx_attention_block(float* x, const float* to_qkv_w, const float* to_out_w, const float* to_out_b, const float* norm_g, const float* norm_b,
                         int B, int L, int Lv, int C, void* stream) {
    if (!x || !to_qkv_w || !to_out_w || !to_out_b || !norm_g || !norm_b) return fail(MPDX_E_INVALID, "null argument");
    if (B <= 0) return fail(MPDX_E_INVALID, "batch must be positive");
    if (const char* why = attn_unsupported(C, L)) return fail(MPDX_E_INVALID, "self-attention block (%d channels on %d positions): %s", C, L, why);
    if (Lv < 1 || Lv > L) return fail(MPDX_E_INVALID, "valid positions must be in [1, %d]", L);
    hipStream_t st = (hipStream_t)stream;
    Layer l;
    l.name = "mpdx_attention_block"; l.attn = true; l.mode = CONV_S1; l.ks = 0; l.epi = EPI_BIAS;
    l.c1 = C; l.cout = C; l.L_in = L; l.L_out = L;
    l.Lv_out = Lv != L ? Lv : 0;
    l.cin_pad = pad_cin(C);
    l.rs = pick_row_stride(l.cin_pad, CONV_S1, L, L, L);
    const int hid_pad = pad_cin(kAttnHid);
    const size_t n_qkv = (size_t)(3 * kAttnHid / 16) * (l.cin_pad / 16) * 256, n_out = (size_t)(C / 16) * (hid_pad / 16) * 256;
    float* packed = nullptr;
    HIP_TRY(hipMalloc(&packed, (n_qkv + n_out) * sizeof(float)));
    hipLaunchKernelGGL(pack_conv_weights_kernel, dim3((unsigned)std::min<size_t>((n_qkv + 255) / 256, 2048)), dim3(256), 0, st, to_qkv_w, packed,
                       3 * kAttnHid, C, 1, l.cin_pad, 1, 0);
    hipLaunchKernelGGL(pack_conv_weights_kernel, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 2048)), dim3(256), 0, st, to_out_w, packed + n_qkv,
                       C, kAttnHid, 1, hid_pad, 1, 0);
    AttnArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.x = x; aa.wqkv = packed; aa.wout = packed + n_qkv; aa.bout = to_out_b; aa.g = norm_g; aa.b = norm_b;
    int rc = launch_attention(l, aa, B, st);
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    (void)hipFree(packed);
    if (rc) return rc;
    if (e != hipSuccess) return fail((int)e, "mpdx_attention_block: %s", hipGetErrorString(e));
    return 0;
}

}  // extern "C"

