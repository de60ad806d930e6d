// train_host.hpp - host side of the training step (included at the end of k_train.hip; kernels in train.hpp).
// Entry points: mpdx_train_* (include/mpdx.h).  Everything is enqueued on the caller's stream; no synchronisation.
// mpdx_train_loss_backward runs the stages of TrainPass below; the whole-trajectory backward programs among them live in train_bwd_prog.hpp.
#pragma once

namespace mpdx {

// one-off: the flat (reference-layout) offsets of every parameter, the dgrad convolution of every layer whose input needs a
// gradient, and the producer of every tensor a layer reads (the forward engine recycles 4 + n_levels slots; training keeps
// every layer's output)
static void build_train_plan(mpdx_unet* u) {
    if (u->train_ready) return;
    size_t fo = 0;
    for (auto& p : u->params) { p.foff = fo; fo += (p.n + 3) / 4 * 4; }
    u->flat_floats = fo;
    const int n = (int)u->layers.size();
    u->tl.assign(n, {});
    std::unordered_map<int, int> owner;   // slot -> layer that wrote it last
    size_t pt = 0;
    for (int i = 0; i < n; ++i) {
        const Layer& l = u->layers[i];
        auto& t = u->tl[i];
        auto prod = [&](int s) { return s == SRC_X ? -1 : (s == SRC_NONE ? -2 : owner.at(s)); };
        t.src1_l = prod(l.src1); t.src2_l = prod(l.src2); t.res_l = prod(l.res);
        owner[l.dst] = i;
        t.need_dgrad = (t.src1_l >= 0) || (t.src2_l >= 0);
        t.dgrad_woff = ~(size_t)0;
        if (t.need_dgrad) {
            Layer d;
            d.name = "dgrad(" + l.name + ")";
            d.mode = CONV_S1; d.epi = EPI_BIAS;
            d.ks = l.mode == CONV_S1 ? l.ks : (l.mode == CONV_DOWN ? 3 : 5);
            d.c1 = l.cout; d.c2 = 0; d.cout = l.c1 + l.c2;
            d.L_in = d.L_out = l.mode == CONV_UPT ? l.L_out : l.L_in;
            // a padded container: valid rows of the dgrad's output = of the layer's input (ConvTranspose: full resolution, decimated at the store)
            d.Lv_out = l.Lv_out == 0 ? 0 : (l.mode == CONV_UPT ? l.Lv_out : (l.mode == CONV_DOWN ? 2 * l.Lv_out : l.Lv_out));
            d.cin_pad = (d.c1 + 15) / 16 * 16;
            d.rs = pick_row_stride(d.cin_pad, CONV_S1, d.L_in, d.L_out, d.L_in + 2 * (d.ks / 2));
            t.dg = d;
            t.dgrad_woff = pt;
            pt += (size_t)(d.cout / 16) * (d.cin_pad / 16) * d.ks * 256;
        }
    }
    u->packedT_floats = pt;
    // packing table
    std::vector<PackDesc> descs;
    for (size_t k = 0; k < u->params.size(); ++k) {
        const Param& p = u->params[k];
        PackDesc d;
        memset(&d, 0, sizeof(d));
        d.src = p.foff; d.dst = p.off; d.dstT = ~0ull;
        d.n = p.n; d.pn = p.pn; d.kind = p.kind;
        d.cout = p.cout; d.cin = p.cin; d.ks = p.ksz; d.cin_pad = p.cin_pad; d.nslot = p.nslot;
        for (int i = 0; i < n; ++i)
            if (u->layers[i].w == (int)k && u->tl[i].need_dgrad) {
                const Layer& g = u->tl[i].dg;
                d.dstT = u->tl[i].dgrad_woff;
                d.t_cout = g.cout; d.t_cin = g.c1; d.t_ks = g.ks; d.t_cin_pad = g.cin_pad;
                d.t_mode = u->layers[i].mode == CONV_UPT ? 1 : 0;
                d.pnT = (size_t)(g.cout / 16) * (g.cin_pad / 16) * g.ks * 256;
            }
        descs.push_back(d);
    }
    u->pack_descs_host = descs;
    u->train_ready = true;
}

static int ensure_pack_descs(mpdx_unet* u) {
    if (u->pack_descs_dev) return 0;
    // the chunk table of pack_train_kernel: kPackGroups groups of one pack of one parameter per block
    std::vector<PackChunk> chunks;
    for (size_t k = 0; k < u->pack_descs_host.size(); ++k) {
        const PackDesc& d = u->pack_descs_host[k];
        if (d.pn >= (1ull << 32) || d.pnT >= (1ull << 32) || d.n >= (1ull << 32)) return fail(MPDX_E_INVALID, "parameter %zu: more than 2^32 packed floats", k);
        // (PackChunk::first: the chunk's first GROUP - nslot consecutive 256-float blocks; kPackGroups groups per chunk)
        const unsigned long long gf = 256ull * (unsigned long long)(d.kind == 0 ? 1 : d.nslot), gt = 256ull * (unsigned long long)std::max(d.t_ks, 1);
        if (d.kind != 0 && d.nslot > 5) return fail(MPDX_E_INVALID, "parameter %zu: %d tap slots (the repack kernel holds 5)", k, d.nslot);
        if (d.dstT != ~0ull && d.t_ks > 5) return fail(MPDX_E_INVALID, "parameter %zu: %d dgrad taps (the repack kernel holds 5)", k, d.t_ks);
        for (unsigned long long g = 0; g * gf < d.pn; g += kPackGroups) chunks.push_back(PackChunk{(int)k, 0, (unsigned)g, 0u});
        if (d.dstT != ~0ull)
            for (unsigned long long g = 0; g * gt < d.pnT; g += kPackGroups) chunks.push_back(PackChunk{(int)k, 1, (unsigned)g, 0u});
    }
    u->n_pack_chunks = chunks.size();
    HIP_TRY(hipMalloc(&u->pack_chunks_dev, chunks.size() * sizeof(PackChunk)));
    HIP_TRY(hipMemcpy(u->pack_chunks_dev, chunks.data(), chunks.size() * sizeof(PackChunk), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&u->pack_descs_dev, u->pack_descs_host.size() * sizeof(PackDesc)));
    HIP_TRY(hipMemcpy(u->pack_descs_dev, u->pack_descs_host.data(), u->pack_descs_host.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
    return 0;
}

// workspace layout for a batch of B (float offsets)
struct TrainWs {
    size_t xn, eps, dE, out0, pre0, grad0, dU, pvec, wpart, rpart, emb, h1, temb, tm, h1m, tb, dT, dtm, dh1, zeros, ticket, lossp, total;
    size_t slotB;          // floats of one activation slot for the batch
    size_t wpart_floats;
    // deferred reductions (one launch each at the end of the backward pass): every layer keeps its own partial sums
    bool deferred;
    size_t wparts, pvecs;  // areas; carved up in launch order by the backward pass
};
static size_t wgrad_splits(int M, int N, int B) {
    const int tiles = ((M + 31) / 32) * ((N + 31) / 32);
    int S = (256 + tiles - 1) / tiles;   // about one workgroup per CU
    // How many batch splits: more splits = shorter trajectory chains per block but more partial sums to write and re-read (wgrad_reduce_all).  With the
    // prefetching trajectory loop the measured optimum of the 256 x 256 layers (64 tiles, 4 splits by the rule above) is 2 / 2 / 4 / 8 splits at batch
    // 32 / 64 / 128 / 512 (gpurun_out/r04za/wgrad_rule*.txt: batch 32 0.68 -> 0.63 ms with half the splits, batch 512 2.42 -> 2.37 with twice) - the
    // rule's count times sqrt(B / 128), within [1/2, 2]; fewer splits for every layer, more only for the layers with many tiles.
    {
        const float f = std::min(2.0f, std::max(0.5f, sqrtf((float)B / 128.0f)));
        if (f < 1.0f || tiles >= 16) S = std::max(1, (int)lroundf((float)S * f));
    }
    S = std::max(1, std::min(S, B));
    const int per = (B + S - 1) / S;
    return (size_t)((B + per - 1) / per);
}
// make_wgrad's `sdiv` (a divisor of wgrad_splits' count; negative: a multiplier) for the weight gradients that run behind the backward chain, and
// for the backward programs' layers.  MPDX_WGRAD_LATE_DIV, clamped to >= 1, overrides both rules.
static int wgrad_late_div_override() {   // 0: not set
    const int v = sw::wgrad_late_div();
    return v == sw::kUnset ? 0 : std::max(1, v);
}
// fewer batch splits for the weight gradients that run behind the chain (measured, profiles/r06_train_late_div_ab.txt: batch 128 x D = 14 0.898 / 0.84 / 0.82 /
// 0.81 ms with 1 / 4 / 8 / 16; batch 512 2.027 / 1.94 / 1.96 / 2.01): 8 up to batch 128, 4 beyond
static int wgrad_late_sdiv(int B) {
    if (const int o = wgrad_late_div_override()) return o;
    return B < 64 ? 4 : (B <= 128 ? 8 : 4);
}
// the backward programs' layers: the same rule from batch 64 on; below, 4 (measured with the host out of the way, profiles/r06_train_b32_split_ab.txt) unless
// MPDX_WGRAD_PROG_MUL > 1 asks for up to 4 x MORE splits there
static int wgrad_prog_sdiv(int B) {
    const int late_div_env = wgrad_late_div_override(), small_mul = sw::wgrad_prog_mul();
    return late_div_env ? late_div_env : (B >= 64 ? (B <= 128 ? 8 : 4) : (small_mul > 1 ? -std::min(small_mul, 4) : 4));
}
static TrainWs train_ws(const mpdx_unet* u, int B) {
    TrainWs w;
    const size_t n = u->layers.size();
    const int H = u->cfg.n_support_points, D = u->cfg.state_dim;
    w.slotB = u->slot_floats * (size_t)B;
    const size_t xs = ((size_t)B * std::max(H, u->Hc) * D + 3) / 4 * 4;   // (xn and dE live in the network's container layout)
    size_t o = 0;
    auto take = [&](size_t k) { const size_t r = o; o += (k + 3) / 4 * 4; return r; };
    w.xn = take(xs); w.eps = take(xs); w.dE = take(xs);
    w.out0 = take(n * w.slotB);
    w.pre0 = take(n * w.slotB);
    w.grad0 = take(n * w.slotB);
    w.dU = take(w.slotB);
    w.pvec = take((size_t)4 * B * 512);
    size_t wp = 0;
    for (const Layer& l : u->layers) {
        const int M = l.mode == CONV_UPT ? l.c1 + l.c2 : l.cout, N = l.mode == CONV_UPT ? l.cout : std::max(l.c1, l.c2);
        wp = std::max(wp, wgrad_splits(M, N, B) * M * N * (size_t)l.ks);
    }
    wp = std::max(wp, wgrad_splits(D, u->cfg.unet_input_dim, B) * D * (size_t)u->cfg.unet_input_dim);
    w.wpart_floats = wp;
    w.wpart = take(wp);
    {   // total partial-sum storage if no layer re-uses another's: deferred mode while it stays below 256 MB
        size_t tot = 0, pv = 0;
        for (const Layer& l : u->layers) {
            const int KS = l.ks;
            if (l.mode == CONV_UPT) tot += wgrad_splits(l.c1, l.cout, B) * l.c1 * l.cout * (size_t)KS;
            else {
                tot += wgrad_splits(l.cout, l.c1, B) * l.cout * l.c1 * (size_t)KS;
                if (l.c2 > 0) tot += wgrad_splits(l.cout, l.c2, B) * l.cout * l.c2 * (size_t)KS;
            }
            pv += (l.epi == EPI_GN_MISH ? (size_t)3 * B : (size_t)256 + 64) * l.cout;
        }
        tot += wgrad_splits(D, u->cfg.unet_input_dim, B) * D * (size_t)u->cfg.unet_input_dim;
        if (B < 64) tot *= 4;   // (the backward programs' layers may take up to 4 x the rule's splits at small batches: MPDX_WGRAD_PROG_MUL <= 4)
        pv += (size_t)(256 + 64) * D;
        w.deferred = sw::train_deferred() && tot <= ((size_t)96 << 20);   // floats
        w.wparts = take(w.deferred ? tot : 4);
        w.pvecs = take(w.deferred ? pv : 4);
    }
    w.rpart = take((size_t)256 * 512);
    w.emb = take((size_t)B * 32); w.h1 = take((size_t)B * 128); w.temb = take((size_t)B * 32);
    w.tm = take((size_t)B * 32); w.h1m = take((size_t)B * 128);
    w.tb = take((size_t)B * u->tt_row); w.dT = take((size_t)B * u->tt_row);
    w.dtm = take((size_t)B * 32); w.dh1 = take((size_t)B * 128);
    w.zeros = take(1024);
    w.ticket = take(4);      // directly behind `zeros`: one memset clears both
    w.lossp = take(32);       // 16 doubles: the loss value's wave sums (train_loss_kernel); offsets are multiples of 4 floats: 8-byte aligned
    w.total = o;
    return w;
}

static int lg2(int v) {   // the smallest k with 2^k >= v
    int k = 0;
    while ((1 << k) < v) ++k;
    return k;
}

static int fill_geom(const Layer& l, int B, ConvArgs& a) {
    a.c1 = l.c1; a.c2 = l.c2;
    a.B = B; a.L_in = l.L_in; a.L_out = l.L_out; a.C_out = l.cout;
    a.cin_pad = l.cin_pad; a.rs = l.rs; a.gs = l.gs;
    a.Lv_out = l.Lv_out;
    a.lg_c4n = lg2(l.cin_pad / 4); a.lg_Lin = lg2(l.L_in); a.lg_Lout = lg2(l.L_out); a.lg_gs = l.gs > 0 ? lg2(l.gs) : 0;
    if ((1 << a.lg_c4n) != l.cin_pad / 4 || (1 << a.lg_Lin) != l.L_in || (1 << a.lg_Lout) != l.L_out || (l.gs > 0 && (1 << a.lg_gs) != l.gs))
        return fail(MPDX_E_INVALID, "layer %s: channel/length/group sizes must be powers of two", l.name.c_str());
    return 0;
}

// deferred reductions of one backward pass
struct Deferred {
    bool on = false;
    float* ws = nullptr;
    float* grads = nullptr;
    size_t wcur = 0, pcur = 0;   // next free float in the partial areas (offsets from ws)
    ReduceAllArgs red;
    ColsumAllArgs col;
};

// a weight-gradient GEMM ready to launch (alone, or inside bwd_pair_kernel)
struct WgradJob { WgradArgs a; dim3 grid; size_t lds; int KS; bool deferred; float* g; int n_tot, n_off, S; };

// s_div > 1 (weight gradients that run behind the chain in wgrad_multi_kernel, where ALL layers' blocks fill the GPU together): fewer batch splits per
// layer than the one-workgroup-per-CU rule of a layer on its own - the partial sums written and re-read by the reduction shrink by the same factor
static int make_wgrad(const float* A, int LA, int lda, int a_off, int M, const float* Bm, int LB, int ldb, int b_off, int N, int sb, int ob, int KS,
                      int B, float* part, float* g, int n_tot, int n_off, Deferred* df, WgradJob& j, int s_div = 1) {
    size_t S_use = wgrad_splits(M, N, B);
    if ((s_div > 1 || s_div < -1) && df && df->on) {   // (s_div < -1: MORE splits - the small batches, where a block's chain of trajectories is the launch's length)
        const size_t want = s_div > 1 ? std::max<size_t>(1, S_use / (size_t)s_div) : std::min<size_t>((size_t)B, S_use * (size_t)(-s_div));
        const int per = (int)((B + want - 1) / want);
        S_use = (size_t)((B + per - 1) / per);
    }
    if (df && df->on && df->red.n < 96) {   // this layer's partial sums get their own storage; reduced at the end of the pass
        const size_t S0 = S_use;
        part = df->ws + df->wcur;
        auto& e = df->red.e[df->red.n++];
        e.part = df->wcur; e.g = (unsigned long long)(g - df->grads); e.S = (int)S0; e.M = M; e.N = N; e.KS = KS; e.n_tot = n_tot; e.n_off = n_off;
        df->wcur += S0 * M * N * (size_t)KS;
    } else df = nullptr;
    WgradArgs& a = j.a;
    a.bias_part = nullptr; a.bias_from_b = 0;
    a.A = A; a.Bm = Bm; a.part = part;
    a.LA = LA; a.lda = lda; a.a_off = a_off; a.M = M;
    a.LB = LB; a.ldb = ldb; a.b_off = b_off; a.N = N;
    a.sb = sb; a.ob = ob; a.B = B;
    const int S = (int)S_use;
    a.b_per_split = (B + S - 1) / S;
    if (LA % 4) return fail(MPDX_E_INVALID, "wgrad: horizon %d is not a multiple of 4", LA);
    if (KS != 1 && KS != 3 && KS != 4 && KS != 5) return fail(MPDX_E_INVALID, "wgrad: %d taps", KS);
    j.lds = (size_t)(LA + LB + 4) * kWgRS * sizeof(float);
    j.grid = dim3((N + 31) / 32, (M + 31) / 32, S);
    j.KS = KS; j.deferred = df != nullptr; j.g = g; j.n_tot = n_tot; j.n_off = n_off; j.S = S;
    return 0;
}
// let a (deferred) weight-gradient job add up its convolution's bias gradient too: true if attached (else the caller runs launch_rowsum)
static bool attach_bias(WgradJob& j, Deferred* df, float* gbias, bool from_b) {
    if (!df || !df->on || !j.deferred || df->col.n >= 120) return false;
    const int C = from_b ? j.a.N : j.a.M;
    j.a.bias_part = df->ws + df->pcur;
    j.a.bias_from_b = from_b ? 1 : 0;
    auto& e = df->col.e[df->col.n++];
    e.part = df->pcur; e.out = (unsigned long long)(gbias - df->grads); e.rows = j.S; e.C = C;
    df->pcur += (size_t)j.S * C;
    return true;
}
// the reduction of a job whose partial sums are not deferred
static void finish_wgrad(const WgradJob& j, hipStream_t st) {
    if (j.deferred) return;
    const size_t per = (size_t)j.a.M * j.a.N * j.KS;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<size_t>((per + 255) / 256, 1024)), dim3(256), 0, st, (const float*)j.a.part, j.g, j.S,
                       j.a.M, j.a.N, j.KS, j.n_tot, j.n_off);
}
static void run_wgrad(const WgradJob& j, hipStream_t st) {
    switch (j.KS) {
        case 1: hipLaunchKernelGGL(wgrad_kernel<1>, j.grid, dim3(256), j.lds, st, j.a); break;
        case 3: hipLaunchKernelGGL(wgrad_kernel<3>, j.grid, dim3(256), j.lds, st, j.a); break;
        case 4: hipLaunchKernelGGL(wgrad_kernel<4>, j.grid, dim3(256), j.lds, st, j.a); break;
        default: hipLaunchKernelGGL(wgrad_kernel<5>, j.grid, dim3(256), j.lds, st, j.a); break;
    }
    finish_wgrad(j, st);
}

// two wave groups per weight-gradient block inside bwd_pair_kernel's 512-thread workgroups (train.hpp wgrad_body, ngrp = 2): shapes of the prefetching loop
static bool wgrad_two_groups(const WgradJob& j) {
    const int LA = j.a.LA, LB = j.a.LB, nr = LA >> 3;
    return (LA & 7) == 0 && LB == ((j.KS == 3 || j.KS == 4) ? 2 * LA : LA) && (nr == 1 || nr == 2 || nr == 4 || nr == 8);
}
// the LDS a job needs inside a 512-thread workgroup (bwd_pair_kernel, wgrad_multi_kernel)
static size_t wgrad_job_lds(const WgradJob& j) {
    return wgrad_two_groups(j) ? std::max(2 * j.lds, (size_t)(256 * j.KS * 4 + 256) * sizeof(float)) : j.lds;
}
// the weight-gradient blocks of a bwd_pair_kernel launch: jobs -> a.w[0 .. njobs); returns their block count and raises `lds` to what they need
static int add_pair_jobs(BwdPairArgs& a, const WgradJob* jobs, int njobs, size_t& lds) {
    int blocks = 0;
    for (int k = 0; k < njobs; ++k) {
        a.w[k] = jobs[k].a; a.ks_w[k] = jobs[k].KS;
        a.gx[k] = jobs[k].grid.x; a.gy[k] = jobs[k].grid.y;
        a.nw[k] = jobs[k].grid.x * jobs[k].grid.y * jobs[k].grid.z;
        blocks += a.nw[k];
        a.two[k] = wgrad_two_groups(jobs[k]) ? 1 : 0;
        lds = std::max(lds, wgrad_job_lds(jobs[k]));
    }
    return blocks;
}
// a launch's dynamic LDS: more than 160 KB fails, more than 64 KB raises the kernel's limit
static int fit_lds(size_t lds, const void* kern, const char* what) {
    if (lds > 160 * 1024) return fail(MPDX_E_INVALID, "%s needs %zu B of LDS", what, lds);
    return lds > 64 * 1024 ? raise_lds_limit(kern) : 0;
}

// the tile of an input-gradient convolution: the forward engine's choice, 16 rows where the layer's channels are no multiple of it (dispatch_tile's rule, k_conv.hip)
static void dgrad_tile(const Layer& dgl, int B, int& MT, int& NT) {
    choose_tile(dgl, B, MT, NT);
    if (dgl.cout % MT) MT = 16;
}
// the tiles a backward pass launched its input-gradient convolutions on, counted per convolution; gn: those among them with the GroupNorm backward of the
// Conv1dBlock below in their epilogue (EPI_GN_BWD: the tile holds NT / L whole trajectories' regions) - TrainPass::report
struct TileLog {
    int n[2][4] = {}, gn[2][4] = {};   // MT 16 / 32 x NT 16 / 32 / 64 / 128
    void add(int MT, int NT, int k, bool gn_bwd) {
        const int m = MT == 32 ? 1 : 0, c = NT == 16 ? 0 : (NT == 32 ? 1 : (NT == 64 ? 2 : 3));
        n[m][c] += k;
        if (gn_bwd) gn[m][c] += 1;
    }
};

// does bwd_pair_kernel exist for the tile the forward engine picks for this input-gradient convolution?  (levels of more than 64 positions -
// n_support_points = 128 - run one trajectory per 128-position tile: per-layer launches there)
static bool bwd_pair_has_tile(const Layer& dgl, int B) {
    int MT, NT;
    dgrad_tile(dgl, B, MT, NT);
    if (dgl.cout % MT || NT % dgl.L_out) return false;
    return (MT == 32 || MT == 16) && (NT == 64 || NT == 32 || NT == 16);
}

// dgrad convolution + the layer's weight-gradient GEMM(s) in ONE launch (bwd_pair_kernel); the jobs must use distinct partial buffers
// GN_BWD: the dgrad blocks run the EPI_GN_BWD epilogue (cd carries its operands; `dgl` then has epi = EPI_GN_MISH and the group size
// of the Conv1dBlock below, so that the tile holds whole GroupNorm regions)
// dgl2 / cd2 (optional): a second, 1x1 input-gradient convolution on the same tile behind the first one's blocks (BwdPairArgs::cd2); returns kNoPair2 (nothing
// launched) when that convolution does not fit the first one's tile.  `tiles`: the launch's tile is counted there, once per input-gradient convolution
constexpr int kNoPair2 = 99;
template <int KS_D, bool GN_BWD = false>
static int launch_bwd_pair(const Layer& dgl, ConvArgs& cd, int B, const WgradJob* jobs, int njobs, hipStream_t st, TileLog& tiles, const Layer* dgl2 = nullptr,
                           ConvArgs* cd2 = nullptr) {
    int MT, NT;
    dgrad_tile(dgl, B, MT, NT);
    if (dgl.cout % MT || NT % dgl.L_out) return fail(MPDX_E_INVALID, "layer %s: no tile for C_out=%d L=%d", dgl.name.c_str(), dgl.cout, dgl.L_out);
    if (dgl2 && (dgl2->cout % MT || dgl2->L_out != dgl.L_out || dgl2->ks != 1 || dgl2->mode != CONV_S1 || njobs > 3)) return kNoPair2;
    cd.n_tiles_n = (int)(((long)B * dgl.L_out + NT - 1) / NT);
    BwdPairArgs a;
    memset(&a, 0, sizeof(a));
    a.cd = cd;
    a.n_dgrad = (dgl.cout / MT) * cd.n_tiles_n;
    size_t lds = 0;
    if (dgl2) {
        cd2->n_tiles_n = cd.n_tiles_n;
        a.cd2 = *cd2;
        a.n_dgrad2 = (dgl2->cout / MT) * cd2->n_tiles_n;
    }
    const int total = a.n_dgrad + a.n_dgrad2 + add_pair_jobs(a, jobs, njobs, lds);
#define MPDX_BP_TILE(mt, nt)                                                                              \
    if (MT == mt && NT == nt) {                                                                           \
        lds = std::max(lds, conv_block_lds_bytes<CONV_S1, KS_D, mt, nt, 8>(cd.L_in, cd.L_out, cd.rs));      \
        if (dgl2) lds = std::max(lds, conv_block_lds_bytes<CONV_S1, 1, mt, nt, 8>(cd2->L_in, cd2->L_out, cd2->rs)); \
        auto kern = bwd_pair_kernel<KS_D, mt, nt, GN_BWD ? EPI_GN_BWD : EPI_BIAS>;                         \
        if (int rc = fit_lds(lds, (const void*)kern, "backward pair")) return rc;                         \
        hipLaunchKernelGGL(kern, dim3(total), dim3(512), lds, st, a);                                     \
        tiles.add(mt, nt, dgl2 ? 2 : 1, GN_BWD);                                                          \
        for (int k = 0; k < njobs; ++k) finish_wgrad(jobs[k], st);                                        \
        return 0;                                                                                         \
    }
    MPDX_BP_TILE(32, 64) MPDX_BP_TILE(32, 32) MPDX_BP_TILE(16, 64) MPDX_BP_TILE(16, 32) MPDX_BP_TILE(32, 16) MPDX_BP_TILE(16, 16)
#undef MPDX_BP_TILE
    return fail(MPDX_E_INVALID, "no backward-pair instantiation for tile %dx%d", MT, NT);
}

// up to three weight-gradient GEMMs that have no input-gradient convolution to ride on (layers whose input needs no gradient, final_conv[1]) in ONE
// launch: bwd_pair_kernel with n_dgrad = 0 (any instantiation: the dgrad body is never entered)
static int launch_lone_wgrads(const WgradJob* jobs, int njobs, hipStream_t st) {
    if (njobs <= 0) return 0;
    BwdPairArgs a;
    memset(&a, 0, sizeof(a));
    size_t lds = 0;
    const int total = add_pair_jobs(a, jobs, njobs, lds);
    auto kern = bwd_pair_kernel<1, 16, 16, EPI_BIAS>;
    if (int rc = fit_lds(lds, (const void*)kern, "weight-gradient launch")) return rc;
    hipLaunchKernelGGL(kern, dim3(total), dim3(512), lds, st, a);
    for (int k = 0; k < njobs; ++k) finish_wgrad(jobs[k], st);
    return 0;
}

// any number of deferred weight-gradient GEMMs in launches of up to kWgradMultiMax jobs (wgrad_multi_kernel); the longest blocks first
static int launch_wgrads_multi(std::vector<WgradJob>& jobs, hipStream_t st) {
    if (jobs.empty()) return 0;
    std::stable_sort(jobs.begin(), jobs.end(), [](const WgradJob& x, const WgradJob& y) {
        const long wx = (long)x.a.b_per_split * x.a.LA * x.KS, wy = (long)y.a.b_per_split * y.a.LA * y.KS;
        return wx > wy;
    });
    for (size_t k0 = 0; k0 < jobs.size(); k0 += kWgradMultiMax) {
        const int nj = (int)std::min<size_t>(kWgradMultiMax, jobs.size() - k0);
        WgradMultiArgs a;
        memset(&a, 0, sizeof(a));
        a.n = nj;
        size_t lds = 0;
        int total = 0;
        for (int k = 0; k < nj; ++k) {
            const WgradJob& j = jobs[k0 + k];
            if (!j.deferred) return fail(MPDX_E_INVALID, "wgrad_multi: job without its own partial-sum buffer");
            a.w[k] = j.a; a.ks[k] = (signed char)j.KS;
            a.gx[k] = (short)j.grid.x; a.gy[k] = (short)j.grid.y;
            a.start[k] = total;
            total += (int)(j.grid.x * j.grid.y * j.grid.z);
            a.two[k] = wgrad_two_groups(j) ? 1 : 0;
            lds = std::max(lds, wgrad_job_lds(j));
        }
        for (int k = nj; k <= kWgradMultiMax; ++k) a.start[k] = total;
        if (int rc = fit_lds(lds, (const void*)wgrad_multi_kernel, "weight-gradient launch")) return rc;
        hipLaunchKernelGGL(wgrad_multi_kernel, dim3(total), dim3(512), lds, st, a);
    }
    return 0;
}

// channel sums of a dense [rows][C] tensor -> out[C]
static void launch_rowsum(const float* x, size_t rows, int C, float* part, float* out, hipStream_t st, Deferred* df = nullptr) {
    const int nb = (int)std::min<size_t>(64, rows);
    const int rpb = (int)((rows + nb - 1) / nb);
    const int nblk = (int)((rows + rpb - 1) / rpb);
    if (df && df->on && df->col.n < 120) {
        part = df->ws + df->pcur;
        auto& e = df->col.e[df->col.n++];
        e.part = df->pcur; e.out = (unsigned long long)(out - df->grads); e.rows = nblk; e.C = C;
        df->pcur += (size_t)64 * C;
        hipLaunchKernelGGL(rowsum_part_kernel, dim3(nblk), dim3(256), 0, st, x, part, (int)rows, C, rpb);
        return;
    }
    hipLaunchKernelGGL(rowsum_part_kernel, dim3(nblk), dim3(256), 0, st, x, part, (int)rows, C, rpb);
    ColsumArgs c;
    memset(&c, 0, sizeof(c));
    c.part[0] = part; c.out[0] = out; c.B = nblk; c.C = C;
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64, 1), dim3(256), 0, st, c);
}

// Draw mode of the training pass (mpdx_train_draw below): the seed and the device step counter armed for a network
struct TrainRng { unsigned long long seed; const int* counter; };
static std::mutex g_train_rng_mu;
static std::unordered_map<const mpdx_unet*, TrainRng> g_train_rng;

// round 6: the dgrad launch of a ResidualTemporalBlock's blocks[1] (with the GroupNorm backward of blocks[0] in its epilogue) WAITS one layer for the block's
// residual 1x1 convolution (the next layer in backward order): its 1x1 dgrad - and at batch < 48 both layers' weight-gradient blocks - ride on the same
// launch (BwdPairArgs::cd2): one launch less per such block
struct PendingPair { bool on = false; int i_next = -1; Layer dg; ConvArgs a; WgradJob jobs[3]; int njobs = 0; };

// train_bwd_prog.hpp
struct BwdProgLayout;
static int bwd_down_applicable(const mpdx_unet* u);
static int bwd_up_applicable(const mpdx_unet* u);

// ---- one mpdx_train_loss_backward call: what its stages share, and the stages in the order the entry point runs them.  Every stage enqueues on `st`; the
// order of the launches and of the first_write / df.red / df.col / df.pcur bookkeeping is behaviour (partial-sum offsets are kernel arguments).
struct __attribute__((visibility("hidden"))) TrainPass {   // (its members are no symbols of the shared library)
    mpdx_unet* const u;
    const float* const flat;
    const float* const packed;
    const float* const packedT;
    float* const grads_flat;
    float* const ws;
    const int B;
    const hipStream_t st;
    const TrainWs w;
    const int n;         // layers
    const bool masked;   // a horizon in a power-of-two container (24, 40, 48, 96 ...): rows [H, Hc) of every activation / gradient tensor are zero

    bool eps_done = false;             // a fused forward program ran final_conv[1] too
    TimeBwdArgs tb;                    // the time conditioning's backward: filled beside the forward's arguments, launched last
    Deferred df;
    std::vector<WgradJob> lone;        // deferred weight-gradient GEMMs without a dgrad convolution to ride on: launched together behind the walk
    std::vector<int> first_consumer;   // of layer j's output: the reader that comes LAST in backward order (the lowest layer index)
    std::vector<char> du_ready;        // grd(j) already holds the gradient wrt layer j's CONVOLUTION output
    std::vector<char> written;         // grd(j) has been written in this pass (launches execute in the order they are enqueued here)
    int down_variant = 0, dn_last = 0, up_first = -1;   // the backward programs that apply (bwd_down_applicable / bwd_up_applicable): layers [0, dn_last], [up_first, n)
    bool ran_up = false, ran_down = false;
    PendingPair pend;
    TileLog tiles;                     // of the input-gradient convolutions this pass launched itself (the backward programs' layers are not among them)

    TrainPass(mpdx_unet* u_, const float* flat_, const float* packed_, const float* packedT_, float* grads_flat_, float* ws_, int B_, hipStream_t st_)
        : u(u_), flat(flat_), packed(packed_), packedT(packedT_), grads_flat(grads_flat_), ws(ws_), B(B_), st(st_), w(train_ws(u_, B_)), n((int)u_->layers.size()), masked(u_->masked()) {}

    float* xn() const { return ws + w.xn; }
    float* eps() const { return ws + w.eps; }
    float* dE() const { return ws + w.dE; }
    float* part() const { return ws + w.wpart; }   // partial sums of a weight gradient that is not deferred
    float* out(int i) const { return ws + w.out0 + (size_t)i * w.slotB; }
    float* pre(int i) const { return ws + w.pre0 + (size_t)i * w.slotB; }
    float* grd(int i) const { return ws + w.grad0 + (size_t)i * w.slotB; }
    const float* tensor(int li) const { return li == -1 ? xn() : (li < 0 ? nullptr : out(li)); }
    float* gflat(int pidx) const { return grads_flat + u->params[pidx].foff; }
    int goff(const float* p) const { return (int)(p - ws); }
    // (no memset of the gradient buffers: the first writer of each in the backward pass stores, the later ones add)
    bool first_write(int j) { const bool f = !written[j]; written[j] = 1; return f; }
    bool fused_fwd() const { return fused_mask(B) != 0u && (w.total < ((size_t)1 << 31)); }

    // forward, every layer's output (and GroupNorm input) kept
    int forward_time_qsample(const float* x_start, const float* noise, const long long* t_dev, const float* sqrt_ac, const float* sqrt_1mac, const float* freqs16,
                             const float* hard_start, const float* hard_goal, int T);
    int forward_layers();
    int forward_fused_segment(const mpdx_unet::Fused& f);
    int layer_args(int li, ConvArgs& a) const;
    int loss_and_seed_gradient(const float* target, const float* weights_hd, const float* hard_start, const float* hard_goal, int l1, float loss_scale, float* loss_out);
    // backward
    void begin_backward();
    int backward_final_conv1();
    int backward_walk();
    int run_down_program();   // train_bwd_prog.hpp
    int run_up_program();
    BwdArgs prog_args(const BwdProgLayout& lay) const;
    void prog_gn_part(int li, BwdOp& op);
    int backward_layer(int i);
    int gn_backward(int i, const float*& dy);
    int layer_wgrads(int i, const float* dy, int sdiv, WgradJob* jobs, int& njobs);
    int place_wgrads(int i, const float* dy, WgradJob* jobs, int& njobs, bool& paired);
    int input_gradient(int i, const float* dy, const WgradJob* jobs, int njobs, bool paired);
    int gn_epilogue_layer(int i, bool paired) const;
    int dgrad_with_gn_epilogue(int i, int j, ConvArgs& a, const WgradJob* jobs, int njobs);
    int dgrad_paired(const Layer& dgl, ConvArgs& a, const WgradJob* jobs, int njobs);
    int flush_pending();
    size_t colsum3(const Layer& l);
    void report() const;
    int late_wgrads();
    void finish_reductions();
    void backward_time();
};

// the time MLP of every sample, q_sample with its hard conditions and the pass's zero words (the zero bias of the dgrad convolutions + the time backward's
// ticket) as per-sample side jobs of ONE launch, time_train_fwd_kernel: round 3 spent a memset and a launch on them
inline int TrainPass::forward_time_qsample(const float* x_start, const float* noise, const long long* t_dev, const float* sqrt_ac, const float* sqrt_1mac,
                                           const float* freqs16, const float* hard_start, const float* hard_goal, int T) {
    const mpdx_unet_cfg& c = u->cfg;
    TimeTrainArgs ta;
    memset(&ta, 0, sizeof(ta));
    memset(&tb, 0, sizeof(tb));
    ta.flat = flat; ta.t = t_dev; ta.freqs = freqs16;
    ta.emb = ws + w.emb; ta.h1 = ws + w.h1; ta.temb = ws + w.temb; ta.tb = ws + w.tb;
    ta.tm = ws + w.tm; ta.h1m = ws + w.h1m;
    ta.w1 = u->params[u->pidx.at("time_mlp.encoder.1.weight")].foff; ta.b1 = u->params[u->pidx.at("time_mlp.encoder.1.bias")].foff;
    ta.w3 = u->params[u->pidx.at("time_mlp.encoder.3.weight")].foff; ta.b3 = u->params[u->pidx.at("time_mlp.encoder.3.bias")].foff;
    ta.row = u->tt_row; ta.nblk = (int)u->tt_w.size();
    if (ta.nblk > 40 || c.time_emb_dim != 32) return fail(MPDX_E_INVALID, "time MLP shape unsupported by the training kernels");
    for (int i = 0; i < ta.nblk; ++i) {
        ta.woff[i] = u->params[u->tt_w[i]].foff; ta.boff[i] = u->params[u->tt_b[i]].foff;
        ta.cout[i] = u->tt_cout[i]; ta.toff[i] = u->tt_off[i];
    }
    ta.x0 = x_start; ta.noise = noise; ta.sqrt_ac = sqrt_ac; ta.sqrt_1mac = sqrt_1mac;
    ta.hs = hard_start; ta.hg = hard_goal; ta.xn = xn(); ta.zero_words = ws + w.zeros; ta.n_zero = 1024 + 4;
    ta.H = c.n_support_points; ta.D = c.state_dim; ta.T = T;
    {
        std::lock_guard<std::mutex> lk(g_train_rng_mu);
        auto it = g_train_rng.find(u);
        if (it != g_train_rng.end()) {
            if ((ta.H * ta.D) & 3) return fail(MPDX_E_INVALID, "draw mode: H * D = %d is not a multiple of 4", ta.H * ta.D);
            ta.rng_seed = it->second.seed; ta.rng_counter = it->second.counter;
            ta.t_out = const_cast<long long*>(t_dev); ta.noise_out = const_cast<float*>(noise);
        }
    }
    ta.B = B; ta.packed = const_cast<float*>(packed); ta.jobs = nullptr; ta.n_jobs = 0;
    ta.Hc = masked ? u->Hc : 0;
    // the fused forward programs' weight streams: re-assembled by side blocks of this launch (the pack launch before it wrote `packed`)
    if (fused_fwd() && sw::train_restream_ride()) {
        const void* jb = nullptr;
        int nj = 0;
        if (int rc = claim_fused_stream_jobs(u, packed, &jb, &nj)) return rc;
        ta.jobs = (const CopyJobDev*)jb; ta.n_jobs = nj;
    }
    hipLaunchKernelGGL(time_train_fwd_kernel, dim3(2 * B + kRestreamBlocksPerJob * ta.n_jobs), dim3(512), 0, st, ta);
    tb.flat = flat; tb.grad = grads_flat; tb.dT = ws + w.dT; tb.emb = ta.emb; tb.h1 = ta.h1; tb.temb = ta.temb; tb.tm = ta.tm; tb.h1m = ta.h1m;
    tb.dtm = ws + w.dtm; tb.dh1 = ws + w.dh1; tb.ticket = (unsigned*)(ws + w.ticket);
    if (ta.row > kTimeBwdMaxRow)   // time_bwd_all_kernel carves dTs | roff | red out of LDS at fixed offsets of kTimeBwdMaxRow
        return fail(MPDX_E_INVALID, "time table row of %d floats (the training kernels take %d)", ta.row, kTimeBwdMaxRow);
    tb.w1 = ta.w1; tb.b1 = ta.b1; tb.w3 = ta.w3; tb.b3 = ta.b3;
    tb.B = B; tb.row = ta.row; tb.nblk = ta.nblk;
    for (int i = 0; i < ta.nblk; ++i) { tb.woff[i] = ta.woff[i]; tb.boff[i] = ta.boff[i]; tb.cout[i] = ta.cout[i]; tb.toff[i] = ta.toff[i]; }
    return 0;
}

inline int TrainPass::layer_args(int li, ConvArgs& a) const {
    const Layer& l = u->layers[li];
    const auto& t = u->tl[li];
    memset(&a, 0, sizeof(a));
    if (int rc = fill_geom(l, B, a)) return rc;
    a.src1 = tensor(t.src1_l); a.src2 = tensor(t.src2_l);
    a.wp = packed + u->params[l.w].off;
    a.bias = packed + u->params[l.b].off;
    a.gamma = l.gamma >= 0 ? packed + u->params[l.gamma].off : nullptr;
    a.beta = l.beta >= 0 ? packed + u->params[l.beta].off : nullptr;
    if (l.tb_off >= 0) { a.tbias = ws + w.tb + l.tb_off; a.tb_stride = u->tt_row; }
    a.res = tensor(t.res_l);
    a.dst = out(li);
    a.pre = l.epi == EPI_GN_MISH ? pre(li) : nullptr;
    return 0;
}

// one fused level program of the planning path, in the variant that also keeps every op's output and GroupNorm input (FusedArgs::save)
inline int TrainPass::forward_fused_segment(const mpdx_unet::Fused& f) {
    if (int rc = ensure_fused_streams(u, packed, st)) return rc;
    FusedArgs a = f.tmpl;
    a.packed = packed;
    a.tt_row = ws + w.tb; a.tt_stride = u->tt_row;
    const auto& t0 = u->tl[f.first];
    a.gsrc1 = tensor(t0.src1_l); a.gsrc2 = tensor(t0.src2_l);
    a.gsrc3 = f.in3_consumer >= 0 ? tensor(u->tl[f.in3_consumer].src2_l) : a.gsrc1;
    a.B = B;
    a.save = ws;
    int k = 0;
    for (; k < (int)f.op_layer.size(); ++k) {
        const int li = f.op_layer[k];
        a.ops[k].gdst = -1;   // nothing reads the planning path's slots here
        a.ops[k].save_out = (int)(w.out0 + (size_t)li * w.slotB);
        a.ops[k].save_pre = u->layers[li].epi == EPI_GN_MISH ? (int)(w.pre0 + (size_t)li * w.slotB) : -1;
    }
    for (; k < a.nops; ++k) { a.ops[k].save_out = -1; a.ops[k].save_pre = -1; }
    if (f.has_final) {   // final_conv[1] -> eps, no DDPM step
        a.out = eps(); a.fmode = 0; a.n_per_ctx = B;
        eps_done = true;
    }
    return launch_fused_args(f, a, B, st, true);
}

// the fused level programs for the outer levels, one launch per layer for the rest
inline int TrainPass::forward_layers() {
    const bool fused = fused_fwd();
    for (int i = 0; i < n; ++i) {
        const int seg = fused ? u->owner[i] : -1;
        if (seg >= 0 && ((fused_mask(B) >> seg) & 1u) && fused_save_variant(u->fused[seg])) {
            if (i != u->fused[seg].first) continue;   // the segment's launch covers layers [first, first + count)
            if (int rc = forward_fused_segment(u->fused[seg])) return rc;
            continue;
        }
        const Layer& l = u->layers[i];
        ConvArgs a;
        if (int rc = layer_args(i, a)) return rc;
        // blocks[0] and the same block's residual 1x1 convolution (the next layer; both read the block input) as ONE launch - the planning path's conv_pair_kernel
        // (round 6: two launches of ~4.8 us less per pass on the four-level network)
        int MT = 0, NT = 0;
        if (!masked && i + 1 < n && !(fused && u->owner[i + 1] >= 0 && ((fused_mask(B) >> u->owner[i + 1]) & 1u)) && u->tl[i + 1].src1_l == u->tl[i].src1_l &&
            u->tl[i + 1].src2_l == u->tl[i].src2_l && pair_tile(l, u->layers[i + 1], B, MT, NT)) {
            ConvArgs a2;
            if (int rc = layer_args(i + 1, a2)) return rc;
            a.n_tiles_n = a2.n_tiles_n = (int)(((long)B * l.L_out + NT - 1) / NT);
            const int rc = launch_conv_pair(MT, NT, a, a2, l, u->layers[i + 1], st);
            if (rc < 0) return rc;
            if (rc == 1) { ++i; continue; }
        }
        if (int rc = launch_conv_layer(l, a, B, st)) return rc;
    }
    return 0;
}

// final_conv[1] -> eps (the network output) unless a fused program has done it; then hard conditions, the loss value, dE and the gradient wrt
// final_conv[0]'s output (back through final_conv[1]) in one launch
inline int TrainPass::loss_and_seed_gradient(const float* target, const float* weights_hd, const float* hard_start, const float* hard_goal, int l1, float loss_scale,
                                             float* loss_out) {
    const int H = u->cfg.n_support_points, D = u->cfg.state_dim, Hc = u->Hc;
    FinalArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.h = out(n - 1);
    fa.w = packed + u->params[u->pidx.at("final_conv.1.weight")].off;
    fa.bias = packed + u->params[u->pidx.at("final_conv.1.bias")].off;
    fa.out = eps(); fa.mode = 0; fa.n_per_ctx = 1;
    fa.B = B; fa.H = H; fa.D = D; fa.C = u->cfg.unet_input_dim;
    fa.Hc = masked ? Hc : 0;
    if (!eps_done) launch_final_step(fa, st);
    {   // train_loss_kernel: state_dim <= 16 in its plain form (padded containers, odd widths), <= 32 in the LDS-staged form (1024 % C == 0, D C <= 1024)
        const bool staged = !masked && fa.C > 0 && 1024 % fa.C == 0 && 1024 / fa.C <= 64 && D * fa.C <= 1024 && (1024 / fa.C) * D <= 1024;
        if (fa.C < D || D > 32 || (D > 16 && !staged && !masked))   // (the padded-container form loops over d: any D)
            return fail(MPDX_E_INVALID, "training: unet_input_dim %d / state_dim %d (the loss kernel takes state_dim <= 32 <= unet_input_dim)", fa.C, D);
    }
    const size_t tot = (size_t)B * Hc * fa.C;
    hipLaunchKernelGGL(train_loss_kernel, dim3((unsigned)std::min<size_t>((tot + 1023) / 1024, 1024) + 16), dim3(1024), 0, st, (const float*)eps(), target, weights_hd,
                       hard_start, hard_goal, l1, loss_scale, dE(), flat + u->params[u->pidx.at("final_conv.1.weight")].foff, grd(n - 1),
                       B, H, D, fa.C, loss_out, (double*)(ws + w.lossp), (unsigned*)(ws + w.ticket) + 1, masked ? Hc : 0);   // (ticket word 1: zeroed by the pass's first launch)
    return 0;
}

// the bookkeeping of the backward pass, and which backward programs apply
inline void TrainPass::begin_backward() {
    df.on = w.deferred; df.ws = ws; df.grads = grads_flat; df.wcur = w.wparts; df.pcur = w.pvecs;
    df.red.ws = ws; df.red.grad = grads_flat; df.red.n = 0;
    df.col.ws = ws; df.col.grad = grads_flat; df.col.n = 0;
    // A Conv1dBlock j whose output feeds exactly one k5 convolution i (blocks[0] -> blocks[1] of a ResidualTemporalBlock) gets its
    // Mish + GroupNorm backward as the EPILOGUE of i's input-gradient convolution (EPI_GN_BWD): one launch less per residual block.
    // With several consumers the LAST one in backward order (the lowest layer index) carries the epilogue; the others have added
    // their gradients to grd(j) by then.
    first_consumer.assign(n, n);
    for (int i = n - 1; i >= 0; --i)
        for (int sl : {u->tl[i].src1_l, u->tl[i].src2_l, u->tl[i].res_l})
            if (sl >= 0) first_consumer[sl] = i;
    du_ready.assign(n, 0);
    written.assign(n, 0);
    written[n - 1] = 1;   // train_loss_kernel
    const int prog_env = sw::train_bwd_prog();   // (2: the down program only)
    const bool progs_ok = prog_env != 0 && df.on && !masked && B <= sw::train_bwd_prog_max_b() && w.total < ((size_t)1 << 31);
    down_variant = progs_ok ? bwd_down_applicable(u) : 0;
    dn_last = down_variant == 3 ? 20 : (down_variant == 2 ? 16 : 17);
    up_first = (progs_ok && prog_env != 2) ? bwd_up_applicable(u) : -1;
}

// a Conv1dBlock's gamma / beta / bias gradients: three column-sum entries over B partial-sum rows each, carved from the partial area; returns where the rows start
inline size_t TrainPass::colsum3(const Layer& l) {
    const size_t at = df.pcur;
    const int prm[3] = {l.gamma, l.beta, l.b};
    for (int k = 0; k < 3; ++k) {
        auto& e = df.col.e[df.col.n++];
        e.part = at + (size_t)k * B * l.cout; e.out = u->params[prm[k]].foff; e.rows = B; e.C = l.cout;
    }
    df.pcur += (size_t)3 * B * l.cout;
    return at;
}

// final_conv[1]: weight and bias gradient (grd(n - 1) = dE W was written by train_loss_kernel)
inline int TrainPass::backward_final_conv1() {
    const int C = u->cfg.unet_input_dim, D = u->cfg.state_dim, Hc = u->Hc;
    const int wi = u->pidx.at("final_conv.1.weight"), bi = u->pidx.at("final_conv.1.bias");
    const size_t rows = (size_t)B * Hc;   // (dE in the container layout: its rows behind the horizon are zero)
    WgradJob fj;
    if (int rc = make_wgrad(dE(), Hc, D, 0, D, out(n - 1), Hc, C, 0, C, 1, 0, 1, B, part(), gflat(wi), C, 0, &df, fj)) return rc;
    const bool fb = attach_bias(fj, &df, gflat(bi), false);
    if (fj.deferred) lone.push_back(fj);   // rides with the other GEMMs that have no dgrad convolution (one launch behind the walk)
    else run_wgrad(fj, st);
    if (!fb) launch_rowsum(dE(), rows, D, ws + w.rpart, gflat(bi), st, &df);
    return 0;
}

inline int TrainPass::flush_pending() {
    if (!pend.on) return 0;
    pend.on = false;
    return launch_bwd_pair<5, true>(pend.dg, pend.a, B, pend.jobs, pend.njobs, st, tiles);
}

// the layers from final_conv[0] down to the first: a whole-trajectory program where one applies, else the per-layer step
inline int TrainPass::backward_walk() {
    for (int i = n - 1; i >= 0; --i) {
        if (pend.on && i != pend.i_next)
            if (int rc = flush_pending()) return rc;
        if (up_first >= 0 && i == n - 1) {
            const int rc = run_up_program();
            if (rc < 0 || rc > 1) return rc;
            if (rc == 0) { ran_up = true; i = up_first; continue; }   // layers [up_first, n) are done: on with the layer below
        }
        if (down_variant != 0 && i == dn_last) {
            const int rc = run_down_program();
            if (rc < 0 || rc > 1) return rc;
            if (rc == 0) { ran_down = true; break; }   // layers [0, dn_last] are done
        }
        if (int rc = backward_layer(i)) return rc;
    }
    return flush_pending();
}

inline int TrainPass::backward_layer(int i) {
    const Layer& l = u->layers[i];
    float* gy = grd(i);
    if (!written[i]) {   // nothing downstream of this layer carries a gradient: it is zero
        if (sw::debug_train()) fprintf(stderr, "[mpdx] backward: layer %d %s has no gradient-carrying consumer (zeroed)\n", i, l.name.c_str());
        HIP_TRY(hipMemsetAsync(gy, 0, w.slotB * sizeof(float), st));
        written[i] = 1;
    }
    const float* dy = gy;   // gradient wrt the convolution output (after the GroupNorm/Mish backward for Conv1dBlocks)
    if (l.epi == EPI_GN_MISH && !du_ready[i])
        if (int rc = gn_backward(i, dy)) return rc;
    // weight gradient(s) and input gradient: everything below depends only on dy
    WgradJob jobs[2];
    int njobs = 0;
    bool paired = false;
    if (int rc = place_wgrads(i, dy, jobs, njobs, paired)) return rc;
    if (u->tl[i].need_dgrad) return input_gradient(i, dy, jobs, njobs, paired);
    return 0;
}

// Mish + GroupNorm backward of Conv1dBlock `i` as its own launch (no consumer carries it in its epilogue); dy: where it left dU
inline int TrainPass::gn_backward(int i, const float*& dy) {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    float* gy = grd(i);
    GnBwdArgs g;
    memset(&g, 0, sizeof(g));
    if (t.res_l >= 0) { g.gres = grd(t.res_l); g.gres_store = first_write(t.res_l) ? 1 : 0; }
    g.gy = gy; g.pre = pre(i); g.gamma = flat + u->params[l.gamma].foff; g.beta = flat + u->params[l.beta].foff;
    g.du = ws + w.dU;
    g.pg = ws + w.pvec; g.pb = g.pg + (size_t)B * 512; g.pbias = g.pb + (size_t)B * 512;
    const bool dcol = df.on && df.col.n + 3 <= 120;
    if (dcol) { g.pg = ws + colsum3(l); g.pb = g.pg + (size_t)B * l.cout; g.pbias = g.pb + (size_t)B * l.cout; }
    if (l.tb_off >= 0) { g.dT = ws + w.dT + l.tb_off; g.dT_stride = u->tt_row; }
    g.B = B; g.L = l.L_out; g.C = l.cout; g.gs = l.gs; g.n_groups = l.cout / l.gs;
    g.lg_gs = lg2(l.gs);
    if (l.cout > 512) return fail(MPDX_E_INVALID, "layer %s: more than 512 channels", l.name.c_str());
    const int re = l.gs * l.L_out, regions = B * g.n_groups;
    const dim3 ggrid((regions + 3) / 4);
    g.Lv = l.Lv_out;
    const bool mrows = l.Lv_out > 0 && l.Lv_out < l.L_out;   // a padded container: the general kernel carries the row mask
    // du IN PLACE for the two kernels whose body allows it (a lane reads its elements before it writes them): grd(i) outlives the pass, the shared
    // dU scratch does not - so this layer's weight gradients can run behind the chain too (dy == gy in place_wgrads).  Round 6: the one 256 -> 256 layer whose
    // GroupNorm backward is its own launch kept its weight-gradient blocks riding on its dgrad launch - 22.6 us against its six siblings' 12.5 at batch 128
    if (!mrows && (re == 256 || re == 128)) g.du = gy;
    if (re == 256 && !mrows) hipLaunchKernelGGL(gn_mish_bwd_kernel<4>, ggrid, dim3(256), 0, st, g);
    else if (re == 128 && !mrows) hipLaunchKernelGGL(gn_mish_bwd_kernel<2>, ggrid, dim3(256), 0, st, g);
    else if (re == 256 && l.gs >= 4) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<4, 1>), ggrid, dim3(256), 0, st, g);
    else if (re == 128 && l.gs >= 2) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<2, 1>), ggrid, dim3(256), 0, st, g);
    // horizons other than 64 (power-of-two containers 16 ... 128): regions of 64 / 512 / 1024 / 2048 elements
    else if (re == 64) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<1, 1>), ggrid, dim3(256), 0, st, g);
    else if (re == 512 && l.gs >= 4) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<4, 2>), ggrid, dim3(256), 0, st, g);
    else if (re == 1024 && l.gs >= 4) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<4, 4>), ggrid, dim3(256), 0, st, g);
    else if (re == 2048 && l.gs >= 4) hipLaunchKernelGGL((gn_mish_bwd_gen_kernel<4, 8>), ggrid, dim3(256), 0, st, g);
    else return fail(MPDX_E_INVALID, "layer %s: GroupNorm region of %d elements (group of %d channels)", l.name.c_str(), re, l.gs);
    if (!dcol) {
        ColsumArgs cs;
        memset(&cs, 0, sizeof(cs));
        cs.part[0] = g.pg; cs.out[0] = gflat(l.gamma);
        cs.part[1] = g.pb; cs.out[1] = gflat(l.beta);
        cs.part[2] = g.pbias; cs.out[2] = gflat(l.b);
        cs.B = B; cs.C = l.cout;
        hipLaunchKernelGGL(colsum_kernel, dim3((l.cout + 63) / 64, 3), dim3(256), 0, st, cs);
    }
    dy = g.du;
    return 0;
}

// the weight-gradient GEMM(s) of layer `i` on dU = dy: one job, two where the layer reads a channel concat; a ConvTranspose swaps the operands
inline int TrainPass::layer_wgrads(int i, const float* dy, int sdiv, WgradJob* jobs, int& njobs) {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    const int Cin = l.c1 + l.c2;
    float* gw = gflat(l.w);
    if (l.mode == CONV_UPT)
        return make_wgrad(tensor(t.src1_l), l.L_in, l.c1, 0, l.c1, dy, l.L_out, l.cout, 0, l.cout, 2, -1, 4, B, part(), gw, l.cout, 0, &df, jobs[njobs++], sdiv);
    const int sb = l.mode == CONV_DOWN ? 2 : 1, ob = l.mode == CONV_DOWN ? -1 : -(l.ks / 2);
    if (int rc = make_wgrad(dy, l.L_out, l.cout, 0, l.cout, tensor(t.src1_l), l.L_in, l.c1, 0, l.c1, sb, ob, l.ks, B, part(), gw, Cin, 0, &df, jobs[njobs++], sdiv)) return rc;
    if (l.c2 > 0)
        if (int rc = make_wgrad(dy, l.L_out, l.cout, 0, l.cout, tensor(t.src2_l), l.L_in, l.c2, 0, l.c2, sb, ob, l.ks, B, part(), gw, Cin, l.c1, &df, jobs[njobs++], sdiv)) return rc;
    return 0;
}

// builds layer i's weight-gradient jobs and decides where they run: RIDING on the layer's input-gradient launch (they stay in `jobs`; `paired`: that launch
// is bwd_pair_kernel), LATE (behind the chain, with everybody else's in wgrad_multi_kernel), LONE (no input-gradient launch: three per launch) or at once
inline int TrainPass::place_wgrads(int i, const float* dy, WgradJob* jobs, int& njobs, bool& paired) {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    const float* gy = grd(i);
    // round 6 (MPDX_TRAIN_WGRAD_LATE, dev A/B switch): a layer's weight gradients leave the chain when their dU operand outlives the pass - it does
    // whenever it sits in the layer's own gradient slot (grd(i): written once, never recycled), not in the shared dU scratch of an un-fused
    // GroupNorm backward - and run with everybody else's in wgrad_multi_kernel behind the chain
    const int late_env = sw::train_wgrad_late();   // -1: by batch (measured: batch 32 no gain, 128 -3 %, 512 -4.6 %)
    const bool late_on = late_env < 0 ? B >= 48 : late_env != 0;   // (batch 48: 0.58 -> 0.543 ms, batch 32: within noise: profiles/r06_train_b32_late_ab.txt)
    // will this layer's weight gradients run behind the chain (decided below, once the jobs exist: the same conditions)?  Then with fewer batch splits.
    const bool late_cand = late_on && t.need_dgrad && df.on && df.red.n + 2 <= 96 && bwd_pair_has_tile(t.dg, B) && dy == gy;
    if (int rc = layer_wgrads(i, dy, late_cand ? wgrad_late_sdiv(B) : 1, jobs, njobs)) return rc;
    // bias gradient = channel sums of dY: rides on the first weight-gradient job, else its own two launches
    if (l.epi != EPI_GN_MISH && !attach_bias(jobs[0], &df, gflat(l.b), l.mode == CONV_UPT))
        launch_rowsum(gy, (size_t)B * l.L_out, l.cout, ws + w.rpart, gflat(l.b), st, &df);
    // one launch for all of them needs every job on its own partial buffer (the deferred mode)
    paired = t.need_dgrad && jobs[0].deferred && (njobs == 1 || jobs[1].deferred) && bwd_pair_has_tile(t.dg, B);
    if (late_on && paired && dy == gy) {
        for (int k = 0; k < njobs; ++k) lone.push_back(jobs[k]);
        njobs = 0;
    }
    if (!paired)
        for (int k = 0; k < njobs; ++k) {
            if (!t.need_dgrad && jobs[k].deferred) lone.push_back(jobs[k]);
            else run_wgrad(jobs[k], st);
        }
    return 0;
}

// the layer j whose Mish + GroupNorm backward runs in the epilogue of layer i's input-gradient convolution (EPI_GN_BWD), or -1
inline int TrainPass::gn_epilogue_layer(int i, bool paired) const {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    const int j = t.src1_l;
    if (!(paired && !masked && sw::train_gn_fuse() && ((l.mode == CONV_S1 && l.ks == 5) || (l.mode == CONV_DOWN && t.dg.ks == 3)) && l.c2 == 0 && j >= 0 && j != n - 1 && first_consumer[j] == i && t.res_l != j &&
          !(down_variant != 0 && j == dn_last) &&   // (the down program's first op is that layer's GroupNorm backward: it wants G, not dU)
          u->layers[j].epi == EPI_GN_MISH && u->layers[j].cout == l.c1 && df.on && df.col.n + 3 <= 120))
        return -1;
    const Layer& lj = u->layers[j];
    const int re = lj.gs * lj.L_out;
    return (re == 256 || re == 128) && lj.L_out == t.dg.L_out ? j : -1;
}

// layer i's input-gradient convolution with the GroupNorm backward of the Conv1dBlock j below in its epilogue: grd(j) receives dU of layer j
inline int TrainPass::dgrad_with_gn_epilogue(int i, int j, ConvArgs& a, const WgradJob* jobs, int njobs) {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    const Layer& lj = u->layers[j];
    Layer dg2 = t.dg;
    dg2.epi = EPI_GN_MISH; dg2.gs = lj.gs;
    a.dst = grd(j); a.dst2 = nullptr; a.c_split = 0;   // (a.accum bit 0 as the caller set it: the other consumers' gradients are in grd(j))
    if (u->tl[j].res_l >= 0) { a.bw_gres = grd(u->tl[j].res_l); a.bw_gres_store = first_write(u->tl[j].res_l) ? 1 : 0; }
    a.res = pre(j);
    a.gamma = flat + u->params[lj.gamma].foff; a.beta = flat + u->params[lj.beta].foff;
    a.gs = lj.gs; a.lg_gs = lg2(lj.gs);
    a.bw_pg = ws + colsum3(lj); a.bw_pb = a.bw_pg + (size_t)B * lj.cout; a.bw_pbias = a.bw_pb + (size_t)B * lj.cout;
    if (lj.tb_off >= 0) { a.bw_dT = ws + w.dT + lj.tb_off; a.bw_dT_stride = u->tt_row; }
    du_ready[j] = 1;
    // is the next layer in backward order this block's residual 1x1 convolution?  Then this launch waits for it (PendingPair)
    bool defer = false;
    if (dg2.ks == 5 && i >= 1 && t.res_l == i - 1 && njobs <= 1) {
        const Layer& r = u->layers[i - 1];
        defer = r.mode == CONV_S1 && r.ks == 1 && r.epi == EPI_BIAS && u->tl[i - 1].need_dgrad && r.L_out == l.L_out && !(down_variant != 0 && i - 1 <= dn_last);
    }
    if (defer) {
        pend.on = true; pend.i_next = i - 1; pend.dg = dg2; pend.a = a; pend.njobs = njobs;
        for (int k = 0; k < njobs; ++k) pend.jobs[k] = jobs[k];
        return 0;
    }
    return dg2.ks == 5 ? launch_bwd_pair<5, true>(dg2, a, B, jobs, njobs, st, tiles) : launch_bwd_pair<3, true>(dg2, a, B, jobs, njobs, st, tiles);
}

// an input-gradient convolution with the layer's riding weight-gradient blocks (bwd_pair_kernel); a residual 1x1's rides on the waiting blocks[1] launch
inline int TrainPass::dgrad_paired(const Layer& dgl, ConvArgs& a, const WgradJob* jobs, int njobs) {
    if (pend.on && dgl.ks == 1 && pend.njobs + njobs <= 3) {   // the residual 1x1's dgrad (and weight-gradient blocks) ride on the waiting blocks[1] launch
        WgradJob all[3];
        int na = 0;
        for (int k = 0; k < pend.njobs; ++k) all[na++] = pend.jobs[k];
        for (int k = 0; k < njobs; ++k) all[na++] = jobs[k];
        const int rc = launch_bwd_pair<5, true>(pend.dg, pend.a, B, all, na, st, tiles, &dgl, &a);
        if (rc != kNoPair2) {
            pend.on = false;
            return rc;
        }
    }
    if (int rc = flush_pending()) return rc;
    if (dgl.ks == 5) return launch_bwd_pair<5>(dgl, a, B, jobs, njobs, st, tiles);
    if (dgl.ks == 3) return launch_bwd_pair<3>(dgl, a, B, jobs, njobs, st, tiles);
    return launch_bwd_pair<1>(dgl, a, B, jobs, njobs, st, tiles);
}

// layer i's input-gradient convolution on dU = dy, stored to / added into the gradient buffer(s) of the layer's input(s)
inline int TrainPass::input_gradient(int i, const float* dy, const WgradJob* jobs, int njobs, bool paired) {
    const Layer& l = u->layers[i];
    const auto& t = u->tl[i];
    const Layer& dgl = t.dg;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = fill_geom(dgl, B, a)) return rc;
    a.src1 = dy;
    if (l.mode == CONV_DOWN) a.stuff = 1;   // the staging reads dy zero-stuffed (ConvArgs::stuff)
    a.wp = packedT + t.dgrad_woff;
    a.bias = ws + w.zeros;
    if (l.mode == CONV_UPT) {   // even output rows straight into the gradient of the layer's input (ConvArgs::decim); c2 == 0, so src1_l >= 0 (need_dgrad)
        a.dst = grd(t.src1_l); a.decim = 1;
        if (!first_write(t.src1_l)) a.accum |= 1;
    } else {   // added straight into the gradient buffer(s) of the layer's input(s)
        a.dst = t.src1_l >= 0 ? grd(t.src1_l) : nullptr;
        if (t.src1_l >= 0 && !first_write(t.src1_l)) a.accum |= 1;
        if (l.c2 > 0) {
            a.c_split = l.c1; a.dst2 = t.src2_l >= 0 ? grd(t.src2_l) : nullptr;
            if (t.src2_l >= 0 && !first_write(t.src2_l)) a.accum |= 2;
        }
    }
    const int j = gn_epilogue_layer(i, paired);
    if (j >= 0) {
        if (int rc = dgrad_with_gn_epilogue(i, j, a, jobs, njobs)) return rc;
    } else if (paired) {
        if (int rc = dgrad_paired(dgl, a, jobs, njobs)) return rc;
    } else {   // the un-paired launch: launch_conv_layer picks the tile by the same rule
        if (int rc = launch_conv_layer(dgl, a, B, st)) return rc;
        int MT, NT;
        dgrad_tile(dgl, B, MT, NT);
        tiles.add(MT, NT, 1, false);
    }
    return 0;
}

inline void TrainPass::report() const {
    if (!sw::debug_train()) return;
    // (tests/test_gpu_train.py reads the first line: the programs must RUN on both networks the reference trains)
    fprintf(stderr, "[mpdx] backward programs: up %d (layers [%d, %d)), down %d (variant %d, layers [0, %d])\n", ran_up ? 1 : 0, up_first, n, ran_down ? 1 : 0, down_variant, dn_last);
    fprintf(stderr, "[mpdx] backward: %zu weight-gradient jobs behind the chain\n", lone.size());
    // (tests/test_gpu_train_batches.py reads this one: the MTxNT tiles of the input-gradient convolutions the pass launched per layer or paired, xCOUNT each;
    //  gn K: K of them ran the GroupNorm backward in their epilogue)
    std::string s;
    const int mts[2] = {16, 32}, nts[4] = {16, 32, 64, 128};
    for (int m = 1; m >= 0; --m)
        for (int k = 3; k >= 0; --k)
            if (tiles.n[m][k])
                s += " " + std::to_string(mts[m]) + "x" + std::to_string(nts[k]) + " x" + std::to_string(tiles.n[m][k]) + " (gn " + std::to_string(tiles.gn[m][k]) + ")";
    fprintf(stderr, "[mpdx] backward: input-gradient tiles:%s\n", s.empty() ? " none" : s.c_str());
}

// the collected weight-gradient GEMMs: all in one launch, or (MPDX_TRAIN_WGRAD_MULTI=0) three per launch
inline int TrainPass::late_wgrads() {
    if (sw::train_wgrad_multi()) return launch_wgrads_multi(lone, st);
    for (size_t k = 0; k < lone.size(); k += 3)
        if (int rc = launch_lone_wgrads(lone.data() + k, (int)std::min<size_t>(3, lone.size() - k), st)) return rc;
    return 0;
}

// every deferred partial sum -> its gradient: one launch for the weight gradients and (riding as side blocks) the column sums
inline void TrainPass::finish_reductions() {
    if (df.red.n) {
        int blocks = 0;
        for (int k = 0; k < df.red.n; ++k) {
            df.red.cstart[k] = blocks;
            auto& e = df.red.e[k];
            e.zsl = reduce_zsl(e);
            const size_t opb = 1024 / (size_t)std::max(1, e.zsl);   // outputs per block
            blocks += (int)(((size_t)e.M * e.N * e.KS + opb - 1) / opb);
        }
        df.red.cstart[df.red.n] = blocks;
        if (df.col.n && sw::train_reduce_join()) {   // the column sums ride on the same launch (side blocks behind the reduction's)
            ReduceColsumArgs rc;   // (8 KB of kernel arguments; the launch copies them)
            rc.red = df.red; rc.col = df.col; rc.n_red_blocks = blocks;
            hipLaunchKernelGGL(wgrad_reduce_colsum_kernel, dim3(blocks + 2 * df.col.n), dim3(256), 0, st, rc);
            df.col.n = 0;
        } else hipLaunchKernelGGL(wgrad_reduce_all_kernel, dim3(blocks), dim3(256), 0, st, df.red);
    }
    if (df.col.n) hipLaunchKernelGGL(colsum_all_kernel, dim3(2, df.col.n), dim3(256), 0, st, df.col);
}

inline void TrainPass::backward_time() {
    tb.split_tail = sw::time_tail_split() ? 1 : 0;
    hipLaunchKernelGGL(time_bwd_all_kernel, dim3(B + (tb.row + 31) / 32), dim3(1024), 0, st, tb);   // the time conditioning's backward
    if (tb.split_tail) hipLaunchKernelGGL(time_tail_kernel, dim3(kTimeTailBlocks), dim3(512), 0, st, tb);   // ... and its encoder tail, 8 blocks
}

}  // namespace mpdx

#include "train_bwd_prog.hpp"

using namespace mpdx;

// a self_attention=True network (attn.hpp) is inference and evaluation only: every training entry point that takes the handle refuses it
static int train_refuses_attention(const mpdx_unet* u) {
    if (u && u->cfg.self_attention)
        return fail(MPDX_E_INVALID, "self-attention network: the training pass has no backward for the self-attention blocks (self_attention=True runs inference and evaluation only)");
    return 0;
}

extern "C" {

size_t mpdx_train_flat_floats(mpdx_unet* u) {
    if (!u || train_refuses_attention(u)) return 0;
    build_train_plan(u);
    return u->flat_floats;
}
size_t mpdx_train_dgrad_pack_floats(mpdx_unet* u) {
    if (!u || train_refuses_attention(u)) return 0;
    build_train_plan(u);
    return std::max<size_t>(u->packedT_floats, 4);
}
size_t mpdx_train_workspace_floats(mpdx_unet* u, int B) {
    if (!u || B <= 0 || train_refuses_attention(u)) return 0;
    build_train_plan(u);
    return train_ws(u, B).total;
}
int mpdx_train_param_offset(mpdx_unet* u, int idx, size_t* off, size_t* n) {
    if (!u || idx < 0 || idx >= (int)u->params.size() || !off || !n) return fail(MPDX_E_INVALID, "bad argument");
    if (int rc = train_refuses_attention(u)) return rc;
    build_train_plan(u);
    *off = u->params[idx].foff; *n = u->params[idx].n;
    return 0;
}

/* flat parameter vector (reference layout) -> forward pack (+ the dgrad pack when packedT is given): one launch */
int mpdx_train_pack(mpdx_unet* u, const float* flat, float* packed, float* packedT, void* stream) {
    if (!u || !flat || !packed) return fail(MPDX_E_INVALID, "null argument");
    if (int rc = train_refuses_attention(u)) return rc;
    build_train_plan(u);
    if (int rc = ensure_pack_descs(u)) return rc;
    hipLaunchKernelGGL(pack_train_kernel, dim3((unsigned)u->n_pack_chunks), dim3(256), 0, (hipStream_t)stream, (const PackDesc*)u->pack_descs_dev,
                       (const PackChunk*)u->pack_chunks_dev, flat, packed, packedT);
    HIP_TRY(hipGetLastError());
    for (auto& p : u->params) if (!p.done) { p.done = true; u->n_done++; }
    u->pack_version++;
    return 0;
}

/* Draw mode of the training pass (an iteration captured into a hipGraph, trainer.TrainStep.step): with a non-null `step_counter_dev` (a device int
 * that counts the optimiser steps taken: mpdx_adam_step(step < 0) advances it) the NEXT mpdx_train_loss_backward calls treat `t_dev` and `noise` as
 * OUTPUTS and draw them on the device (Philox4x32-10 keyed by `seed`, stream position step * B + sample); null disarms. */
int mpdx_train_draw(mpdx_unet* u, unsigned long long seed, const int* step_counter_dev) {
    if (!u) return fail(MPDX_E_INVALID, "null handle");
    if (int rc = train_refuses_attention(u)) return rc;
    std::lock_guard<std::mutex> lk(g_train_rng_mu);
    if (step_counter_dev) g_train_rng[u] = TrainRng{seed, step_counter_dev};
    else g_train_rng.erase(u);
    return 0;
}

/* One p_losses evaluation WITH its gradient (diffusion_model_base.py:331-352 + loss.backward()):
 *   x_noisy = q_sample(x_start, t, noise) with hard conditions; x_recon = unet(x_noisy, t) with hard conditions;
 *   loss = mean(|x_recon - target|^p [* weights]);  grads_flat = d loss * loss_scale / d parameters  (every entry written).
 * `flat` / `packed` / `packedT`: the parameters and their two packs (mpdx_train_pack).  loss_out: one device float. */
int mpdx_train_loss_backward(mpdx_unet* u, const float* flat, const float* packed, const float* packedT, float* grads_flat, const float* x_start,
                             const float* noise, const long long* t_dev, const float* sqrt_alphas_cumprod_dev,
                             const float* sqrt_one_minus_alphas_cumprod_dev, const float* freqs16, const float* hard_start, const float* hard_goal,
                             const float* weights_hd, int T, int B, int predict_epsilon, int l1, float loss_scale, float* loss_out, float* ws,
                             void* stream) {
    if (!u || !flat || !packed || !packedT || !grads_flat || !x_start || !noise || !t_dev || !freqs16 || !loss_out || !ws || B <= 0)
        return fail(MPDX_E_INVALID, "bad argument");
    if (int rc = train_refuses_attention(u)) return rc;
    build_train_plan(u);
    if (int rc = check_ready(u)) return rc;
    if (!sqrt_alphas_cumprod_dev || !sqrt_one_minus_alphas_cumprod_dev) return fail(MPDX_E_INVALID, "schedule tables missing");
    TrainPass p(u, flat, packed, packedT, grads_flat, ws, B, (hipStream_t)stream);
    if (int rc = p.forward_time_qsample(x_start, noise, t_dev, sqrt_alphas_cumprod_dev, sqrt_one_minus_alphas_cumprod_dev, freqs16, hard_start, hard_goal, T)) return rc;
    if (int rc = p.forward_layers()) return rc;
    if (int rc = p.loss_and_seed_gradient(predict_epsilon ? noise : x_start, weights_hd, hard_start, hard_goal, l1, loss_scale, loss_out)) return rc;
    HIP_TRY(hipGetLastError());
    p.begin_backward();
    if (int rc = p.backward_final_conv1()) return rc;
    if (int rc = p.backward_walk()) return rc;
    p.report();
    if (int rc = p.late_wgrads()) return rc;
    p.finish_reductions();
    p.backward_time();
    HIP_TRY(hipGetLastError());
    return 0;
}

/* clip_grad_norm_ (max_norm > 0) + Adam step on flat vectors; scratch: >= 1032 floats; step: 1-based step count, or < 0: the count lives on the device
 * (int at scratch + 4, the number of steps taken so far; this call advances it) - the form a step replayed as a hipGraph needs, its kernel arguments being frozen */
int mpdx_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2, float eps,
                   int step, float max_norm, float* scratch, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !scratch || n == 0 || step == 0) return fail(MPDX_E_INVALID, "bad argument");
    if (lr < 0.f && step > 0) return fail(MPDX_E_INVALID, "lr < 0 (the learning rate from scratch[5]) needs the device-resident step count (step < 0)");
    hipStream_t st = (hipStream_t)stream;
    const float* clip = nullptr;
    int n_part = 0;
    int* cnt = step < 0 ? (int*)(scratch + 4) : nullptr;
    if (max_norm > 0.f || cnt) {   // (device-counter mode: the launch also advances the counter, clipping or not)
        const int nb = (int)std::min<size_t>((n + 255) / 256, 1024);
        hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, st, grads, n, scratch + 8, cnt);
        if (max_norm > 0.f) {
            clip = scratch + 8;   // the partial sums; adam_kernel finishes the norm itself (every block, the same fixed order: the same bits) and publishes scratch[0..1]
            n_part = nb;
        }
    }
    // the bias corrections 1 - beta^t and sqrt(1 - beta2^t) in double, rounded ONCE (torch.optim.Adam computes them in Python doubles): 1.0f - (float)pow(..)
    // rounds beta^t at 2^-25 absolute first, which is 1.5e-5 of 1 - 0.999^2 - the whole update of step 2 was off by 50 fp32 roundings
    const float bc1 = step > 0 ? (float)(1.0 - pow((double)beta1, step)) : 1.0f, bc2_sqrt = step > 0 ? (float)sqrt(1.0 - pow((double)beta2, step)) : 1.0f;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, lr,
                       beta1, beta2, eps, bc1, bc2_sqrt, clip, n_part, max_norm, scratch, (const int*)cnt);
    HIP_TRY(hipGetLastError());
    return 0;
}

int mpdx_ema_update(float* ema, const float* params, size_t n, float beta, void* stream) {
    if (!ema || !params || n == 0) return fail(MPDX_E_INVALID, "bad argument");
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream, ema, params, n, beta);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
