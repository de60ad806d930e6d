// train_bwd_prog.hpp - the whole-trajectory backward programs of the training pass (kernels: fused_bwd.hpp): the networks they are written for, and the
// two stages of TrainPass (train_host.hpp, which includes this file behind that struct) that enqueue them.
#pragma once

namespace mpdx {

// ---- whole-trajectory backward programs (fused_bwd.hpp).  The DOWN program: the backward pass of downs[0..2] of the standard network (three levels of
// [blocks.0 | residual 1x1 | blocks.1] [blocks.0 | blocks.1 (identity residual)] [Downsample1d], 32 / 64 / 128 channels on 64 / 32 / 16 positions) in
// ONE launch.  Layer indices: level k occupies [6 k, 6 k + 6) = b0.0, r, b0.1, b1.0, b1.1, down.
struct BwdProgLayout { int off4[5]; int stat_off; size_t lds_bytes; };
static BwdProgLayout bwd_down_layout() {
    // five LDS slots of the largest buffer (20 rows x (128 + 4) floats = 660 float4): IN (the stride-2 layer's zero-stuffed dU), GB, DUa, DUb, GA
    BwdProgLayout L;
    const int slot4 = kBwdSlot4;   // >= 20 x 33, 36 x 17, 68 x 9 float4
    for (int k = 0; k < 5; ++k) L.off4[k] = k * slot4;
    L.stat_off = 5 * slot4 * 4;
    L.lds_bytes = (size_t)(L.stat_off + 384) * sizeof(float);
    return L;
}
// is the head of the network the three-level down path the program is written for?  1: layers [0, 18), every level ends in a Downsample1d (dim_mults (1, 2, 4, 8));
// 2: layers [0, 17), the third level is the innermost one and has none (dim_mults (1, 2, 4): the reference's UNET_DIM_MULTS option 0); 0: neither
static int bwd_down_applicable(const mpdx_unet* u) {
    if ((int)u->layers.size() < 19 || u->cfg.n_support_points != 64 || u->masked()) return 0;
    int variant = 1;
    for (int k = 0; k < 3; ++k) {
        const int C = 32 << k, Lk = 64 >> k, b = 6 * k;
        const int cin = k == 0 ? u->cfg.state_dim : C / 2;
        auto blk = [&](int i, int c_in) { const Layer& l = u->layers[i]; return l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH && l.c1 == c_in && l.c2 == 0 && l.cout == C && l.L_out == Lk && l.gs * 8 == C; };
        if (!blk(b + 0, cin) || !blk(b + 2, C) || !blk(b + 3, C) || !blk(b + 4, C)) return 0;
        const Layer& r = u->layers[b + 1];
        if (!(r.mode == CONV_S1 && r.ks == 1 && r.epi == EPI_BIAS && r.c1 == cin && r.cout == C && r.L_out == Lk)) return 0;
        const Layer& d = u->layers[b + 5];
        const auto& tl = u->tl;
        const bool has_down = d.mode == CONV_DOWN && d.ks == 3 && d.epi == EPI_BIAS && d.c1 == C && d.cout == C && d.L_in == Lk && d.L_out == Lk / 2 && tl[b + 5].src1_l == b + 4;
        if (!has_down) {
            if (k < 2) return 0;
            variant = 2;   // (layer 17 is mid_block1's first convolution: the per-layer path has put its gradient into grd(16) by the time the program runs)
        }
        if (u->layers[b + 0].tb_off < 0 || u->layers[b + 3].tb_off < 0 || u->layers[b + 2].tb_off >= 0 || u->layers[b + 4].tb_off >= 0) return 0;
        if (tl[b + 2].res_l != b + 1 || tl[b + 4].res_l != b + 2 || tl[b + 2].src1_l != b || tl[b + 3].src1_l != b + 2 || tl[b + 4].src1_l != b + 3) return 0;
        if (k > 0 && (tl[b].src1_l != b - 1 || tl[b + 1].src1_l != b - 1)) return 0;
        for (int i = b + (k == 0 ? 2 : 0); i < b + (has_down ? 6 : 5); ++i) if (!tl[i].need_dgrad) return 0;
    }
    if (variant == 2 && (int)u->layers.size() == 34) {   // 3: ... and the two middle blocks (layers 17 .. 20: identity residuals, 128 channels on 16 positions) in front
        const auto& tl = u->tl;
        bool ok = true;
        for (int i = 17; i <= 20 && ok; ++i) {
            const Layer& l = u->layers[i];
            ok = l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH && l.c1 == 128 && l.c2 == 0 && l.cout == 128 && l.L_out == 16 && l.gs == 16 && tl[i].src1_l == i - 1 && tl[i].need_dgrad &&
                 ((i & 1) ? l.tb_off >= 0 : l.tb_off < 0);
        }
        if (ok && tl[18].res_l == 16 && tl[20].res_l == 18 && tl[17].res_l < 0 && tl[19].res_l < 0) variant = 3;
    }
    return variant;
}

// is the tail of the network [Upsample1d(128) | up level of 64 channels on 16 positions | up level of 32 on 32 | final_conv[0]] the UP program is written for?
// The four-level network: layers [33, 46) (ups[1], ups[2]); the three-level one: [21, 34) (ups[0], ups[1]).  Returns the first layer of the program, or -1.
static int bwd_up_applicable(const mpdx_unet* u) {
    const int n = (int)u->layers.size();
    if (n < 34 || u->cfg.n_support_points != 64 || u->masked()) return -1;
    const auto& tl = u->tl;
    const int fi = n - 1;   // final_conv[0] (final_conv[1], the 1x1, lives in the loss kernel and in final_conv[0]'s epilogue: it is no layer of the list)
    const Layer& f = u->layers[fi];
    if (!(f.mode == CONV_S1 && f.ks == 5 && f.epi == EPI_GN_MISH && f.c1 == 32 && f.c2 == 0 && f.cout == 32 && f.L_out == 64 && f.gs == 4 && f.tb_off < 0 && tl[fi].src1_l == fi - 1 && tl[fi].res_l < 0))
        return -1;
    const int bases[2] = {fi - 6, fi - 12}, Cs[2] = {32, 64}, Ls[2] = {32, 16}, skips[2] = {10, 16};
    for (int k = 0; k < 2; ++k) {
        const int b = bases[k], C = Cs[k], Lk = Ls[k];
        auto blk = [&](int i, int c1, int c2) { const Layer& l = u->layers[i]; return l.mode == CONV_S1 && l.ks == 5 && l.epi == EPI_GN_MISH && l.c1 == c1 && l.c2 == c2 && l.cout == C && l.L_out == Lk && l.gs * 8 == C; };
        if (!blk(b, 2 * C, 2 * C) || !blk(b + 2, C, 0) || !blk(b + 3, C, 0) || !blk(b + 4, C, 0)) return -1;
        const Layer& r = u->layers[b + 1];
        if (!(r.mode == CONV_S1 && r.ks == 1 && r.epi == EPI_BIAS && r.c1 == 2 * C && r.c2 == 2 * C && r.cout == C && r.L_out == Lk)) return -1;
        const Layer& up = u->layers[b + 5];
        if (!(up.mode == CONV_UPT && up.ks == 4 && up.epi == EPI_BIAS && up.c1 == C && up.cout == C && up.L_in == Lk && up.L_out == 2 * Lk)) return -1;
        if (u->layers[b].tb_off < 0 || u->layers[b + 3].tb_off < 0 || u->layers[b + 2].tb_off >= 0 || u->layers[b + 4].tb_off >= 0) return -1;
        if (tl[b].src1_l != b - 1 || tl[b + 1].src1_l != b - 1 || tl[b].src2_l != skips[k] || tl[b + 1].src2_l != skips[k]) return -1;
        if (tl[b + 2].res_l != b + 1 || tl[b + 4].res_l != b + 2 || tl[b + 2].src1_l != b || tl[b + 3].src1_l != b + 2 || tl[b + 4].src1_l != b + 3 || tl[b + 5].src1_l != b + 4) return -1;
        for (int i = b; i < b + 6; ++i) if (!tl[i].need_dgrad) return -1;
    }
    const int first = fi - 12;
    // the producer of the inner level's x half: 128 channels on 16 positions (the Upsample1d of the level below, or - three levels - mid_block2's blocks.1)
    const Layer& x = u->layers[first - 1];
    if (!(x.cout == 128 && x.L_out == 16 && u->layers[16].cout == 128 && u->layers[10].cout == 64 && tl[fi].need_dgrad)) return -1;
    return first;
}

// the next op of a program: its shape, every optional operand absent
static BwdOp& add_bwd_op(BwdArgs& a, int mode, int ks, int nc16, int ncr, int cout, int L, int gn) {
    BwdOp& op = a.ops[a.nops++];
    memset(&op, 0, sizeof(op));
    op.shape = bwd_shape_id(mode, ks, nc16, ncr, cout, L, gn);
    op.add_off4 = -1; op.gadd = -1; op.gy_off4 = -1; op.gy_g = -1; op.dst_off4 = -1; op.out_g = -1; op.part_g = -1; op.dT_g = -1;
    return op;
}
static int bwd_rs4_of(int C) { return C / 4 + kBwdPad4; }   // float4 per LDS row of a C-channel buffer

inline BwdArgs TrainPass::prog_args(const BwdProgLayout& lay) const {
    BwdArgs a;
    memset(&a, 0, sizeof(a));
    a.packedT = packedT; a.flat = flat; a.ws = ws; a.B = B; a.dT_stride = u->tt_row; a.stat_off = lay.stat_off;
    a.dbg = sw::bwd_dbg();
    return a;
}
// the lower Conv1dBlock `li` of an op: its GroupNorm input, parameters and the partial-sum rows of its gamma / beta / bias gradients
inline void TrainPass::prog_gn_part(int li, BwdOp& op) {
    const Layer& lj = u->layers[li];
    op.pre_g = goff(pre(li));
    op.gamma_f = (int)u->params[lj.gamma].foff; op.beta_f = (int)u->params[lj.beta].foff;
    op.part_g = (int)colsum3(lj);
    op.dT_g = lj.tb_off >= 0 ? (int)(w.dT + lj.tb_off) : -1;
}

// round 6: the backward pass of downs[0..2] as ONE whole-trajectory program (MPDX_TRAIN_BWD_PROG=0 switches it off): layers [0, dn_last] = [0, 18), on the
// three-level network [0, 17) or, with the middle blocks, [0, 21).  Returns 0 ok, < 0 error, 1 not applicable here (the per-layer path takes over)
inline int TrainPass::run_down_program() {
    const int n_gn = down_variant == 3 ? 16 : 12;   // GroupNorm ops (three column-sum entries each); dn_last + 1 weight-gradient jobs
    if (!written[dn_last] || df.red.n + dn_last + 1 > 96 || df.col.n + n_gn * 3 + 6 > 120) return 1;
    if (down_variant == 3 && !written[16]) return 1;   // (the skip connection's gradient, an addend of op M5)
    const int sdiv = wgrad_prog_sdiv(B);
    const BwdProgLayout lay = bwd_down_layout();
    BwdArgs a = prog_args(lay);
    enum { IN = 0, GB = 1, DUA = 2, DUB = 3, GA = 4 };
    a.gin = grd(17); a.in_L = 8; a.in_C = 128; a.in_stuff = 1; a.in_off4 = lay.off4[IN]; a.in_rs4 = bwd_rs4_of(128);
    if (down_variant >= 2) { a.gin = nullptr; a.in_L = 0; a.in_stuff = 0; }   // (no staged input: the first op takes grd(16) / grd(20) as its global addend)
    if (down_variant == 3) {   // M1 .. M4: the two middle blocks (fused_bwd.hpp bwd_down_mid_geom); M5 = the level loop's first op below
        const int r4 = bwd_rs4_of(128);
        {   // M1: G(layer 20 out) from the up program -> GB (the identity residual of mid_block2 passes it on to layer 18's output); GroupNorm backward of layer 20
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, 0, 0, 128, 16, 1);
            op.gadd = goff(grd(20));
            op.gy_off4 = lay.off4[GB]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(20));
            prog_gn_part(20, op);
        }
        {   // M2: dgrad of layer 20 -> G(19 out) (time bias), GroupNorm backward of 19
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, 8, 0, 128, 16, 1);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4; op.wbase = (int)u->tl[20].dgrad_woff;
            op.dst_off4 = lay.off4[DUB]; op.dst_rs4 = r4; op.out_g = goff(grd(19));
            prog_gn_part(19, op);
        }
        {   // M3: dgrad of 19 + GB -> G(18 out) -> GA; GroupNorm backward of 18
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, 8, 0, 128, 16, 1);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4; op.wbase = (int)u->tl[19].dgrad_woff;
            op.add_off4 = lay.off4[GB]; op.add_rs4 = r4;
            op.gy_off4 = lay.off4[GA]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(18));
            prog_gn_part(18, op);
        }
        {   // M4: dgrad of 18 -> G(17 out) (time bias), GroupNorm backward of 17
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, 8, 0, 128, 16, 1);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4; op.wbase = (int)u->tl[18].dgrad_woff;
            op.dst_off4 = lay.off4[DUB]; op.dst_rs4 = r4; op.out_g = goff(grd(17));
            prog_gn_part(17, op);
        }
    }
    for (int k = 2; k >= 0; --k) {
        const int C = 32 << k, Lk = 64 >> k, b0 = 6 * k, r4 = bwd_rs4_of(C);
        if (k == 2 && down_variant == 3) {   // M5: dgrad of layer 17 + GA (mid_block1's identity residual) + the skip connection's gradient -> G(16 out) -> GB; GroupNorm backward of 16
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4; op.wbase = (int)u->tl[17].dgrad_woff;
            op.add_off4 = lay.off4[GA]; op.add_rs4 = r4;
            op.gadd = goff(grd(b0 + 4));
            op.gy_off4 = lay.off4[GB]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 4));
            prog_gn_part(b0 + 4, op);
        } else if (k == 2 && down_variant == 2) {   // P1 of an innermost level (no Downsample1d): G(b1.1 out) is what the per-layer path accumulated in grd(16)
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, 0, 0, C, Lk, 1);
            op.gadd = goff(grd(b0 + 4));
            op.gy_off4 = lay.off4[GB]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 4));
            prog_gn_part(b0 + 4, op);
        } else {   // P1: dgrad of the Downsample1d (its dU zero-stuffed in IN) + the skip connection's gradient -> G(b1.1 out) -> GB; GroupNorm backward of b1.1
            BwdOp& op = add_bwd_op(a, CONV_S1, 3, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[IN]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 5].dgrad_woff;
            if (written[b0 + 4]) op.gadd = goff(grd(b0 + 4));
            op.gy_off4 = lay.off4[GB]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 4));
            prog_gn_part(b0 + 4, op);
        }
        {   // P2: dgrad of b1.1 -> G(b1.0 out) (its time-bias gradient), GroupNorm backward of b1.0
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 4].dgrad_woff;
            op.dst_off4 = lay.off4[DUB]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 3));
            prog_gn_part(b0 + 3, op);
        }
        {   // P3: dgrad of b1.0 + the identity residual's G (GB) -> G(b0.1 out) -> GA + the residual 1x1's dY (global); GroupNorm backward of b0.1
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 3].dgrad_woff;
            op.add_off4 = lay.off4[GB]; op.add_rs4 = r4;
            op.gy_off4 = lay.off4[GA]; op.gy_rs4 = r4; op.gy_g = goff(grd(b0 + 1));
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 2));
            prog_gn_part(b0 + 2, op);
        }
        {   // P4: dgrad of b0.1 -> G(b0.0 out) (time bias), GroupNorm backward of b0.0
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 2].dgrad_woff;
            op.dst_off4 = k > 0 ? lay.off4[DUB] : -1; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 0));
            prog_gn_part(b0 + 0, op);
        }
        if (k > 0) {   // P5: dgrad of b0.0 + the residual 1x1's (from GA) -> dU of the level above's Downsample1d, zero-stuffed into IN
            const int Cp = C / 2;
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, C / 16, Cp, Lk, 0);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4;
            op.rsrc_off4 = lay.off4[GA]; op.rsrc_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 0].dgrad_woff; op.rwbase = (int)u->tl[b0 + 1].dgrad_woff;
            op.dst_off4 = lay.off4[IN]; op.dst_rs4 = bwd_rs4_of(Cp); op.dst_mode = 1; op.out_g = goff(grd(b0 - 1));
        }
    }
    for (int k = 0; k < a.nops; ++k)
        if (a.ops[k].shape < 0) return fail(MPDX_E_INVALID, "backward program: op %d has no shape", k);
    const bool last = down_variant == 2, mid = down_variant == 3;
    bool is_static = a.nops == (mid ? BwdSeqDown3Mid::N : BwdSeqDown3::N);
    for (int k = 0; k < a.nops && is_static; ++k)
        is_static = a.ops[k].shape == (mid ? BwdSeqDown3Mid::ids[k] : (last ? BwdSeqDown3Last::ids[k] : BwdSeqDown3::ids[k])) &&
                    bwd_geom_matches(a.ops[k], mid ? bwd_down_mid_geom(k) : bwd_down_geom(k, last), a.ops[k].shape == 2 || a.ops[k].shape == 5);
    if (!is_static) return fail(MPDX_E_STATE, "backward program (down): the layout differs from the static program's table");
    const void* kern = mid ? (const void*)fused_bwd_program_kernel<BwdSeqDown3Mid> : (last ? (const void*)fused_bwd_program_kernel<BwdSeqDown3Last> : (const void*)fused_bwd_program_kernel<BwdSeqDown3>);
    if (int rc = raise_lds_limit(kern)) return rc;
    if (mid) hipLaunchKernelGGL(fused_bwd_program_kernel<BwdSeqDown3Mid>, dim3(B), dim3(kFusedThreads), lay.lds_bytes, st, a);
    else if (last) hipLaunchKernelGGL(fused_bwd_program_kernel<BwdSeqDown3Last>, dim3(B), dim3(kFusedThreads), lay.lds_bytes, st, a);
    else hipLaunchKernelGGL(fused_bwd_program_kernel<BwdSeqDown3>, dim3(B), dim3(kFusedThreads), lay.lds_bytes, st, a);
    // the layers' weight gradients (their dY operands now sit in grd(i)) behind the chain; bias gradients of the three convolutions without GroupNorm
    for (int i = dn_last; i >= 0; --i) {
        const Layer& l = u->layers[i];
        const auto& t = u->tl[i];
        written[i] = 1; du_ready[i] = 1;
        const int sb = l.mode == CONV_DOWN ? 2 : 1, ob = l.mode == CONV_DOWN ? -1 : -(l.ks / 2);
        WgradJob j;
        if (int rc = make_wgrad(grd(i), l.L_out, l.cout, 0, l.cout, tensor(t.src1_l), l.L_in, l.c1, 0, l.c1, sb, ob, l.ks, B, part(), gflat(l.w), l.c1, 0, &df, j, sdiv)) return rc;
        if (!j.deferred) return fail(MPDX_E_STATE, "backward program: no partial-sum storage left for layer %d", i);
        if (l.epi != EPI_GN_MISH && !attach_bias(j, &df, gflat(l.b), false)) return fail(MPDX_E_STATE, "backward program: no column-sum slot left for layer %d", i);
        lone.push_back(j);
    }
    return 0;
}

// final_conv[0] and the two outer up levels, layers [up_first, n) = [33, 46) ([21, 34) with three levels), as ONE program; 0 ok, < 0 error, 1 not applicable here
inline int TrainPass::run_up_program() {
    const int up_fi = n - 1;   // final_conv[0]
    if (!written[up_fi] || df.red.n + 17 > 96 || df.col.n + 9 * 3 + 4 > 120) return 1;
    const int sdiv = wgrad_prog_sdiv(B);
    const BwdProgLayout lay = bwd_down_layout();   // (the same five slots: the largest buffer here is 68 rows x 36 floats = 612 float4)
    BwdArgs a = prog_args(lay);
    enum { IN = 0, GB = 1, DUA = 2, DUB = 3, GA = 4 };
    a.gin = nullptr; a.in_L = 64; a.in_C = 32; a.in_stuff = 0; a.in_off4 = lay.off4[IN]; a.in_rs4 = bwd_rs4_of(32);   // (no staged input: U0 reads the loss kernel's gradient itself)
    {   // U0: final_conv[0]'s Mish + GroupNorm backward on the loss kernel's gradient (an op without a convolution: the gradient is its global addend);
        // dU -> IN and, in place, grd(45) (the operand of final_conv[0]'s weight gradient)
        BwdOp& op = add_bwd_op(a, CONV_S1, 5, 0, 0, 32, 64, 1);
        op.gadd = goff(grd(up_fi));
        op.dst_off4 = lay.off4[IN]; op.dst_rs4 = bwd_rs4_of(32); op.out_g = goff(grd(up_fi));
        prog_gn_part(up_fi, op);
    }
    {   // U1: dgrad of final_conv[0] -> dU of ups[2]'s Upsample1d (64 positions)
        BwdOp& op = add_bwd_op(a, CONV_S1, 5, 2, 0, 32, 64, 0);
        op.src_off4 = lay.off4[IN]; op.src_rs4 = bwd_rs4_of(32);
        op.wbase = (int)u->tl[up_fi].dgrad_woff;
        op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = bwd_rs4_of(32); op.out_g = goff(grd(up_fi - 1));
    }
    const int bases[2] = {up_fi - 6, up_fi - 12}, Cs[2] = {32, 64}, Ls[2] = {32, 16}, skips[2] = {10, 16};
    int src_slot = DUA;   // where the level's Upsample1d dU sits (2 L positions)
    for (int k = 0; k < 2; ++k) {
        const int b0 = bases[k], C = Cs[k], Lk = Ls[k], r4 = bwd_rs4_of(C);
        {   // dgrad of the Upsample1d (its 5-tap pack at stride 2) -> G(b1.1 out) -> GB; GroupNorm backward of b1.1
            BwdOp& op = add_bwd_op(a, CONV_DOWN, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[src_slot]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 5].dgrad_woff;
            op.gy_off4 = lay.off4[GB]; op.gy_rs4 = r4;
            op.dst_off4 = lay.off4[DUB]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 4));
            prog_gn_part(b0 + 4, op);
        }
        {   // dgrad of b1.1 -> G(b1.0 out) (time bias), GroupNorm backward of b1.0
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 4].dgrad_woff;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 3));
            prog_gn_part(b0 + 3, op);
        }
        {   // dgrad of b1.0 + the identity residual's G -> G(b0.1 out) -> GA + the residual 1x1's dY; GroupNorm backward of b0.1
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 3].dgrad_woff;
            op.add_off4 = lay.off4[GB]; op.add_rs4 = r4;
            op.gy_off4 = lay.off4[GA]; op.gy_rs4 = r4; op.gy_g = goff(grd(b0 + 1));
            op.dst_off4 = lay.off4[DUB]; op.dst_rs4 = r4; op.out_g = goff(grd(b0 + 2));
            prog_gn_part(b0 + 2, op);
        }
        {   // dgrad of b0.1 -> G(b0.0 out) (time bias), GroupNorm backward of b0.0
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, 0, C, Lk, 1);
            op.src_off4 = lay.off4[DUB]; op.src_rs4 = r4;
            op.wbase = (int)u->tl[b0 + 2].dgrad_woff;
            op.dst_off4 = lay.off4[DUA]; op.dst_rs4 = r4; op.out_g = goff(grd(b0));
            prog_gn_part(b0, op);
        }
        // dgrad of b0.0 + the residual 1x1's (from GA): the gradient of the channel concat [x | skip], one op per half (2 C channels each)
        const int nblk = (C / 16) * 5, ncr = C / 16, rows_half = 2 * C / 16;
        for (int half = 0; half < 2; ++half) {
            BwdOp& op = add_bwd_op(a, CONV_S1, 5, C / 16, C / 16, 2 * C, Lk, 0);
            op.src_off4 = lay.off4[DUA]; op.src_rs4 = r4;
            op.rsrc_off4 = lay.off4[GA]; op.rsrc_rs4 = r4;
            op.wbase = (int)u->tl[b0].dgrad_woff + half * rows_half * nblk * 256;
            op.rwbase = (int)u->tl[b0 + 1].dgrad_woff + half * rows_half * ncr * 256;
            if (half == 0) {   // x: the level below's Upsample1d output (its dU); the next level of this program reads it from LDS
                op.out_g = goff(grd(b0 - 1));
                if (k == 0) { op.dst_off4 = lay.off4[IN]; op.dst_rs4 = bwd_rs4_of(2 * C); }
            } else op.out_g = goff(grd(skips[k]));   // the skip connection's gradient (first writer: stored)
        }
        src_slot = IN;
    }
    for (int k = 0; k < a.nops; ++k)
        if (a.ops[k].shape < 0) return fail(MPDX_E_INVALID, "backward program (up): op %d has no shape", k);
    bool is_static = a.nops == BwdSeqUp2::N;
    for (int k = 0; k < a.nops && is_static; ++k) is_static = a.ops[k].shape == BwdSeqUp2::ids[k] && bwd_geom_matches(a.ops[k], bwd_up_geom(k), a.ops[k].shape == 11 || a.ops[k].shape == 14);
    if (!is_static) return fail(MPDX_E_STATE, "backward program (up): the layout differs from the static program's table");
    if (int rc = raise_lds_limit((const void*)fused_bwd_program_kernel<BwdSeqUp2>)) return rc;
    hipLaunchKernelGGL(fused_bwd_program_kernel<BwdSeqUp2>, dim3(B), dim3(kFusedThreads), lay.lds_bytes, st, a);
    written[up_first - 1] = written[16] = written[10] = 1;
    for (int i = up_fi; i >= up_first; --i) {
        const Layer& l = u->layers[i];
        written[i] = 1; du_ready[i] = 1;
        WgradJob jb[2];
        int nj = 0;
        if (int rc = layer_wgrads(i, grd(i), sdiv, jb, nj)) return rc;
        for (int k = 0; k < nj; ++k) if (!jb[k].deferred) return fail(MPDX_E_STATE, "backward program: no partial-sum storage left for layer %d", i);
        if (l.epi != EPI_GN_MISH && !attach_bias(jb[0], &df, gflat(l.b), l.mode == CONV_UPT)) return fail(MPDX_E_STATE, "backward program: no column-sum slot left for layer %d", i);
        for (int k = 0; k < nj; ++k) lone.push_back(jb[k]);
    }
    return 0;
}

}  // namespace mpdx
