// fused_build.hpp - host side of the whole-trajectory programs (fused_level.hpp): a range of the layer plan as one mpdx_unet::Fused (SegmentBuilder)
// and which ranges of a network become programs (build_units).  Included by mpdx.hip alone, behind build_model; no device code.
#pragma once
#include "host.hpp"

namespace mpdx {

// MPDX_DEBUG_FUSE: 0 not set, 1 set (the segments built and the shape constraint that rejected one), 2 a value >= 2 (their LDS geometry too)
static int debug_fuse_level() {
    const char* e = sw::debug_fuse();
    return !e ? 0 : (atoi(e) >= 2 ? 2 : 1);
}
static bool fuse_reject(int line) {
    if (debug_fuse_level()) fprintf(stderr, "[mpdx] fused segment rejected at fused_build.hpp:%d\n", line);
    return false;
}

struct HostBuf { int off4 = -1, rs4 = 0, rows = 0; size_t size4 = 0; int def = 1 << 30, last = -1; };

// Layers [i0, i1) (an outer U-Net level: 2 residual blocks + resample [+ final_conv[0]]) as one fused_level_kernel program.  The stages run in
// the order of build(); each returns false (after fuse_reject) when a shape constraint fails, and nothing of the handle is touched before the
// last one has passed.
struct __attribute__((visibility("hidden"))) SegmentBuilder {   // (its members are no symbols of the shared library)
    struct HostOp { int src = -1, rsrc = -1, res = -1, dst = -1; const Layer* l = nullptr; const Layer* r = nullptr; int nblk = 0, ncr = 0, tot = 0, nstream = 0; };

    mpdx_unet* const u;
    const int i0, i1;
    const bool with_final;
    const Layer& l0;
    mpdx_unet::Fused f;
    FusedArgs& a;                          // f.tmpl
    // LDS activation buffers are placed AFTER the op list is known, by live range [first write, last read] in op indices (-1 = staged by the
    // prologue): buffers whose ranges do not intersect share addresses
    std::vector<HostBuf> bufs;
    std::unordered_map<long, int> bufmap;  // (slot, L) -> LDS buffer
    std::vector<HostOp> hops;
    int in_buf = -1, final_src = -1;
    int cat_buf = -1;                      // buffer whose tail columns hold a skip tensor staged by the prologue (concat inside the program)
    bool in_slot_rewritten = false;        // a layer of the segment has written the workspace slot the segment's input came in
    int ng = 0, poff = 0;                  // global outputs assigned so far; floats of the parameter block
    size_t off4 = 0, area = 0;             // LDS float4s laid out so far; end of the segment's streams + parameter block in `packed`

    SegmentBuilder(mpdx_unet* u_, int i0_, int i1_, bool with_final_)
        : u(u_), i0(i0_), i1(i1_), with_final(with_final_), l0(u_->layers[i0_]), a(f.tmpl) {
        f.first = i0; f.count = i1 - i0; f.has_final = with_final;
        memset(&a, 0, sizeof(a));
        f.in1 = l0.src1; f.in2 = l0.src2;
        a.gc1 = l0.c1; a.gc2 = l0.c2; a.L0 = l0.L_in;
    }

    static long key(int slot, int L) { return (long)(slot + 8) * 4096 + L; }
    int new_buf(int cpad, int L) {
        HostBuf hb;
        const int rs = pick_row_stride(cpad, CONV_S1, L, L, L + 4);
        hb.rs4 = rs / 4; hb.rows = L + 4; hb.size4 = (size_t)(L + 4) * (rs / 4);
        bufs.push_back(hb);
        return (int)bufs.size() - 1;
    }
    void touch(int id, int opi, bool write) {
        if (id < 0) return;
        if (write) bufs[id].def = std::min(bufs[id].def, opi);
        bufs[id].last = std::max(bufs[id].last, opi);
    }
    // the LDS buffer a layer writes its output (workspace slot `slot`, L positions) to.  A slot written again with the same shape re-uses its buffer (the
    // blocks' HB / RB temporaries, an up level's second block writing the slot the level's input came in) - except a buffer too narrow for it (three-level
    // network, round 6: mid_block1's 128 channels go to the slot downs.1's Downsample1d output - the segment input, 64 channels - came in): a buffer of its own
    int buf_for(int slot, int L, int cpad) {
        auto it = bufmap.find(key(slot, L));
        if (it != bufmap.end()) {
            const int rs = pick_row_stride(cpad, CONV_S1, L, L, L + 4);
            if (it->second == in_buf) in_slot_rewritten = true;   // (src_buf: from here on that slot is a tensor of the segment, no longer its input)
            if (bufs[it->second].rs4 >= rs / 4) return it->second;
        }
        const int id = new_buf(cpad, L);
        bufmap[key(slot, L)] = id;
        return id;
    }
    int src_buf(const Layer& l, int i) {   // LDS buffer a layer reads (-1: not available inside the segment)
        if (i == i0 || (!in_slot_rewritten && l.src1 == l0.src1 && l.src2 == l0.src2 && l.L_in == l0.L_in)) return in_buf;
        const long k = key(l.src1, l.L_in);
        if (!bufmap.count(k)) return -1;
        if (l.src2 != SRC_NONE) {   // cat(x produced in LDS, skip from global): the producer's buffer was made wide enough (pick_destination)
            if (bufmap[k] != cat_buf || f.in3 != l.src2) return -1;
        }
        return bufmap[k];
    }
    // a layer of the segment (not the first) that concatenates a global skip tensor behind a tensor produced inside
    const Layer* cat_consumer(int from, int slot, int L) const {
        for (int k = from; k < i1; ++k) {
            const Layer& n = u->layers[k];
            if (n.src1 == slot && n.L_in == L && n.src2 != SRC_NONE && !(n.src1 == l0.src1 && n.src2 == l0.src2)) return &n;
            if (n.dst == slot) break;   // overwritten: later readers see another tensor
        }
        return nullptr;
    }

    // ---- stage 1: the op list.  Folds a block's residual 1x1 conv into blocks[1], picks source and destination buffers, records live ranges
    bool collect_ops() {
        in_buf = new_buf(l0.cin_pad, l0.L_in);
        a.in_clear = (l0.cin_pad != l0.c1 + l0.c2) ? 1 : 0;  // channel padding of the staged input
        touch(in_buf, -1, true);
        bufmap[key(l0.src1, l0.L_in)] = in_buf;
        int pending_res = -1;   // index of a residual 1x1 conv waiting to be folded into the block's blocks[1]
        for (int i = i0; i < i1; ++i) {
            const Layer& l = u->layers[i];
            // a block's residual 1x1 conv is folded into blocks[1] (the next layer, which adds its output after Mish)
            if (l.mode == CONV_S1 && l.ks == 1 && l.epi == EPI_BIAS && i + 1 < i1 && u->layers[i + 1].res == l.dst &&
                u->layers[i + 1].epi == EPI_GN_MISH && u->layers[i + 1].L_out == l.L_out && u->layers[i + 1].cout == l.cout) {
                pending_res = i;
                continue;
            }
            if (!add_op(i, pending_res)) return false;
            pending_res = -1;
        }
        if (pending_res >= 0) return fuse_reject(__LINE__);
        if (with_final) {
            const Layer& lf = u->layers[i1 - 1];
            FusedOp& op = a.ops[a.nops++];
            memset(&op, 0, sizeof(op));
            op.shape = kFusedShapeFinal;
            final_src = bufmap[key(lf.dst, lf.L_out)];
            touch(final_src, a.nops - 1, false);
            a.H = lf.L_out;
            a.Cf = u->cfg.unet_input_dim; a.D = u->cfg.state_dim;
            a.fw_off = (int)u->params[u->pidx.at("final_conv.1.weight")].off;
            a.fb_off = (int)u->params[u->pidx.at("final_conv.1.bias")].off;
        }
        return true;
    }
    // layer i as op a.nops (pending_res >= 0: with that residual 1x1 conv folded in)
    bool add_op(int i, int pending_res) {
        const Layer& l = u->layers[i];
        if (a.nops >= kMaxFusedOps - (with_final ? 1 : 0)) return fuse_reject(__LINE__);
        FusedOp& op = a.ops[a.nops];
        memset(&op, 0, sizeof(op));
        HostOp ho;
        ho.l = &l;
        const int gn = l.epi == EPI_GN_MISH ? 1 : 0;
        if (gn && (l.gs * 8 != l.cout || l.mode != CONV_S1)) return fuse_reject(__LINE__);   // the shapes assume GroupNorm(8 groups)
        ho.src = src_buf(l, i);
        if (ho.src < 0) return fuse_reject(__LINE__);
        if (pending_res >= 0) {
            ho.r = &u->layers[pending_res];
            ho.rsrc = src_buf(*ho.r, pending_res);
            if (ho.rsrc < 0) return fuse_reject(__LINE__);
        } else if (l.res != SRC_NONE) {
            if (!bufmap.count(key(l.res, l.L_out))) return fuse_reject(__LINE__);
            ho.res = bufmap[key(l.res, l.L_out)];
        }
        const int nc16 = l.cin_pad / 16, rnc16 = ho.r ? ho.r->cin_pad / 16 : 0;
        op.shape = fused_shape_id(l.mode, l.ks, nc16, rnc16, l.cout, l.L_out, gn);
        if (op.shape < 0) return fuse_reject(__LINE__);
        ho.nblk = nc16 * (l.mode == CONV_UPT ? 2 : l.ks); ho.ncr = rnc16; ho.tot = ho.nblk + ho.ncr;
        ho.nstream = (l.cout / 16) * (l.mode == CONV_UPT ? 2 : 1);
        const int msn = l.cout / 16, msw = std::min(msn, kFusedWaves), mp = msn / msw;   // tile rows, rows in flight, M-passes (FusedShape)
        a.msmask[a.nops] = msw - 1;
        a.slen[a.nops] = ho.tot * (l.mode == CONV_UPT ? 2 : mp);
        bool read_outside = false;
        if (!pick_destination(i, ho, read_outside)) return false;
        op.gdst = -1;
        if (read_outside) {
            if (ng >= 3) return fuse_reject(__LINE__);
            f.gout_slot[ng] = l.dst;
            op.gdst = ng++;
        }
        touch(ho.src, a.nops, false); touch(ho.res, a.nops, false); touch(ho.rsrc, a.nops, false); touch(ho.dst, a.nops, true);
        hops.push_back(ho);
        f.op_layer.push_back(i);
        a.nops++;
        return true;
    }
    // destination of layer i: LDS (ho.dst) if a later layer of the segment (or the final op) reads it; global if someone outside does.  An output
    // that heads a concat gets a buffer wide enough for the skip tensor behind it
    bool pick_destination(int i, HostOp& ho, bool& read_outside) {
        const Layer& l = *ho.l;
        bool read_inside = with_final && i == i1 - 1;
        for (int k = i + 1; k < i1; ++k) {
            const Layer& n = u->layers[k];
            if ((n.src1 == l.dst && n.L_in == l.L_out) || (n.res == l.dst && n.L_out == l.L_out)) read_inside = true;
            if (n.dst == l.dst) break;  // overwritten
        }
        bool overwritten_inside = false;  // the slot is re-used by a later layer of this segment: this value never leaves
        for (int k = i + 1; k < i1; ++k)
            if (u->layers[k].dst == l.dst) { overwritten_inside = true; break; }
        for (size_t k = i1; k < u->layers.size() && !overwritten_inside; ++k) {
            const Layer& n = u->layers[k];
            if (n.src1 == l.dst || n.src2 == l.dst || n.res == l.dst) { read_outside = true; break; }
            if (n.dst == l.dst) break;
        }
        if (i == i1 - 1 && !with_final) read_outside = true;
        ho.dst = -1;
        if (read_inside) {
            const Layer* cc = cat_consumer(i + 1, l.dst, l.L_out);
            if (cc) {   // this op's output is the head of a concat: make the buffer wide enough for the skip tensor behind it
                if (cat_buf >= 0 || cc->c1 != l.cout || (cc->c2 & 3) || (l.cout & 3) || (size_t)cc->L_in * (cc->c2 / 4) > 1024) {
                    if (debug_fuse_level()) fprintf(stderr, "[mpdx] cat: layer %s -> %s cat_buf %d c1 %d c2 %d cout %d L %d\n", l.name.c_str(), cc->name.c_str(), cat_buf, cc->c1, cc->c2, l.cout, cc->L_in);
                    return fuse_reject(__LINE__);
                }
                ho.dst = buf_for(l.dst, l.L_out, cc->c1 + cc->c2);
                cat_buf = ho.dst;
                f.in3 = cc->src2;
                f.in3_consumer = (int)(cc - &u->layers[0]);
                a.c3 = cc->c2; a.L3 = cc->L_in; a.s3_col4 = cc->c1 / 4;
                touch(cat_buf, -1, true);   // its skip columns are written by the prologue: live from the start
            } else ho.dst = buf_for(l.dst, l.L_out, l.cout);
        }
        if (ho.dst >= 0 && (ho.dst == ho.src || ho.dst == ho.res || ho.dst == ho.rsrc)) return fuse_reject(__LINE__);
        return true;
    }

    // ---- stage 2: first-fit placement in order of definition; two buffers may share addresses iff one is dead strictly before the op that first
    // writes the other.  The offsets go into the descriptors of the input, the concat and every op
    void place_buffers() {
        const int nbuf = (int)bufs.size();
        std::vector<int> order(nbuf);
        for (int i = 0; i < nbuf; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int x, int y) { return bufs[x].def < bufs[y].def; });
        for (int oi = 0; oi < nbuf; ++oi) {
            HostBuf& bi = bufs[order[oi]];
            if (bi.last < bi.def) bi.last = bi.def;
            size_t cand = 0;
            for (bool moved = true; moved;) {
                moved = false;
                for (int oj = 0; oj < oi; ++oj) {
                    const HostBuf& bj = bufs[order[oj]];
                    const bool live_overlap = !(bj.last < bi.def || bi.last < bj.def);
                    const size_t lo = (size_t)bj.off4, hi = lo + bj.size4;
                    if (live_overlap && cand < hi && lo < cand + bi.size4) { cand = hi; moved = true; }
                }
            }
            bi.off4 = (int)cand;
            off4 = std::max(off4, cand + bi.size4);
        }
        a.in_off4 = bufs[in_buf].off4; a.in_rs4 = bufs[in_buf].rs4; a.in_rows = bufs[in_buf].rows;
        if (cat_buf >= 0) { a.s3_off4 = bufs[cat_buf].off4; a.s3_rs4 = bufs[cat_buf].rs4; }
        for (size_t k = 0; k < hops.size(); ++k) {
            const HostOp& ho = hops[k];
            FusedOp& op = a.ops[k];
            op.src_off4 = bufs[ho.src].off4; op.src_rs4 = bufs[ho.src].rs4;
            op.rsrc_off4 = ho.rsrc >= 0 ? bufs[ho.rsrc].off4 : 0; op.rsrc_rs4 = ho.rsrc >= 0 ? bufs[ho.rsrc].rs4 : 0;
            op.res_off4 = ho.res >= 0 ? bufs[ho.res].off4 : -1; op.res_rs4 = ho.res >= 0 ? bufs[ho.res].rs4 : 0;
            op.dst_off4 = ho.dst >= 0 ? bufs[ho.dst].off4 : -1; op.dst_rs4 = ho.dst >= 0 ? bufs[ho.dst].rs4 : 0;
        }
        if (with_final) { a.ops[a.nops - 1].src_off4 = bufs[final_src].off4; a.ops[a.nops - 1].src_rs4 = bufs[final_src].rs4; }
    }

    // ---- stage 3: weight streams + parameter block of the segment: a dedicated area at the end of `packed`, and the CopyJobs that assemble it
    bool lay_out_streams_and_params() {
        area = u->packed_floats;
        int tt_lo = 1 << 30, tt_hi = 0;
        for (size_t k = 0; k < hops.size(); ++k) {
            const HostOp& ho = hops[k];
            const Layer& l = *ho.l;
            FusedOp& op = a.ops[k];
            op.sbase = (int)area;
            const int MSn = l.cout / 16, nc16 = l.cin_pad / 16;
            const size_t woff = u->params[l.w].off;
            if (l.mode == CONV_UPT) {   // streams (ms, parity): slots {2 par, 2 par + 1} of every 16-channel chunk
                for (int par = 0; par < 2; ++par)
                    f.jobs.push_back({woff + (size_t)par * 2 * 256, area + (size_t)par * ho.tot * 256, MSn, nc16 * 4 * 256, 2 * ho.tot * 256, nc16, 4 * 256, 2 * 256, 512});
            } else if (MSn > kFusedWaves) {   // M-passes: wave-stream s = [tile row s | tile row s + 4], each [conv blocks | folded residual blocks]
                const int mp = MSn / kFusedWaves;
                f.jobs.push_back({woff, area, mp, kFusedWaves * ho.nblk * 256, ho.tot * 256, kFusedWaves, ho.nblk * 256, mp * ho.tot * 256, ho.nblk * 256});
                if (ho.r)
                    f.jobs.push_back({u->params[ho.r->w].off, area + (size_t)ho.nblk * 256, mp, kFusedWaves * ho.ncr * 256, ho.tot * 256, kFusedWaves, ho.ncr * 256,
                                      mp * ho.tot * 256, ho.ncr * 256});
            } else {
                f.jobs.push_back({woff, area, MSn, ho.nblk * 256, ho.tot * 256, 1, 0, 0, ho.nblk * 256});
                if (ho.r) f.jobs.push_back({u->params[ho.r->w].off, area + (size_t)ho.nblk * 256, MSn, ho.ncr * 256, ho.tot * 256, 1, 0, 0, ho.ncr * 256});
            }
            area += (size_t)ho.nstream * ho.tot * 256;
            op.p_off = poff;
            poff += 4 * l.cout;
            op.tb_off = l.tb_off;   // made relative to the staged slice below
            if (l.tb_off >= 0) { tt_lo = std::min(tt_lo, l.tb_off); tt_hi = std::max(tt_hi, l.tb_off + l.cout); }
        }
        area += (size_t)kFusedRing * 256;   // the ring request of the last stream may read up to 16 blocks past its end
        if (with_final) {   // final_conv[1]: rows padded to Cf + 4 floats (bank spread), the bias behind them
            if (a.H * a.D > kFinalPre * kFusedThreads || (a.Cf & 3)) return fuse_reject(__LINE__);
            a.fpar_off = poff;
            poff += (a.D * (a.Cf + 4) + a.D + 3) / 4 * 4;
        }
        a.gpar_off = (int)area; a.par_floats = poff;
        for (size_t k = 0; k < hops.size(); ++k) {
            const HostOp& ho = hops[k];
            const Layer& l = *ho.l;
            const size_t pb = area + a.ops[k].p_off;
            f.jobs.push_back({u->params[l.b].off, pb, 1, 0, 0, 1, 0, 0, l.cout});
            if (l.gamma >= 0) f.jobs.push_back({u->params[l.gamma].off, pb + l.cout, 1, 0, 0, 1, 0, 0, l.cout});
            if (l.beta >= 0) f.jobs.push_back({u->params[l.beta].off, pb + 2 * (size_t)l.cout, 1, 0, 0, 1, 0, 0, l.cout});
            if (ho.r) f.jobs.push_back({u->params[ho.r->b].off, pb + 3 * (size_t)l.cout, 1, 0, 0, 1, 0, 0, l.cout});
        }
        if (with_final) {
            f.jobs.push_back({(size_t)a.fw_off, area + a.fpar_off, a.D, a.Cf, a.Cf + 4, 1, 0, 0, a.Cf});
            f.jobs.push_back({(size_t)a.fb_off, area + a.fpar_off + (size_t)a.D * (a.Cf + 4), 1, 0, 0, 1, 0, 0, a.D});
        }
        area += poff;
        if (tt_hi > 0) {
            a.tt_lo = tt_lo; a.tt_n = (tt_hi - tt_lo + 3) / 4 * 4;
            for (int k = 0; k < (int)hops.size(); ++k)
                if (a.ops[k].tb_off >= 0) a.ops[k].tb_off -= tt_lo;
        }
        return true;
    }
    // ---- stage 4: behind the activation buffers: GroupNorm exchange | time-table slice | parameter block.  The block whose size depends on the state
    // dimension (final_conv[1]'s weights) comes LAST, so that every other LDS offset of a program is the same for every state_dim
    // (fused_geom.hpp holds them as compile-time constants).  Then the limits of the prologue and of the LDS
    bool lay_out_tail() {
        a.stat_off = (int)off4 * 4;     // GroupNorm exchange: 8 tiles x 4 rows x (mean, M2)
        off4 += 16;
        a.tt_off = (int)off4 * 4;
        off4 += (size_t)a.tt_n / 4;
        a.par_off = (int)off4 * 4;
        off4 += (size_t)(poff + 3) / 4;
        if ((size_t)(poff / 4 + a.tt_n / 4) > 2048) return fuse_reject(__LINE__);   // prologue: 2048 float4 of parameters per workgroup
        const int c4n = (a.gc1 + a.gc2 + 3) / 4;
        int l4 = 0;
        while ((1 << l4) < c4n) ++l4;
        a.lg_c4n = ((1 << l4) == c4n) ? l4 : -1;
        if ((size_t)a.L0 * c4n > 2048) return fuse_reject(__LINE__);   // prologue holds the input window in registers (2048 float4)
        f.lds_bytes = off4 * 16;
        if (f.lds_bytes > 160 * 1024) return fuse_reject(__LINE__);
        return true;
    }

    // ---- stage 5: a known op sequence runs as a static program
    void match_program() {
        if (!sw::static_programs()) return;
        auto matches = [&](const int* ids, int n) {
            if (n != a.nops) return false;
            for (int k = 0; k < n; ++k) if (a.ops[k].shape != ids[k]) return false;
            return true;
        };
        if (matches(FusedSeqDown::ids, FusedSeqDown::N)) f.program = 0;
        else if (matches(FusedSeqUpA::ids, FusedSeqUpA::N)) f.program = 1;
        else if (matches(FusedSeqUpB::ids, FusedSeqUpB::N)) f.program = 2;
        else if (matches(FusedSeqUpAB::ids, FusedSeqUpAB::N)) f.program = 3;
        else if (matches(FusedSeqMid2::ids, FusedSeqMid2::N)) f.program = 4;
        else if (matches(FusedSeqDown3::ids, FusedSeqDown3::N)) f.program = 5;
        else if (matches(FusedSeqMid3::ids, FusedSeqMid3::N)) f.program = 6;
        // the static programs with a geometry table read their LDS layout as compile-time constants (fused_geom.hpp): the layout computed
        // by the stages above must BE that table, otherwise the segment runs on the generic op-list kernel (runtime descriptors)
        const int sdim = u->cfg.state_dim;
        if ((f.program == 0 && !fused_geom_matches(a, GeomDown::g, sdim)) || (f.program == 3 && !fused_geom_matches(a, GeomUpAB::g, sdim)) ||
            (f.program == 5 && !fused_geom_matches(a, GeomDown3::g, sdim)) || (f.program == 6 && !fused_geom_matches(a, GeomMid3::g, sdim))) {
            if (debug_fuse_level()) fprintf(stderr, "[mpdx] fused segment: geometry differs from the table of program %d -> generic kernel\n", f.program);
            f.program = -1;
        }
    }

    // MPDX_DEBUG_FUSE: the segment (to be u->fused[index]) in one line; from level 2 on its LDS geometry as a fused_geom.hpp initialiser ahead of it
    void dump(size_t index) const {
        if (debug_fuse_level() >= 2) {
            fprintf(stderr, "// program %d: layers [%d,%d) %s..%s, LDS %zu B\n{ %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, {\n", f.program, i0, i1,
                    u->layers[i0].name.c_str(), u->layers[i1 - 1].name.c_str(), f.lds_bytes, a.nops, a.in_off4, a.in_rs4, a.in_rows, a.L0,
                    (a.gc1 == u->cfg.state_dim && a.gc2 == 0) ? -1 : a.gc1, a.gc2, a.c3, a.L3, a.s3_off4, a.s3_rs4, a.s3_col4, a.stat_off, a.par_off, with_final ? -1 : a.par_floats, a.tt_off,
                    a.tt_n, a.fpar_off, with_final ? a.H : 0, with_final ? a.Cf : 0);
            for (int k = 0; k < a.nops; ++k) {
                const FusedOp& o = a.ops[k];
                fprintf(stderr, "    {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d},\n", o.shape, o.src_off4, o.src_rs4, o.rsrc_off4, o.rsrc_rs4, o.res_off4, o.res_rs4,
                        o.dst_off4, o.dst_rs4, o.gdst, o.p_off, o.tb_off);
            }
            fprintf(stderr, "}},\n");
        }
        if (debug_fuse_level())
            fprintf(stderr, "[mpdx] fused segment %zu: layers [%d,%d) %s..%s  %d ops  %zu buffers  LDS %zu B  streams+params %zu floats  program %d\n",
                    index, i0, i1, u->layers[i0].name.c_str(), u->layers[i1 - 1].name.c_str(), a.nops, bufs.size(), f.lds_bytes,
                    area - (size_t)a.ops[0].sbase, f.program);
    }

    // true: the segment is u->fused.back() and its streams + parameter block have their place in `packed`; false: the handle is as it was
    bool build() {
        if (!collect_ops()) return false;
        place_buffers();
        if (!lay_out_streams_and_params() || !lay_out_tail()) return false;
        match_program();
        dump(u->fused.size());
        u->packed_floats = area;
        u->fused.push_back(f);
        return true;
    }
};

// which layer ranges of the network run as programs: u->fused and u->owner.  The ORDER of the attempts is part of the interface (segment indices,
// MPDX_FUSED_MASK bits)
static void build_units(mpdx_unet* u) {
    const int nl = u->cfg.n_levels;
    const int n = (int)u->layers.size();
    std::vector<int> owner(n, -1);
    // a horizon in a zero-padded container: every layer as its own (masking) launch.  Self-attention: a block sits between a level's second residual
    // block and its resample, which the whole-trajectory programs run back to back in LDS - every layer as its own launch (the convolutions keep
    // their pairs and weight-stationary variants)
    if (u->masked() || u->cfg.self_attention) { u->owner = owner; return; }
    auto range_of = [&](const std::string& prefix, int& i0, int& i1) {
        i0 = -1; i1 = -1;
        for (int i = 0; i < n; ++i)
            if (u->layers[i].name.compare(0, prefix.size(), prefix) == 0) { if (i0 < 0) i0 = i; i1 = i + 1; }
        return i0 >= 0;
    };
    // the layers of several prefixes when every one exists and each starts where the one before it ends
    auto span_of = [&](std::initializer_list<std::string> prefixes, int& i0, int& i1) {
        i0 = -1;
        for (const std::string& p : prefixes) {
            int b0, b1;
            if (!range_of(p, b0, b1) || (i0 >= 0 && b0 != i1)) return false;
            if (i0 < 0) i0 = b0;
            i1 = b1;
        }
        return true;
    };
    auto before_final = [&](int i1) { return i1 == n - 1 && u->layers[n - 1].name.compare(0, 12, "final_conv.0") == 0; };
    // layers [i0, i1) as one program, if none of them has an owner yet and the segment builds
    auto claim = [&](int i0, int i1, bool with_final) {
        for (int i = i0; i < i1; ++i) if (owner[i] >= 0) return false;
        if (!SegmentBuilder(u, i0, i1, with_final).build()) return false;
        for (int i = i0; i < i1; ++i) owner[i] = (int)u->fused.size() - 1;
        return true;
    };
    auto try_seg = [&](const std::string& prefix, bool with_final) {
        int i0, i1;
        if (!range_of(prefix, i0, i1)) return;
        if (with_final) {
            if (!before_final(i1)) return;
            i1 = n;
        }
        claim(i0, i1, with_final);
    };
    auto ups = [&](int j) { return "ups." + std::to_string(j) + "."; };
    const bool merge = !sw::no_merge();
    int i0, i1;
    // the outer down levels as ONE program if it fits (every launch boundary + prologue removed is ~5 us per step): with four
    // levels downs.0 + downs.1 + downs.2 (15 ops; measured cfg 2 23.10 -> 22.47 ms, cfg 5 shard 624 -> 617 ms against two programs;
    // MPDX_MERGE_DOWN3=0 keeps them apart), else downs.0 + downs.1
    bool merged_down = nl >= 4 && merge && sw::merge_down3() && span_of({"downs.0.", "downs.1.", "downs.2."}, i0, i1) && claim(i0, i1, false);
    if (!merged_down) merged_down = nl >= 3 && merge && span_of({"downs.0.", "downs.1."}, i0, i1) && claim(i0, i1, false);
    if (!merged_down) {
        try_seg("downs.0.", false);
        if (nl >= 3) try_seg("downs.1.", false);
    }
    // the third down level (C = 128, L = 16: two tile rows per wave) as its own program
    if (nl >= 4 && !sw::no_mid2()) try_seg("downs.2.", false);
    // three levels: the innermost level (no Downsample1d) and the two middle blocks - eight Conv1dBlocks of 128 channels on L / 4 positions - as ONE
    // program (round 6; they were nine launches of ~4.8 us: a training iteration at batch 32 spent 43 us there).  MPDX_NO_MID3=1: per layer as before
    if (nl == 3 && !sw::no_mid3() && span_of({"downs.2.", "mid_block1.", "mid_block2."}, i0, i1)) claim(i0, i1, false);
    // the two outer up levels + final_conv + DDPM step as ONE program (the second level's skip tensor is staged by the prologue)
    const bool merged_up = nl >= 3 && !sw::no_merge_up() && merge && span_of({ups(nl - 3), ups(nl - 2)}, i0, i1) && before_final(i1) && claim(i0, n, true);
    if (!merged_up) {
        if (nl >= 3) try_seg(ups(nl - 3), false);
        try_seg(ups(nl - 2), true);
    }
    u->owner = owner;
}

}  // namespace mpdx
