// unet_measure.hpp - the measurement and trace entry points of the U-Net pass (bench.py's roofline leg, tools/*_trace.py, tools/time_layer.py) and the
// launch-unit queries, over the launch functions of mpdx.hip: it includes this header behind walk_pass and PlanSchedule, and it alone.  No device code.
#pragma once
#include "host.hpp"

namespace mpdx {

// ---- owners: whatever an entry point creates is released on every return path
struct __attribute__((visibility("hidden"))) Events {
    std::vector<hipEvent_t> ev;
    int create(int n) { ev.assign(n, nullptr); for (hipEvent_t& e : ev) HIP_TRY(hipEventCreate(&e)); return 0; }
    hipEvent_t operator[](int i) const { return ev[i]; }
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
struct __attribute__((visibility("hidden"))) DevStamps {   // zeroed stamp buffer of a traced launch
    long long* p = nullptr;
    int alloc(size_t n, hipStream_t st) { HIP_TRY(hipMalloc(&p, n * sizeof(long long))); HIP_TRY(hipMemsetAsync(p, 0, n * sizeof(long long), st)); return 0; }
    ~DevStamps() { if (p) (void)hipFree(p); }
};
struct __attribute__((visibility("hidden"))) CapturedGraph {   // a stream capture (capturing: the stream, while it lasts) and the graph / executable made from it
    hipStream_t capturing = nullptr; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    ~CapturedGraph() {
        if (capturing) (void)hipStreamEndCapture(capturing, &graph);   // an error inside the captured region: the stream leaves capture mode
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};
template <class T>
struct ResetOnExit { T& ref; T value; ~ResetOnExit() { ref = value; } };   // a trace global points into a DevStamps only while its entry point runs

// the eps sink of the measurement entries: a library-owned buffer for one pass's output at batch B (grown on demand, never handed out) as the
// mode-0 FinalArgs that writes it
static int eps_sink(const mpdx_unet* u, int B, FinalArgs& fa) {
    static float* scratch = nullptr;
    static size_t scratch_n = 0;
    const size_t need = (size_t)B * u->cfg.n_support_points * u->cfg.state_dim;
    if (scratch_n < need) {
        if (scratch) { (void)hipFree(scratch); scratch = nullptr; scratch_n = 0; }
        HIP_TRY(hipMalloc(&scratch, need * sizeof(float)));
        scratch_n = need;
    }
    memset(&fa, 0, sizeof(fa));
    fa.out = scratch; fa.mode = 0; fa.n_per_ctx = 1;
    return 0;
}

// what the timing entries share: argument checks, the launch units of batch B, the eps sink and the time-table row
struct __attribute__((visibility("hidden"))) MeasuredPass {
    std::vector<mpdx_unet::Unit> units; bool final_in_fused = false;
    FinalArgs fa; const float* row = nullptr;
    int prepare(mpdx_unet* u, const float* timetab, int T, int t, int B) {
        if (int rc = check_ready(u)) return rc;
        if (t < 0 || t >= T) return fail(MPDX_E_INVALID, "timestep %d outside [0,%d)", t, T);
        units = current_units(u, B, &final_in_fused);
        row = timetab + (size_t)t * u->tt_row;
        return eps_sink(u, B, fa);
    }
};

static std::string fused_unit_name(const mpdx_unet* u, const mpdx_unet::Fused& f) {
    const std::string& first = u->layers[f.first].name;
    return "fused[" + first.substr(0, first.find(".blocks")) + "..+" + std::to_string(f.count) + (f.has_final ? " layers+final_conv.1+ddpm_step]" : " layers]");
}

static bool unit_at(const mpdx_unet* u, int B, int i, mpdx_unet::Unit& un) {
    if (!u) return false;
    const auto units = current_units(u, B, nullptr);
    if (i < 0 || i >= (int)units.size()) return false;
    un = units[i];
    return true;
}

}  // namespace mpdx

extern "C" {

int mpdx_unet_profile(mpdx_unet* u, const float* packed, const float* timetab, int T, const float* x, int t, int B, float* ws,
                      void* stream, int cap, float* ms_out, double* flops_out, const char** names_out, int* n_out) {
    if (!u || !packed || !timetab || !x || !ws || !ms_out || !n_out) return fail(MPDX_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    MeasuredPass p;
    if (int rc = p.prepare(u, timetab, T, t, B)) return rc;
    const int nu = (int)p.units.size(), nl = nu + (p.final_in_fused ? 0 : 1);
    if (cap < nl) return fail(MPDX_E_INVALID, "need room for %d launches", nl);
    static std::vector<std::string> fused_names;   // names_out points into it until the next call
    fused_names.resize(u->fused.size());
    for (int i = 0; i < nl; ++i) {
        const char* name = "final_conv.1+ddpm_step";
        if (i < nu && p.units[i].kind == mpdx_unet::kProgram) name = (fused_names[p.units[i].fused] = fused_unit_name(u, u->fused[p.units[i].fused])).c_str();
        else if (i < nu) name = u->layers[p.units[i].layer].name.c_str();
        if (names_out) names_out[i] = name;
        if (flops_out) flops_out[i] = i < nu ? unit_flops(u, p.units[i], B) : 0.0;
    }
    Events ev;
    if (int rc = ev.create(2 * nl)) return rc;
    auto bracket = [&](PassEvent e, int i) -> int {   // one event pair per launch, the final kernel's included
        if (e != kSkipUnit) HIP_TRY(hipEventRecord(ev[2 * i + (e == kAfterLaunch ? 1 : 0)], st));
        return 0;
    };
    if (int rc = walk_pass(u, p.units, packed, p.row, x, ws, B, p.fa, st, bracket)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < nl; ++i) HIP_TRY(hipEventElapsedTime(&ms_out[i], ev[2 * i], ev[2 * i + 1]));
    *n_out = nl;
    return 0;
}

/* dev tool: one launch of layer `layer` with s_memtime stamps (7 per workgroup) of the first and the last workgroup */
int mpdx_layer_trace(mpdx_unet* u, const float* packed, const float* timetab, const float* x, int layer, int B, float* ws, void* stream,
                     long long* stamps32) {
    if (int rc = dev_hooks_missing(__func__)) return rc;
    if (!u || layer < 0 || layer >= (int)u->layers.size() || !stamps32) return fail(MPDX_E_INVALID, "bad argument");
    if (int rc = check_ready(u)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevStamps dev;
    if (int rc = dev.alloc(32, st)) return rc;
    ResetOnExit<long long*> untrace{g_conv_trace, nullptr};
    g_conv_trace = dev.p;
    if (int rc = run_layer(u, u->layers[layer], packed, timetab, x, ws, B, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(stamps32, dev.p, 32 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

/* dev tool: run fused segment `seg` once with per-phase s_memtime stamps of workgroup 0 / wave 0; stamps_out[n].
 * seg == number of segments: the JOINED launch of mpdx_plan (up program of a pass + down program of the next, fused_join_kernel), in the same context;
 * its stamps are the up program's, one after the junction's barrier, then five per down op as far as a wave's 128 slots reach; *nops_out = both programs' ops */
int mpdx_fused_trace(mpdx_unet* u, const float* packed, const float* timetab, const float* x, int seg, int B, float* ws, void* stream,
                     long long* stamps_out, int cap, int* n_out, int* nops_out) {
    if (int rc = dev_hooks_missing(__func__)) return rc;
    if (!u || seg < 0 || seg > (int)u->fused.size() + 2) return fail(MPDX_E_INVALID, "bad segment");
    if (B <= 0) return fail(MPDX_E_INVALID, "B must be positive");
    const int nseg = (int)u->fused.size();
    const bool joined = seg == nseg;
    // seg == number of segments + 1 / + 2: the seven-layer run / the tail run of mpdx_plan (inner_run.hpp) - kRunTraceSlots stamps per layer, workgroup 0
    const int run_kind = seg == nseg + 1 ? (int)mpdx_unet::kInnerRun : seg == nseg + 2 ? (int)mpdx_unet::kTailRun : -1;
    PlanSchedule ps;   // (a program / the joined launch: without the runs - the per-layer units of the single-pass entry points)
    if (int rc = ps.build(u, B, run_kind >= 0)) return rc;
    if (joined && !ps.join) return fail(MPDX_E_INVALID, "bad segment (this network / batch has no joined launch)");
    int run_layers = 0;
    for (const auto& un : ps.units)
        if ((int)un.kind == run_kind) run_layers = un.count;
    if (run_kind >= 0 && !run_layers) return fail(MPDX_E_INVALID, "bad segment (this network / batch / handle setting does not select that run)");
    if (int rc = check_ready(u)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevStamps dev;
    if (int rc = dev.alloc(1024, st)) return rc;
    FinalArgs fa;
    if (int rc = eps_sink(u, B, fa)) return rc;
    // the traced launch runs IN CONTEXT: two untraced U-Net passes, then a third pass in which only segment `seg` stamps - same
    // predecessors, cache and clock state as in production, no host synchronisation in between
    ResetOnExit<long long*> untrace{g_fused_trace, nullptr};
    ResetOnExit<int> unselect{g_fused_trace_seg, -1};
    ResetOnExit<long long*> untrace_run{g_run_trace, nullptr};
    ResetOnExit<int> unselect_run{g_run_trace_kind, -1};
    for (int pass = 0; pass < 3; ++pass) {   // joined: the third pass as mpdx_plan runs it when the next one follows unguided - its last unit is the joined launch
        if (pass == 2 && run_kind >= 0) { g_run_trace = dev.p; g_run_trace_kind = run_kind; }
        else if (pass == 2 && !joined) { g_fused_trace = dev.p; g_fused_trace_seg = seg; }
        const float* next_row = pass == 2 && joined ? timetab : nullptr;
        if (int rc = walk_pass(u, ps.units, packed, timetab, padded_input(u, x, ws, B, st), ws, B, fa, st, no_hook, false, next_row, dev.p, ps.split)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    const int n = std::min(cap, 1024);   // 8 waves x 128 slots
    HIP_TRY(hipMemcpy(stamps_out, dev.p, n * sizeof(long long), hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    if (nops_out) {
        if (run_kind >= 0) *nops_out = run_layers;
        else if (joined) *nops_out =u->fused[ps.units.back().fused].tmpl.nops + u->fused[ps.units.front().fused].tmpl.nops;
        else *nops_out = u->fused[seg].tmpl.nops;
    }
    return 0;
}

/* in-situ timing: `reps` full U-Net passes; ONE event pair brackets launch units [unit_first, unit_last] of each pass
 * (so the bracketed kernels run in their real context - cold weights, real predecessor - and the event cost is
 * amortised over the run).  *ms_avg = average bracketed time per pass.  Synchronises. */
int mpdx_unet_time_units(mpdx_unet* u, const float* packed, const float* timetab, int T, const float* x, int t, int B, float* ws,
                         void* stream, int unit_first, int unit_last, int reps, float* ms_avg) {
    if (!u || !packed || !timetab || !x || !ws || !ms_avg || reps < 1) return fail(MPDX_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    MeasuredPass p;
    if (int rc = p.prepare(u, timetab, T, t, B)) return rc;
    if (unit_first < 0 || unit_last >= (int)p.units.size() || unit_first > unit_last) return fail(MPDX_E_INVALID, "bad unit range");
    Events ev;
    if (int rc = ev.create(2 * reps)) return rc;
    int r = 0;
    auto bracket = [&](PassEvent e, int i) -> int {
        if (e == kBeforeLaunch && i == unit_first) HIP_TRY(hipEventRecord(ev[2 * r], st));
        if (e == kAfterLaunch && i == unit_last) HIP_TRY(hipEventRecord(ev[2 * r + 1], st));
        return 0;
    };
    for (r = 0; r < reps; ++r)
        if (int rc = walk_pass(u, p.units, packed, p.row, x, ws, B, p.fa, st, bracket)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    double tot = 0.0;
    for (r = 0; r < reps; ++r) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1])); tot += ms; }
    *ms_avg = (float)(tot / reps);
    return 0;
}

/* measurement helper (bench.py roofline leg, the DIFFERENTIAL form): `reps` back-to-back U-Net passes WITHOUT the launch units whose bit is set in skip_mask
 * (0: nothing skipped) between ONE HIP-event pair on the launch stream -> average ms per pass.  The cost of a launch class inside
 * the pass = (pass with everything) - (pass without the class): no event pair sits next to the measured launches (an event pair around a single
 * 35-us launch adds ~5 us of marker processing + dispatch gap that the un-instrumented stream does not have).  The skipped units' consumers read
 * whatever the workspace holds: timing only, the output is not meaningful. */
int mpdx_unet_time_without(mpdx_unet* u, const float* packed, const float* timetab, int T, const float* x, int t, int B, float* ws,
                           void* stream, unsigned long long skip_mask, int reps, float* ms_avg) {
    if (!u || !packed || !timetab || !x || !ws || !ms_avg || reps < 1) return fail(MPDX_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    MeasuredPass p;
    if (int rc = p.prepare(u, timetab, T, t, B)) return rc;
    if (p.units.size() > 64) return fail(MPDX_E_INVALID, "more than 64 launch units");
    Events ev;
    if (int rc = ev.create(2)) return rc;
    auto without = [&](PassEvent e, int i) -> int { return e == kSkipUnit && ((skip_mask >> i) & 1ull); };
    for (int r = 0; r < 3; ++r)   // warm-up (code objects, clocks)
        if (int rc = walk_pass(u, p.units, packed, p.row, x, ws, B, p.fa, st, without)) return rc;
    HIP_TRY(hipEventRecord(ev[0], st));
    for (int r = 0; r < reps; ++r)
        if (int rc = walk_pass(u, p.units, packed, p.row, x, ws, B, p.fa, st, without)) return rc;
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *ms_avg = ms / (float)reps;
    return 0;
}

/* layer index of launch unit i (-1 for a fused unit / the final kernel): lets bench.py query the tile of a unit */
int mpdx_unet_unit_layer(const mpdx_unet* u, int B, int i) {
    mpdx_unet::Unit un;
    return (unit_at(u, B, i, un) && un.kind != mpdx_unet::kProgram) ? un.layer : -1;
}

/* which kernel runs fused segment `seg`: 0..5 = a static program (fused_program_kernel<FusedSeq...>; 0, 3, 5 read their LDS geometry from the
 * compile-time tables of fused_geom.hpp), -1 = the generic op-list kernel (runtime descriptors), -2 = no such segment */
int mpdx_unet_fused_program(const mpdx_unet* u, int seg) {
    if (!u || seg < 0 || seg >= (int)u->fused.size()) return -2;
    return u->fused[seg].program;
}

/* algorithmic bytes of launch unit i at batch B (weights once + boundary activations once); 0 for a bad index */
double mpdx_unet_unit_bytes(const mpdx_unet* u, int B, int i) {
    mpdx_unet::Unit un;
    return unit_at(u, B, i, un) ? unit_bytes(u, un, B) : 0.0;
}

/* 1 when launch unit i is a paired launch (blocks[0] + the block's residual 1x1 conv in one conv_pair_kernel) */
int mpdx_unet_unit_is_pair(const mpdx_unet* u, int B, int i) {
    mpdx_unet::Unit un;
    return (unit_at(u, B, i, un) && un.kind == mpdx_unet::kPair) ? 1 : 0;
}

int mpdx_bench_layer(mpdx_unet* u, const float* packed, const float* timetab, const float* x, int layer, int B, float* ws,
                     void* stream, int reps, int dbg, float* ms_per_launch) {
    if (!u || !packed || !timetab || !x || !ws || !ms_per_launch) return fail(MPDX_E_INVALID, "null argument");
    if (int rc = check_ready(u)) return rc;
    if (layer < 0 || layer >= (int)u->layers.size()) return fail(MPDX_E_INVALID, "bad layer index");
#ifndef MPDX_DEV_HOOKS
    if (dbg & 15) return fail(MPDX_E_STATE, "phase-ablation masks need a development build of libmpdx.so (MPDX_BUILD_DEFS=-DMPDX_DEV_HOOKS)");
#endif
    hipStream_t st = (hipStream_t)stream;
    const Layer& l = u->layers[layer];
    Events ev;
    if (int rc = ev.create(2)) return rc;
    for (int i = 0; i < 5; ++i)
        if (int rc = run_layer(u, l, packed, timetab, x, ws, B, st, dbg & 15)) return rc;
    CapturedGraph g;
    if (dbg & 16) {  // replay the same launches from a hipGraph (device-side launch cadence, no host in the loop)
        HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        g.capturing = st;
        for (int i = 0; i < reps; ++i)
            if (int rc = run_layer(u, l, packed, timetab, x, ws, B, st, dbg & 15)) return rc;
        g.capturing = nullptr;
        HIP_TRY(hipStreamEndCapture(st, &g.graph));
        HIP_TRY(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
        HIP_TRY(hipGraphLaunch(g.exec, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(hipGraphLaunch(g.exec, st));
        HIP_TRY(hipEventRecord(ev[1], st));
    } else {
        HIP_TRY(hipEventRecord(ev[0], st));
        for (int i = 0; i < reps; ++i)
            if (int rc = run_layer(u, l, packed, timetab, x, ws, B, st, dbg)) return rc;
        HIP_TRY(hipEventRecord(ev[1], st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *ms_per_launch = ms / reps;
    return 0;
}

int mpdx_unet_layer_tile(const mpdx_unet* u, int i, int B, char* buf, size_t buflen) {
    if (!u || !buf || i < 0 || i >= (int)u->layers.size()) return fail(MPDX_E_INVALID, "bad layer index");
    const Layer& l = u->layers[i];
    if (l.attn) { snprintf(buf, buflen, "attn %dx%d", attn_cols(l.cout, l.L_out) / l.L_out, l.L_out); return 0; }   // trajectories x positions per workgroup
    int MT, NT;
    ConvArgs dummy;
    memset(&dummy, 0, sizeof(dummy));
    const Layer* l2 = (i + 1 < (int)u->layers.size() && pair_tile(l, u->layers[i + 1], B, MT, NT)) ? &u->layers[i + 1] : nullptr;
    if (const int v = weight_stationary_variant(l, l2, dummy, B, 0)) {   // "ws": the weight-stationary persistent kernel (conv_ws.hpp)
        if (v == 6) snprintf(buf, buflen, "wsp 32x16/2x1+1x1");   // conv_wsp_kernel: a pair of waves per tile, whole K per wave
        else if (v >= 4) snprintf(buf, buflen, "wsn 16x16/8x1");   // conv_wsn_kernel: 8 waves = 8 position tiles, whole K per wave
        else snprintf(buf, buflen, "ws %dx16/1x8%s", v == 1 ? 32 : 16, v == 3 ? "+1x1" : "");
        return 0;
    }
    choose_tile(l, B, MT, NT);
    if (l.cout % MT) MT = 16;
    const bool ks = layer_ksplit(l);
    snprintf(buf, buflen, "%dx%d/%dx%d", MT, NT, ks ? 1 : NT / 16, ks ? 8 : 8 / (NT / 16));
    return 0;
}

}  // extern "C"
