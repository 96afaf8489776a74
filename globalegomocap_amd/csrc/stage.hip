// The optimisation calls of libgem_hip.so (include/gem_hip.h): which kernels a call runs (Route, decided once per call), the
// evaluation rounds of a stage and what each round reads and fills (RoundSet, built once per round and passed down), the two-stage
// window loop, hipGraph replay of whole calls, and the L-BFGS solver stepped alone for the parity tests.  Host code only: all
// arithmetic runs in the kernels of gemm_f32.hip, gemm_bf16.hip, decoder_bf16.hip, tail.hip, tail_bf16.hip, energy.hip, lbfgs.hip.
// No call leaves anything behind in the workspace for the next one except its buffers' contents and the n_log cursor.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>

#include "gem_internal.h"

namespace gem {

__global__ void fill_u32_kernel(uint32_t* __restrict__ p, uint32_t v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
static int launch_fill_u32(uint32_t* p, uint32_t v, size_t n, hipStream_t s) {
    if (!n) return 0;
    hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, v, n);
    GEM_HIP(hipGetLastError());
    return 0;
}


// ---- one route per call -------------------------------------------------------------------------------------------------------
// fp32 / bf16x3: the fused tail trades throughput for latency (~45 us per workgroup whatever the batch, one or two workgroups per CU
// at a time): measured against the batched GEMMs for the narrow layers it wins up to ten workgroups per CU in its two-per-CU shape,
// five otherwise (tail_cap_workgroups, tail.hip, has the table).
// bf16: the multi-window tail at every size (round 3 sent batches below 256 windows to the fp32 one-window tail; with ONE row tile per
// workgroup -- one window of ten frames, every window its own CU like the fp32 tail, round 4 -- the bf16 tail wins at every size: 60 /
// 120 / 240 windows 14.9 / 26.1 / 47.8 k windows/s against 11.1 / 20.6 / 38.7 k); GEM_TAIL16=0 forbids it, GEM_BATCHED_NARROW both
// tails (GEM_DEV=1; read per call: the tests flip them inside one process).
// The composed front layer exists only where the tail starts right behind conv 0 (gem_load_vae), so "it exists" is the whole test.
// Re-packing between the rounds: inside the first few-rows GEMM of the next round (one sequence in fp32: gemm_rows.h, FUSE); by
// lbfgs_advance handing out the next round's slots itself on every path whose kernels address rows through perm / slot_of only and do
// not depend on the slot ORDER -- front products (rows gathered through perm) + a fused tail (windows independent of their position in a
// workgroup: test_bf16_tail_row_tile_variants_compute_the_same) + lbfgs_advance (slot_of); else by compact_kernel (the batched
// narrow layers, taps = 3, read n_active[1] = rows and need its order).  No cap on B for the atomic slots: one same-address atomic
// per window and round is spread over the advance kernel's duration -- 8192 windows: 289.0 k against 282.3 k windows/s with
// compact_kernel's 12 us single-workgroup scan per round; 6144: +0.4 %.
Route plan_route(const gem_handle* h, int stage, int B, Call call) {
    const StageNet& net = h->net[stage];
    Route rt;
    rt.precision = h->precision;
    const bool bf16 = h->precision == GEM_PRECISION_BF16, have_tail = net.tail_start >= 1;
    const int tail_g = h->T <= 16 ? 16 / h->T : 1;
    rt.tail_wgs = (B + tail_g - 1) / tail_g;
    if (call == CALL_DECODE) {          // the batched layers of the fp32 entry points (their bf16 images in the bf16 mode, layer by layer)
        rt.front = !bf16 && net.front.w;
        return rt;
    }
    if (bf16) {
        const char* t16_env = dev_env("GEM_TAIL16");
        const bool batched_narrow = dev_env("GEM_BATCHED_NARROW") != nullptr;
        rt.front = net.front.wb_hi != nullptr;
        rt.tail_cap = 5 * h->n_cu;
        if (have_tail && !batched_narrow) {
            if (net.tb_stream && !(t16_env && t16_env[0] == '0')) rt.narrow = NARROW_TAIL_BF16;
            else if (rt.tail_wgs <= rt.tail_cap) rt.narrow = NARROW_TAIL_F32;
        }
        if (call == CALL_ROUNDS && rt.narrow == NARROW_TAIL_BF16 && rt.front) rt.repack = REPACK_ATOMIC;
        return rt;
    }
    rt.front = net.front.w != nullptr;
    rt.tail_cap = have_tail ? tail_cap_workgroups(h, net.dec, net.tail_start) : 0;
    if (have_tail && rt.tail_wgs <= rt.tail_cap) rt.narrow = NARROW_TAIL_F32;
    if (call == CALL_ROUNDS && rt.narrow == NARROW_TAIL_F32) {
        const Layer& first = rt.front ? net.front : net.dec_in;
        if (rows_can_fuse_compaction(h, first, h->Dp, first.N, B, /*slabs=*/rt.front)) rt.repack = REPACK_FUSED;
        else if (h->precision == GEM_PRECISION_F32 && rt.front) rt.repack = REPACK_ATOMIC;
    }
    return rt;
}

// ---- the rounds' view of the active windows --------------------------------------------------------------------------------------
// Round k of a run whose round 0 count lies at n_log[log0]: round k's count is logged at n_log[log0 + k] in every mode.  With atomic
// slots that entry IS the round's count (filled by lbfgs_advance of round k - 1) and the two (perm, slot_of) pairs alternate.
static RoundSet round_set(Workspace& w, long log0, int k, Repack mode) {
    RoundSet r;
    const bool odd = mode == REPACK_ATOMIC && (k & 1);
    r.perm = odd ? w.perm2 : w.perm;
    r.slot_of = mode == REPACK_NONE ? nullptr : odd ? w.slot_of2 : w.slot_of;
    r.n_active = w.n_active;
    r.log_idx = log0 + k;
    if (mode == REPACK_ATOMIC) {
        r.n_active = w.n_log + (log0 + k) % N_LOG;
        r.next_count = r.n_active + 1;
        r.next_perm = odd ? w.perm : w.perm2;
        r.next_slot_of = odd ? w.slot_of : w.slot_of2;
    }
    r.trace = k < TRACE_ROUNDS ? w.trace + (size_t)k * w.Bmax : nullptr;
    return r;
}

// Round 0: every window takes part (identity slots, B logged at n_log[*log0]).  counters > 0 (atomic slots): that many entries behind
// it are zeroed by the same kernel -- one per later round -- and the whole range is kept from wrapping around the ring.
static int begin_rounds(gem_handle* h, int B, int counters, hipStream_t s, long* log0) {
    Workspace& w = h->ws;
    if (counters && (w.log_pos % N_LOG) + counters + 1 > N_LOG) w.log_pos += N_LOG - (w.log_pos % N_LOG);
    *log0 = w.log_pos;
    if (launch_compact(h, round_set(w, *log0, 0, REPACK_KERNEL), B, 1, s, counters)) return 1;
    w.log_pos = *log0 + 1 + counters;
    return 0;
}

static int check_lbfgs_opts(const Workspace& w, const gem_lbfgs_opts& o, const char* who) {
    if (o.max_iter < 1 || o.max_eval < 1 || o.max_iter - 1 > w.hist_cap || o.max_iter > MAX_HIST) {
        set_error(std::string(who) + ": max_iter must be 1.." + std::to_string(w.hist_cap + 1)); return 1;
    }
    // (the per-round counters of a stage are zeroed by one 1024-thread workgroup, and the trace keeps TRACE_ROUNDS rounds)
    if (o.max_eval > 1021) { set_error(std::string(who) + ": max_eval must be at most 1021 (torch's default for max_iter = 25 is 31)"); return 1; }
    return 0;
}

static int check_call(gem_handle* h, int stage, int B, const char* who) {
    if (!h) { set_error(std::string(who) + ": null handle"); return 1; }
    if (stage < 0 || stage > 1 || !h->net[stage].loaded) { set_error(std::string(who) + ": VAE weights of this stage are not loaded"); return 1; }
    if (B < 0 || B > h->ws.Bmax) { set_error(std::string(who) + ": B exceeds max_windows"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    return 0;
}

static int encoder_forward(gem_handle* h, int stage, int B, const float* d_pose, hipStream_t s) {
    StageNet& net = h->net[stage];
    Workspace& w = h->ws;
    const int rows = B * h->T;
    if (launch_pack_pose(d_pose, w.pose_p, rows, h->C, s)) return 1;
    const float* in = w.pose_p;
    int lda = PAD;
    for (size_t i = 0; i < net.enc.size(); ++i) {
        if (launch_gemm(h, net.enc[i], EPI_BIAS_LRELU, in, lda, nullptr, w.enc_act[i], net.enc[i].N, rows, h->T, s, -1)) return 1;
        in = w.enc_act[i];
        lda = net.enc[i].N;
    }
    return launch_gemm(h, net.fc, EPI_BIAS, in, net.fc.K, nullptr, w.mulv, net.fc.N, B, h->T, s, -1);
}


// repack_log: the round's first launch also re-packs the active windows (REPACK_FUSED)
static int decoder_forward(gem_handle* h, const Route& rt, int stage, int B, const float* zp, hipStream_t s, const RoundSet* rs = nullptr,
                           int* repack_log = nullptr) {
    StageNet& net = h->net[stage];
    Workspace& w = h->ws;
    const int rows = B * h->T;
    const GemmOpts gathered(rs, rs ? rs->perm : nullptr, nullptr, repack_log), in_rounds(rs, nullptr);
    const float* in = w.h0;
    if (rt.front) {          // decoder_input o conv 0 as one product (compose_front)
        if (launch_gemm(h, net.front, EPI_BIAS_LRELU, zp, h->Dp, nullptr, w.dec_act[0], net.front.N, B, h->T, s, 0, gathered)) return 1;
        in = w.dec_act[0];
    } else if (launch_gemm(h, net.dec_in, EPI_BIAS, zp, h->Dp, nullptr, w.h0, net.dec_in.N, B, h->T, s, 0, gathered)) {
        return 1;
    }
    for (size_t i = rt.front ? 1 : 0; i < net.dec.size(); ++i) {
        const int epi = (i + 1 < net.dec.size()) ? EPI_BIAS_LRELU : EPI_BIAS;
        if (launch_gemm(h, net.dec[i], epi, in, net.dec[i].K, nullptr, w.dec_act[i], net.dec[i].N, rows, h->T, s, -1, in_rounds)) return 1;
        in = w.dec_act[i];
    }
    return 0;
}

// backward-data from decoder conv `from` down to the latent; gin = gradient w.r.t. the output of conv `from` (with the composed front
// layer: down to conv 1, then its transpose -- gin is then the gradient w.r.t. conv 0's pre-activation; replaces the conv adjoint, its
// reduce pass and the decoder_input backward product).  In the rounds lbfgs_advance sums the slabs of the last product itself (its
// bias is zero): *grad describes them.
static int decoder_backward(gem_handle* h, const Route& rt, int stage, int B, hipStream_t s, int from, const float* gin, const RoundSet* rs,
                            SlabSrc* grad) {
    StageNet& net = h->net[stage];
    Workspace& w = h->ws;
    const int rows = B * h->T;
    for (int i = from; i >= (rt.front ? 1 : 0); --i) {
        const Layer& L = net.dec_bwd[i];
        const float* aux = i > 0 ? w.dec_act[i - 1] : nullptr;      // LeakyReLU' from the sign of the stored activation
        if (launch_gemm(h, L, i > 0 ? EPI_MASK : EPI_NONE, gin, L.K, aux, w.dec_grad[i], L.N, rows, h->T, s, -1, GemmOpts(rs, nullptr))) return 1;
        gin = w.dec_grad[i];
    }
    const Layer& last = rt.front ? net.front_bwd : net.dec_in_bwd;
    return launch_gemm(h, last, EPI_BIAS, gin, last.K, nullptr, w.dz, h->Dp, B, h->T, s, 0, GemmOpts(rs, nullptr, rs ? grad : nullptr));
}

// tex: hand the texel-block cache of the reprojection term to the kernels (inside a stage only)
static EnergyArgs energy_args(gem_handle* h, const float* X0, const float* heat, const int32_t* frame0, const float* mean_bone,
                              const gem_energy_weights& wt, bool tex) {
    Workspace& w = h->ws;
    EnergyArgs a;
    a.Xp = w.dec_act.back(); a.X0 = X0; a.heat = heat; a.frame0 = frame0; a.mean_bone = mean_bone;
    a.dXp = w.dXp; a.dXp_b = nullptr; a.f = w.f; a.parts = w.parts;
    a.tex_key = tex ? w.tex_key : nullptr; a.tex_val = tex ? w.tex_val : nullptr;
    a.w3d = (float)wt.w3d; a.ws = (float)wt.smooth; a.wb = (float)wt.bone; a.wv = (float)wt.vae; a.wr = (float)wt.reproj;
    a.dw3d = wt.w3d; a.dws = wt.smooth; a.dwb = wt.bone; a.dwv = wt.vae; a.dwr = wt.reproj;
    a.T = h->T; a.J = h->J; a.H = h->cfg.heat_h; a.W = h->cfg.heat_w; a.n_poly = h->cfg.n_poly;
    for (int i = 0; i < GEM_MAX_POLY; ++i) a.poly[i] = i < h->cfg.n_poly ? (float)h->cfg.poly[i] : 0.f;
    a.cx = (float)h->cfg.cx; a.cy = (float)h->cfg.cy;
    a.parents = h->d_parents; a.children = h->d_children;
    a.n_dev = nullptr; a.perm = nullptr;          // all B windows in their own order; the rounds put their RoundSet's here
    return a;
}

void fill_tail_args(const gem_handle* h, const StageNet& net, const Route& rt, int B, bool forward_only, const SlabSrc& in_slab,
                    const EnergyArgs& ea, const RoundSet* rs, TailArgs* ta) {
    const Workspace& w = h->ws;
    const int st = net.tail_start;
    ta->B = B; ta->forward_only = forward_only ? 1 : 0; ta->dbg_ts = nullptr;
    ta->in_slab = in_slab; ta->in_bias = rt.front ? net.front.bias : net.dec[st - 1].bias;
    ta->in_bias_ld = rt.front ? net.dec[0].N : 0;
    for (int i = 0; i < ta->n; ++i) {
        const Layer& f = net.dec[st + i];
        const Layer& g = net.dec_bwd[st + i];
        ta->fwd[i] = TailLayerDev{f.w4, f.bias, f.K, f.N};
        ta->bwd[i] = TailLayerDev{g.w4, nullptr, g.K, g.N};
    }
    ta->a_in = w.dec_act[st - 1];
    ta->Xp = (rs && !forward_only) ? nullptr : w.dec_act.back();     // the pose is only read back outside the rounds
    ta->e = ea;
}

// One evaluation of the trial points zp (== ws.trial, mirrored in ws.trial_b in the bf16 mode): pose in ws.dec_act.back(), energies in
// ws.f / ws.parts, dE/dz in ws.dz -- or, in the rounds, as the slabs *grad describes.  forward_only: decode only (the final pose of
// a stage), same kernels.  repack_log: the round's first launch also re-packs the active windows (REPACK_FUSED: never planned for the
// bf16 mode).
static int evaluate(gem_handle* h, const Route& rt, int stage, int B, const float* zp, const EnergyArgs& ea, hipStream_t s, bool forward_only,
                    const RoundSet* rs, SlabSrc* grad, int* repack_log = nullptr) {
    StageNet& net = h->net[stage];
    Workspace& w = h->ws;
    *grad = SlabSrc{};
    if (rt.precision == GEM_PRECISION_BF16) return evaluate_bf16(h, rt, stage, B, ea, s, forward_only, rs, grad);
    if (rt.narrow == NARROW_BATCHED) {
        if (decoder_forward(h, rt, stage, B, zp, s, rs, repack_log)) return 1;
        if (forward_only) return 0;
        if (launch_energy(h, ea, B, s)) return 1;
        return decoder_backward(h, rt, stage, B, s, (int)net.dec.size() - 1, w.dXp, rs, grad);
    }
    // wide layers as batched GEMMs, the narrow tail + energy + its adjoints in one kernel; in the rounds the split-K slabs (if any)
    // of the product in front of the tail go to the tail kernel (sum + bias + LeakyReLU while staging)
    const int st = net.tail_start, rows = B * h->T;
    const int* perm = rs ? rs->perm : nullptr;
    SlabSrc in_slab;
    SlabSrc* to_tail = rs ? &in_slab : nullptr;
    if (rt.front) {
        if (launch_gemm(h, net.front, EPI_BIAS_LRELU, zp, h->Dp, nullptr, w.dec_act[0], net.front.N, B, h->T, s, 0,
                        GemmOpts(rs, perm, to_tail, repack_log))) return 1;
    } else {
        if (launch_gemm(h, net.dec_in, EPI_BIAS, zp, h->Dp, nullptr, w.h0, net.dec_in.N, B, h->T, s, 0, GemmOpts(rs, perm, nullptr, repack_log)))
            return 1;
        const float* in = w.h0;
        for (int i = 0; i < st; ++i) {
            if (launch_gemm(h, net.dec[i], EPI_BIAS_LRELU, in, net.dec[i].K, nullptr, w.dec_act[i], net.dec[i].N, rows, h->T, s, -1,
                            GemmOpts(rs, nullptr, i == st - 1 ? to_tail : nullptr))) return 1;
            in = w.dec_act[i];
        }
    }
    TailArgs ta;
    const size_t tail_lds = plan_tail_for(h, net.dec, st, rt.tail_wgs, &ta);
    fill_tail_args(h, net, rt, B, forward_only, in_slab, ea, rs, &ta);
    ta.g_out = w.dec_grad[st]; ta.g_out_b = nullptr;
    if (launch_tail(h, ta, tail_lds, s, rs)) return 1;
    if (forward_only) return 0;
    return decoder_backward(h, rt, stage, B, s, st - 1, w.dec_grad[st], rs, grad);
}

// One stage of B windows as three host steps: begin (encode, initial state), round r (one evaluation + one L-BFGS advance for
// every window still iterating), finish (decode the result).  optimize_stage_impl runs them back to back.
struct StageRun {
    gem_handle* h = nullptr;
    int stage = 0, B = 0;
    const float* pose_in = nullptr; const float* heat = nullptr; const int32_t* frame0 = nullptr; const float* mean_bone = nullptr;
    const float* eps = nullptr;
    gem_energy_weights wt{}; gem_lbfgs_opts opt{};
    float* pose_out = nullptr; gem_window_stats* stats = nullptr;
    hipStream_t s = nullptr;
    EnergyArgs ea{};
    Route route;
    long log0 = 0;                      // n_log entry of round 0's count (round k: log0 + k)
    int rounds = 0;
};

static int stage_begin(StageRun& r) {
    gem_handle* h = r.h;
    Workspace& w = h->ws;
    const int B = r.B, stage = r.stage;
    hipStream_t s = r.s;
    if (r.wt.reproj != 0.0 && (!r.heat || !r.frame0)) { set_error("optimize: reproj weight != 0 needs heat-maps and frame indices"); return 1; }
    if (check_lbfgs_opts(w, r.opt, "optimize")) return 1;
    r.rounds = r.opt.max_eval + 1;          // upper bound on evaluations per window (see lbfgs.hip)
    w.dbg_slots = -1;                       // (a debug run of the solver alone ends where a stage begins)
    if (encoder_forward(h, stage, B, r.pose_in, s)) return 1;
    if (launch_reparam(w.mulv, r.eps, nullptr, nullptr, nullptr, w.trial, B, h->D, h->Dp, s)) return 1;
    if (h->precision == GEM_PRECISION_BF16 && launch_f32_to_bf16(w.trial, w.trial_b, (size_t)B * h->Dp, s)) return 1;
    if (launch_lbfgs_init(h, B, s)) return 1;
    // Rounds run on the windows that are still iterating: after every advance they are re-packed to the front
    // (perm / n_active on the device) and the kernels of the next round read their row count from there.
    r.route = plan_route(h, stage, B, CALL_ROUNDS);
    if (begin_rounds(h, B, r.route.repack == REPACK_ATOMIC ? r.rounds + 1 : 0, s, &r.log0)) return 1;
    // texel-block cache of the reprojection term: valid for this stage's heat-maps / windows only
    const bool tex = h->tex_cache && w.tex_key && r.wt.reproj != 0.0;
    // (a fill KERNEL, not hipMemsetAsync: inside a captured graph a memset node was seen to run out of order with the kernels around it
    // once two graphs replayed side by side on two streams -- round 5, ROCm 7.2; a late invalidation here would hand the stage texels
    // of the previous contents of the heat-maps)
    if (tex && launch_fill_u32(reinterpret_cast<uint32_t*>(w.tex_key), 0xFFFFFFFFu, (size_t)B * h->T * h->J, s)) return 1;
    r.ea = energy_args(h, r.pose_in, r.heat, r.frame0, r.mean_bone, r.wt, tex);
    // closure values of this stage, one row per round (0xFF bytes = NaN: "window took no evaluation in this round")
    return launch_fill_u32(reinterpret_cast<uint32_t*>(w.trace), 0xFFFFFFFFu, (size_t)TRACE_ROUNDS * w.Bmax * 2, s);
}

static int stage_round(StageRun& r, int k) {
    gem_handle* h = r.h;
    Workspace& w = h->ws;
    const Repack mode = r.route.repack;
    const RoundSet rs = round_set(w, r.log0, k, mode);
    // the windows that went on iterating in round k - 1 move to the front: by compact_kernel here, by the round's first GEMM
    // (launch_rows refuses if it cannot), or they already have (atomic slots)
    int* repack_log = nullptr;
    if (k > 0 && mode != REPACK_ATOMIC) {
        if (mode == REPACK_FUSED) repack_log = w.n_log + rs.log_idx % N_LOG;
        else if (launch_compact(h, rs, r.B, 0, r.s)) return 1;
        w.log_pos = rs.log_idx + 1;
    }
    r.ea.n_dev = rs.n_active; r.ea.perm = rs.perm;
    SlabSrc grad;
    if (evaluate(h, r.route, r.stage, r.B, w.trial, r.ea, r.s, false, &rs, &grad, repack_log)) return 1;
    return launch_lbfgs_advance(h, r.B, r.opt, rs, grad, r.s);
}

static int stage_finish(StageRun& r) {
    gem_handle* h = r.h;
    Workspace& w = h->ws;
    // every window is finished now: trial == x*; decode it with the same kernels as the rounds (all windows again)
    SlabSrc none;
    if (evaluate(h, r.route, r.stage, r.B, w.trial, energy_args(h, r.pose_in, r.heat, r.frame0, r.mean_bone, r.wt, false), r.s, true, nullptr, &none))
        return 1;
    if (launch_unpack_pose(w.dec_act.back(), r.pose_out, r.B * h->T, h->C, r.s)) return 1;
    if (r.stats && launch_lbfgs_stats(h, r.B, r.stats, r.s)) return 1;
    return 0;
}

static int optimize_stage_impl(gem_handle* h, int stage, int B, const float* d_pose_in, const float* d_heat,
                               const int32_t* d_frame0, const float* d_mean_bone, const float* d_eps,
                               const gem_energy_weights& wt, const gem_lbfgs_opts& opt, float* d_pose_out,
                               gem_window_stats* d_stats, hipStream_t s) {
    StageRun r;
    r.h = h; r.stage = stage; r.B = B; r.pose_in = d_pose_in; r.heat = d_heat; r.frame0 = d_frame0; r.mean_bone = d_mean_bone; r.eps = d_eps;
    r.wt = wt; r.opt = opt; r.pose_out = d_pose_out; r.stats = d_stats; r.s = s;
    int rc = stage_begin(r);
    for (int k = 0; k < r.rounds && !rc; ++k) rc = stage_round(r, k);
    return rc || stage_finish(r);
}

// ---- both stages of the window loop (optimizer.py:370-423), as host steps around the stage rounds ---------------------------
struct WindowsRun {
    gem_handle* h = nullptr;
    int B = 0;
    const float* local_pose = nullptr; const double* cams = nullptr; const float* heat = nullptr; const int32_t* frame0 = nullptr;
    const float* mean_bone = nullptr; const float* eps_local = nullptr; const float* eps_global = nullptr;
    gem_energy_weights w_local{}, w_global{}; gem_lbfgs_opts opt{};
    float* mid_local = nullptr; double* global = nullptr; gem_window_stats* stats_local = nullptr; gem_window_stats* stats_global = nullptr;
    hipStream_t s = nullptr;
    StageRun st;
    float* mid = nullptr;
};

static int windows_begin_local(WindowsRun& r) {
    gem_handle* h = r.h;
    Workspace& w = h->ws;
    if (launch_gather_windows(r.local_pose, r.frame0, w.pose_a, r.B, h->T, h->C, r.s)) return 1;
    r.mid = r.mid_local ? r.mid_local : w.pose_b;
    StageRun& s = r.st;
    s = StageRun{};
    s.h = h; s.stage = GEM_STAGE_LOCAL; s.B = r.B; s.pose_in = w.pose_a; s.heat = r.heat; s.frame0 = r.frame0; s.mean_bone = r.mean_bone;
    s.eps = r.eps_local; s.wt = r.w_local; s.opt = r.opt; s.pose_out = r.mid; s.stats = r.stats_local; s.s = r.s;
    return stage_begin(s);
}
static int windows_begin_global(WindowsRun& r) {       // local stage -> fp64 relative-global transform -> global stage set up
    gem_handle* h = r.h;
    Workspace& w = h->ws;
    if (stage_finish(r.st)) return 1;
    if (launch_relative_global(r.mid, r.cams, r.frame0, w.pose_a, r.B, h->T, h->J, r.s)) return 1;
    StageRun& s = r.st;
    s = StageRun{};
    s.h = h; s.stage = GEM_STAGE_GLOBAL; s.B = r.B; s.pose_in = w.pose_a; s.heat = r.heat; s.frame0 = r.frame0; s.mean_bone = r.mean_bone;
    s.eps = r.eps_global; s.wt = r.w_global; s.opt = r.opt; s.pose_out = w.pose_b;      // (the stage-A result kept there, if any, is dead after the transform)
    s.stats = r.stats_global; s.s = r.s;
    return stage_begin(s);
}
static int windows_end(WindowsRun& r) {
    gem_handle* h = r.h;
    if (stage_finish(r.st)) return 1;
    return launch_to_global(h->ws.pose_b, r.cams, r.frame0, r.global, r.B, h->T, h->J, r.s);
}

static int windows_single(WindowsRun& r) {
    int rc = windows_begin_local(r);
    for (int k = 0; k < r.st.rounds && !rc; ++k) rc = stage_round(r.st, k);
    rc = rc || windows_begin_global(r);
    for (int k = 0; k < r.st.rounds && !rc; ++k) rc = stage_round(r.st, k);
    return rc || windows_end(r);
}

// ---- hipGraph replay of a whole call ------------------------------------------------------------------------------------
// An optimisation call is a fixed sequence of ~700 launches whose grids and arguments do not depend on the data (row counts
// live on the device, finished windows are skipped inside the kernels), i.e. it is capture-safe as it stands.  With graphs
// enabled, the first call with a given signature runs eagerly (it also performs the one-time hipFuncSetAttribute settings),
// the second one is captured into a hipGraph and instantiated, every later one is a single hipGraphLaunch: the host cost of a
// call drops from ~3 ms of launches to one launch (BASELINE configs[4]; several sequences in flight from one host thread).
static bool same_key(const GraphKey& a, const GraphKey& b) {
    if (a.kind != b.kind || a.stage != b.stage || a.B != b.B || a.precision != b.precision || a.stream != b.stream || a.tex_cache != b.tex_cache)
        return false;
    for (int i = 0; i < 12; ++i)
        if (a.ptr[i] != b.ptr[i]) return false;
    return std::memcmp(a.w, b.w, sizeof(a.w)) == 0 && std::memcmp(&a.opt, &b.opt, sizeof(a.opt)) == 0;
}

template <typename Body>
static int run_graphed(gem_handle* h, const GraphKey& key, hipStream_t s, Body body) {
    // the legacy default stream cannot be captured; event-based profiling records events between launches
    if (!h->graphs_on || s == nullptr || h->prof.on) return body();
    GraphEntry* e = nullptr;
    for (auto& g : h->graphs)
        if (same_key(g.key, key)) { e = &g; break; }
    ++h->graph_tick;
    if (!e) {                                   // first sighting: eager run (warm-up), remember the signature
        if (h->graphs.size() >= 16) {           // bounded cache: drop the least recently used entry
            size_t lru = 0;
            for (size_t i = 1; i < h->graphs.size(); ++i)
                if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
            if (h->graphs[lru].exec) (void)hipGraphExecDestroy(h->graphs[lru].exec);
            if (h->graphs[lru].graph) (void)hipGraphDestroy(h->graphs[lru].graph);
            h->graphs.erase(h->graphs.begin() + lru);
        }
        GraphEntry n;
        n.key = key; n.last_use = h->graph_tick;
        h->graphs.push_back(n);
        return body();
    }
    e->last_use = h->graph_tick;
    if (!e->exec) {
        GEM_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int rc = body();
        hipGraph_t g = nullptr;
        const hipError_t ec = hipStreamEndCapture(s, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (!hip_ok(ec, "hipStreamEndCapture")) return 1;
        hipGraphExec_t x = nullptr;
        if (!hip_ok(hipGraphInstantiate(&x, g, nullptr, nullptr, 0), "hipGraphInstantiate")) { (void)hipGraphDestroy(g); return 1; }
        e->graph = g; e->exec = x;
        ++h->graph_captures;
    }
    GEM_HIP(hipGraphLaunch(e->exec, s));
    ++h->graph_replays;
    return 0;
}

}  // namespace gem

using namespace gem;

extern "C" {

int gem_encode(gem_handle* h, int stage, int B, const float* d_pose, const float* d_eps, float* d_mu, float* d_logvar,
               float* d_z, void* stream) {
    if (check_call(h, stage, B, "gem_encode")) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return 0;
    if (encoder_forward(h, stage, B, d_pose, s)) return 1;
    return launch_reparam(h->ws.mulv, d_eps, d_mu, d_logvar, d_z, nullptr, B, h->D, h->Dp, s);
}

int gem_decode(gem_handle* h, int stage, int B, const float* d_z, float* d_pose, void* stream) {
    if (check_call(h, stage, B, "gem_decode")) return 1;
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return 0;
    if (launch_pad_latent(d_z, h->ws.trial, B, h->D, h->Dp, s)) return 1;
    if (decoder_forward(h, plan_route(h, stage, B, CALL_DECODE), stage, B, h->ws.trial, s)) return 1;
    return launch_unpack_pose(h->ws.dec_act.back(), d_pose, B * h->T, h->C, s);
}

int gem_energy_grad(gem_handle* h, int stage, int B, const float* d_z, const float* d_pose_init, const float* d_heat,
                    const int32_t* d_frame0, const float* d_mean_bone, const gem_energy_weights* wt, double* d_energy,
                    double* d_parts, float* d_dz, float* d_pose, void* stream) {
    if (check_call(h, stage, B, "gem_energy_grad")) return 1;
    if (B == 0) return 0;
    if (!wt || !d_z || !d_pose_init || !d_mean_bone) { set_error("gem_energy_grad: null argument"); return 1; }
    if (wt->reproj != 0.0 && (!d_heat || !d_frame0)) { set_error("gem_energy_grad: reproj weight != 0 needs heat-maps"); return 1; }
    hipStream_t s = (hipStream_t)stream;
    Workspace& w = h->ws;
    if (launch_pad_latent(d_z, w.trial, B, h->D, h->Dp, s)) return 1;
    if (h->precision == GEM_PRECISION_BF16 && launch_f32_to_bf16(w.trial, w.trial_b, (size_t)B * h->Dp, s)) return 1;
    const EnergyArgs ea = energy_args(h, d_pose_init, d_heat, d_frame0, d_mean_bone, *wt, false);
    SlabSrc none;          // (outside the rounds the gradient is finished in ws.dz)
    if (evaluate(h, plan_route(h, stage, B, CALL_EVALUATE), stage, B, w.trial, ea, s, false, nullptr, &none)) return 1;
    if (d_energy) GEM_HIP(hipMemcpyAsync(d_energy, w.f, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (d_parts) GEM_HIP(hipMemcpyAsync(d_parts, w.parts, (size_t)B * 5 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (d_dz && launch_unpad_latent(w.dz, d_dz, B, h->D, h->Dp, s)) return 1;
    if (d_pose && launch_unpack_pose(w.dec_act.back(), d_pose, B * h->T, h->C, s)) return 1;
    return 0;
}

int gem_optimize_stage(gem_handle* h, int stage, int B, const float* d_pose_in, const float* d_heat, const int32_t* d_frame0,
                       const float* d_mean_bone, const float* d_eps, const gem_energy_weights* wt, const gem_lbfgs_opts* opt,
                       float* d_pose_out, gem_window_stats* d_stats, void* stream) {
    if (check_call(h, stage, B, "gem_optimize_stage")) return 1;
    if (B == 0) return 0;
    if (!d_pose_in || !d_mean_bone || !wt || !opt || !d_pose_out) { set_error("gem_optimize_stage: null argument"); return 1; }
    GraphKey key;
    key.kind = 1; key.stage = stage; key.B = B; key.precision = h->precision; key.stream = stream; key.tex_cache = h->tex_cache;
    const void* ptrs[] = {d_pose_in, d_heat, d_frame0, d_mean_bone, d_eps, d_pose_out, d_stats};
    for (int i = 0; i < 7; ++i) key.ptr[i] = ptrs[i];
    key.w[0] = *wt; key.opt = *opt;
    return run_graphed(h, key, (hipStream_t)stream, [&]() {
        return optimize_stage_impl(h, stage, B, d_pose_in, d_heat, d_frame0, d_mean_bone, d_eps, *wt, *opt, d_pose_out, d_stats,
                                   (hipStream_t)stream);
    });
}

int gem_optimize_windows(gem_handle* h, int B, const float* d_local_pose, const double* d_cams, const float* d_heat,
                         const int32_t* d_frame0, const float* d_mean_bone, const float* d_eps_local, const float* d_eps_global,
                         const gem_energy_weights* w_local, const gem_energy_weights* w_global, const gem_lbfgs_opts* opt,
                         float* d_mid_local, double* d_global, gem_window_stats* d_stats, void* stream) {
    if (check_call(h, 0, B, "gem_optimize_windows") || check_call(h, 1, B, "gem_optimize_windows")) return 1;
    if (B == 0) return 0;
    if (!d_local_pose || !d_cams || !d_frame0 || !d_mean_bone || !w_local || !w_global || !opt || !d_global) {
        set_error("gem_optimize_windows: null argument"); return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    GraphKey key;
    key.kind = 2; key.B = B; key.precision = h->precision; key.stream = stream; key.tex_cache = h->tex_cache;
    const void* ptrs[] = {d_local_pose, d_cams, d_heat, d_frame0, d_mean_bone, d_eps_local, d_eps_global, d_mid_local, d_global, d_stats};
    for (int i = 0; i < 10; ++i) key.ptr[i] = ptrs[i];
    key.w[0] = *w_local; key.w[1] = *w_global; key.opt = *opt;
    return run_graphed(h, key, s, [&]() -> int {
        WindowsRun a;
        a.h = h; a.B = B; a.local_pose = d_local_pose; a.cams = d_cams; a.heat = d_heat; a.frame0 = d_frame0; a.mean_bone = d_mean_bone;
        a.eps_local = d_eps_local; a.eps_global = d_eps_global; a.w_local = *w_local; a.w_global = *w_global; a.opt = *opt;
        a.mid_local = d_mid_local; a.global = d_global; a.stats_local = d_stats; a.stats_global = d_stats ? d_stats + B : nullptr; a.s = s;
        return windows_single(a);
    });
}

int gem_read_trace(gem_handle* h, int B, int n_rounds, double* d_out, void* stream) {
    if (!h || !d_out || B < 0 || B > h->ws.Bmax || n_rounds < 0 || n_rounds > TRACE_ROUNDS) {
        set_error("gem_read_trace: need 0 <= B <= max_windows and 0 <= n_rounds <= 64"); return 1;
    }
    GEM_HIP(hipSetDevice(h->cfg.device));
    if (B == 0 || n_rounds == 0) return 0;
    GEM_HIP(hipMemcpy2DAsync(d_out, (size_t)B * sizeof(double), h->ws.trace, (size_t)h->ws.Bmax * sizeof(double),
                             (size_t)B * sizeof(double), (size_t)n_rounds, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ---- for parity tests: the L-BFGS state machine stepped alone (include/gem_hip.h) ---------------------------------------------
// The caller plays the decoder and the energy.  Every launch goes through the launchers and the round helpers of a stage; a session
// is the four dbg_* cursors of the workspace and nothing else.
static const int DBG_MAX_ROUNDS = 1022;          // max_eval <= 1021 (check_lbfgs_opts): at most max_eval + 1 rounds
static Repack dbg_repack(int slots) { return slots == 2 ? REPACK_ATOMIC : slots == 1 ? REPACK_KERNEL : REPACK_NONE; }

int gem_lbfgs_debug_begin(gem_handle* h, int B, const float* d_x0, int slots, void* stream) {
    if (!h) { set_error("gem_lbfgs_debug_begin: null handle"); return 1; }
    Workspace& w = h->ws;
    if (B < 1 || B > w.Bmax) { set_error("gem_lbfgs_debug_begin: B exceeds max_windows (or is < 1)"); return 1; }
    if (!d_x0 || slots < 0 || slots > 2) { set_error("gem_lbfgs_debug_begin: null x0 or slots not 0, 1 or 2"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    w.dbg_slots = -1;
    if (launch_pad_latent(d_x0, w.trial, B, h->D, h->Dp, s)) return 1;
    if (h->precision == GEM_PRECISION_BF16 && launch_f32_to_bf16(w.trial, w.trial_b, (size_t)B * h->Dp, s)) return 1;
    if (launch_lbfgs_init(h, B, s)) return 1;
    if (begin_rounds(h, B, slots == 2 ? DBG_MAX_ROUNDS + 1 : 0, s, &w.dbg_log0)) return 1;
    w.dbg_slots = slots; w.dbg_B = B; w.dbg_round = 0;
    return 0;
}

int gem_lbfgs_debug_advance(gem_handle* h, int B, const gem_lbfgs_opts* opt, const double* d_f, const float* d_g, int n_slabs,
                            void* stream) {
    if (!h) { set_error("gem_lbfgs_debug_advance: null handle"); return 1; }
    Workspace& w = h->ws;
    if (B < 1 || B > w.Bmax) { set_error("gem_lbfgs_debug_advance: B exceeds max_windows (or is < 1)"); return 1; }
    if (w.dbg_slots < 0 || B != w.dbg_B) { set_error("gem_lbfgs_debug_advance: no gem_lbfgs_debug_begin with this B came before"); return 1; }
    if (!opt || !d_f || !d_g) { set_error("gem_lbfgs_debug_advance: null argument"); return 1; }
    if (check_lbfgs_opts(w, *opt, "gem_lbfgs_debug_advance")) return 1;
    const size_t slab = (size_t)B * h->Dp;
    if (n_slabs < 0 || (size_t)n_slabs * slab > w.splitk_elems) {
        set_error("gem_lbfgs_debug_advance: n_slabs must be 0.." + std::to_string(w.splitk_elems / slab) + " (the split-K scratch)"); return 1;
    }
    if (w.dbg_round >= DBG_MAX_ROUNDS) { set_error("gem_lbfgs_debug_advance: more rounds than any max_eval allows"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    GEM_HIP(hipMemcpyAsync(w.f, d_f, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
    float* rows = n_slabs ? w.splitk : w.dz;
    for (int z = 0; z < (n_slabs ? n_slabs : 1); ++z)
        if (launch_pad_latent(d_g + (size_t)z * B * h->D, rows + z * slab, B, h->D, h->Dp, s)) return 1;
    const int k = w.dbg_round;
    const Repack mode = dbg_repack(w.dbg_slots);
    RoundSet rs = round_set(w, w.dbg_log0, k, mode);      // slot table, slot hand-out and slabs are what the rounds of a stage use
    rs.trace = nullptr;
    SlabSrc grad;
    if (n_slabs) { grad.base = w.splitk; grad.nslab = n_slabs; grad.stride = slab; }
    int rc = launch_lbfgs_advance(h, B, *opt, rs, grad, s);
    // slot mode 1: the compaction between this round and the next (a stage runs it at the head of the next round)
    if (!rc && mode == REPACK_KERNEL) {
        const RoundSet next = round_set(w, w.dbg_log0, k + 1, mode);
        rc = launch_compact(h, next, B, 0, s);
        w.log_pos = next.log_idx + 1;
    }
    if (rc) { w.dbg_slots = -1; return 1; }
    w.dbg_round = k + 1;
    return 0;
}

int gem_lbfgs_debug_read(gem_handle* h, int B, gem_lbfgs_debug_state* d_state, float* d_x, float* d_d, float* d_trial,
                         int32_t* d_slot_of, int32_t* d_count, void* stream) {
    if (!h) { set_error("gem_lbfgs_debug_read: null handle"); return 1; }
    Workspace& w = h->ws;
    if (B < 1 || B > w.Bmax) { set_error("gem_lbfgs_debug_read: B exceeds max_windows (or is < 1)"); return 1; }
    if (w.dbg_slots < 0 || B != w.dbg_B) { set_error("gem_lbfgs_debug_read: no gem_lbfgs_debug_begin with this B came before"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (launch_lbfgs_debug_read(h, B, d_state, d_x, d_d, d_trial, s)) return 1;
    // the set the NEXT round reads: slot mode 0 never touches the identity table of the begin call, mode 1 compacts in place, mode 2 alternates
    const RoundSet rs = round_set(w, w.dbg_log0, w.dbg_round, w.dbg_slots == 2 ? REPACK_ATOMIC : REPACK_KERNEL);
    if (d_slot_of) GEM_HIP(hipMemcpyAsync(d_slot_of, rs.slot_of, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (d_count) GEM_HIP(hipMemcpyAsync(d_count, rs.n_active, sizeof(int), hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---- for parity tests: one layer through launch_gemm / gemm_bf16a (include/gem_hip.h) ------------------------------------------
int gem_gemm_debug_layer_create(gem_handle* h, int taps, int N, int K, const float* h_w, const float* h_bias,
                                gem_gemm_debug_layer** out) {
    if (!h || !h_w || !h_bias || !out) { set_error("gem_gemm_debug_layer_create: null argument"); return 1; }
    if ((taps != 1 && taps != 3) || N < 64 || K < 32 || N % 64 != 0 || K % 32 != 0 || (size_t)taps * N * K > ((size_t)1 << 28)) {
        set_error("gem_gemm_debug_layer_create: need taps 1 or 3, N % 64 == 0, K % 32 == 0, taps * N * K <= 2^28"); return 1;
    }
    GEM_HIP(hipSetDevice(h->cfg.device));
    std::unique_ptr<gem_gemm_debug_layer> l(new gem_gemm_debug_layer());
    if (make_layer_images(l->allocs, &l->L, taps, N, K, h_w, h_bias)) { free_all(l->allocs); return 1; }
    h->dbg_layers.push_back(l.get());
    *out = l.release();
    return 0;
}

int gem_gemm_debug_layer_destroy(gem_handle* h, gem_gemm_debug_layer* layer) {
    if (!h) { set_error("gem_gemm_debug_layer_destroy: null handle"); return 1; }
    auto it = std::find(h->dbg_layers.begin(), h->dbg_layers.end(), layer);
    if (!layer || it == h->dbg_layers.end()) { set_error("gem_gemm_debug_layer_destroy: not a layer of this handle"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    GEM_HIP(hipDeviceSynchronize());
    h->dbg_layers.erase(it);
    free_all(layer->allocs);
    delete layer;
    return 0;
}

int gem_gemm_debug_run(gem_handle* h, const gem_gemm_debug_layer* layer, const gem_gemm_debug_args* a, char* names, int names_len,
                       int32_t* info, void* stream) {
    const char* me = "gem_gemm_debug_run: ";
    auto bad = [&](const char* what) { set_error(std::string(me) + what); return 1; };
    if (!h || !layer || !a) return bad("null argument");
    if (std::find(h->dbg_layers.begin(), h->dbg_layers.end(), layer) == h->dbg_layers.end()) return bad("not a layer of this handle");
    if ((names && names_len < 1) || (!names && names_len != 0)) return bad("names buffer without a length (or the reverse)");
    const Layer& L = layer->L;
    Workspace& w = h->ws;
    const bool b16a = a->route == 1;
    if (a->route != 0 && a->route != 1) return bad("route must be 0 (launch_gemm) or 1 (gemm_bf16a)");
    if (a->epi < 0 || a->epi > 3) return bad("epi must be 0 .. 3");
    if (a->epi == EPI_MASK && (L.taps != 3 || !a->d_aux)) return bad("the mask epilogue belongs to conv layers and needs d_aux");
    if (a->family < -1 || a->family > 3) return bad("family must be -1 .. 3");
    if (!a->d_A || !a->d_C) return bad("null d_A or d_C");
    if (a->M < 1 || (long)a->M > (long)w.Bmax * h->T) return bad("M must be 1 .. max_windows * seq_len");
    if (a->T < 1 || (L.taps == 3 && a->M % a->T != 0)) return bad("need T >= 1, and M % T == 0 for conv layers");
    if (L.taps == 3 && b16a && a->T != h->T) return bad("gemm_bf16a reads the handle's seq_len: T must equal it");
    if (b16a && L.K % 64 != 0) return bad("the bf16 kernels need K % 64 == 0");
    if (!b16a && h->precision != GEM_PRECISION_F32 && L.K % 64 != 0) return bad("the bf16 kernels need K % 64 == 0");
    if (a->d_row_map && L.taps != 1) return bad("a row map gathers the rows of linear layers only");
    if (a->a_rows < 1 || (!a->d_row_map && a->a_rows < a->M)) return bad("a_rows must cover M (or the row map's targets)");
    if (!b16a && (a->out_bf16 || a->allow_split)) return bad("out_bf16 and allow_split belong to gemm_bf16a");
    if (b16a && a->defer && !a->allow_split) return bad("gemm_bf16a leaves slabs only where it may split");
    if ((a->defer || a->allow_split) && (!w.splitk || (size_t)a->M * L.N > w.splitk_elems)) return bad("one slab of M x N does not fit the split-K scratch");
    GEM_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    GEM_HIP(hipStreamSynchronize(s));
    if (a->d_row_map) {
        std::vector<int> map((size_t)a->M);
        GEM_HIP(hipMemcpy(map.data(), a->d_row_map, map.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int r : map) if (r < 0 || r >= a->a_rows) return bad("row map entry outside d_A");
    }
    const int T = L.taps == 3 ? a->T : 1;
    if (a->d_rows) {
        int m[2];
        GEM_HIP(hipMemcpy(m, a->d_rows, sizeof(m), hipMemcpyDeviceToHost));
        if (m[0] < 1 || (long)m[0] * T > a->M || m[1] != m[0] * a->T) return bad("d_rows must hold {m, m * T} with 1 <= m and m (* T for convs) <= M");
    }
    RoundSet rs;
    rs.n_active = const_cast<int*>(a->d_rows);
    SlabSrc slab;
    const GemmOpts o(a->d_rows ? &rs : nullptr, a->d_row_map, a->defer ? &slab : nullptr);
    std::set<std::string> seen;
    std::vector<void*> tmp;
    h->prof.capture = &seen;
    int rc;
    if (b16a) {
        uint16_t *A16 = nullptr, *aux16 = nullptr;
        const size_t na = (size_t)a->a_rows * L.K, nx = (size_t)a->M * L.N;
        rc = dev_alloc(tmp, &A16, na) || launch_f32_to_bf16(a->d_A, A16, na, s);
        if (!rc && a->d_aux) rc = dev_alloc(tmp, &aux16, nx) || launch_f32_to_bf16(a->d_aux, aux16, nx, s);
        if (!rc) rc = gemm_bf16a(h, L, a->epi, A16, L.K, aux16, a->d_C, a->out_bf16 != 0, L.N, a->M, s, a->family, a->allow_split != 0, o);
    } else {
        rc = launch_gemm(h, L, a->epi, a->d_A, L.K, a->d_aux, static_cast<float*>(a->d_C), L.N, a->M, T, s, a->family, o);
    }
    h->prof.capture = nullptr;
    h->prof.pending.clear();
    const bool deferred = !rc && slab.base != nullptr;
    if (deferred)          // the consumer's part: sum the slabs, apply the epilogue
        rc = launch_splitk_reduce(h, a->epi, slab.nslab, slab.stride, L.bias, a->d_aux, static_cast<float*>(a->d_C), a->M, L.N, L.N,
                                  slab.m_dev, s, slab.dyn_W, slab.n_tiles);
    const bool synced = hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize");
    free_all(tmp);
    if (rc || !synced) return 1;
    if (names) {
        std::string out;
        for (const auto& n : seen) { if (!out.empty()) out += "; "; out += n; }
        snprintf(names, (size_t)names_len, "%s", out.c_str());
    }
    if (info) { info[0] = deferred ? slab.nslab : 0; info[1] = deferred ? slab.dyn_W : 0; info[2] = (b16a && a->out_bf16 && !deferred) ? 1 : 0; info[3] = 0; }
    return 0;
}

}  // extern "C"
