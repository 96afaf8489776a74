// C-ABI entry points of libgem_hip.so (see include/gem_hip.h) that are not an optimisation call: error and profiling plumbing,
// gem_create / gem_destroy, the setters and the sequence post-processing calls.  The weights are loaded in weights.hip, the
// optimisation calls are sequenced in stage.hip.  Host code only.
#include <cxxabi.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "gem_internal.h"

namespace gem {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

const char* dev_env(const char* name) {
    const char* on = getenv("GEM_DEV");
    if (!on || on[0] != '1') return nullptr;
    return getenv(name);
}

void note_kernel(gem_handle* h, const void* host_fn) {
    if (!h->prof.on && !h->prof.capture) return;
    const char* m = hipKernelNameRefByPtr(host_fn, nullptr);
    if (!m) return;
    int st = 0;
    char* d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
    std::string n = (st == 0 && d) ? d : m;
    free(d);
    if (n.rfind("void ", 0) == 0) n = n.substr(5);
    // drop the parameter list: everything from the '(' that closes the template-argument list
    int depth = 0;
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0) { n.resize(i); break; }
    }
    h->prof.pending.insert(n);
}

// Every captured call bakes weight and workspace pointers into its kernel arguments: whatever re-allocates them drops the cache.
void drop_graphs(gem_handle* h) {
    for (auto& g : h->graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
    h->graphs.clear();
}

int post_scratch(gem_handle* h, size_t elems) {
    if (elems <= h->post_work_elems) return 0;
    GEM_HIP(hipDeviceSynchronize());                 // a previous call may still be reading the old buffer
    if (h->post_work) GEM_HIP(hipFree(h->post_work));
    h->post_work = nullptr; h->post_work_elems = 0;
    GEM_HIP(hipMalloc((void**)&h->post_work, elems * sizeof(double)));
    h->post_work_elems = elems;
    return 0;
}

}  // namespace gem

using namespace gem;

extern "C" {

const char* gem_last_error(void) { return g_error.c_str(); }
int gem_version(void) { return 1; }

int gem_create(const gem_config* cfg, gem_handle** out) {
    if (!cfg || !out) { set_error("gem_create: null argument"); return 1; }
    if (cfg->seq_len < 3 || cfg->seq_len > 16 || cfg->n_joints < 1 || cfg->n_joints > GEM_MAX_JOINTS) {
        set_error("gem_create: seq_len must be 3..16 and n_joints 1..16"); return 1;
    }
    if (cfg->n_joints * 3 > PAD) { set_error("gem_create: n_joints*3 must be <= 64"); return 1; }
    if (cfg->n_hidden < 1 || cfg->n_hidden > GEM_MAX_HIDDEN || cfg->latent_dim < 1 || cfg->latent_dim > 4096) {
        set_error("gem_create: n_hidden must be 1..8 and latent_dim 1..4096"); return 1;
    }
    if (cfg->n_poly < 1 || cfg->n_poly > GEM_MAX_POLY || cfg->max_windows < 1) { set_error("gem_create: bad n_poly / max_windows"); return 1; }
    GEM_HIP(hipSetDevice(cfg->device));
    std::unique_ptr<gem_handle, void (*)(gem_handle*)> h(new gem_handle(), gem_destroy);     // frees the device memory on any early return
    h->cfg = *cfg;
    h->T = cfg->seq_len; h->J = cfg->n_joints; h->C = cfg->n_joints * 3; h->Cp = pad64(h->C);
    h->D = cfg->latent_dim; h->Dp = pad64(cfg->latent_dim);
    h->top = cfg->hidden[cfg->n_hidden - 1]; h->topp = pad64(h->top);
    GEM_HIP(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    Workspace& w = h->ws;
    const int B = cfg->max_windows, T = h->T;
    const size_t rows = (size_t)B * T;
    w.Bmax = B;
    if (dev_alloc(w.allocs, &w.pose_p, rows * PAD)) return 1;
    w.enc_act.resize(cfg->n_hidden);
    for (int i = 0; i < cfg->n_hidden; ++i)
        if (dev_alloc(w.allocs, &w.enc_act[i], rows * pad64(cfg->hidden[i]))) return 1;
    if (dev_alloc(w.allocs, &w.mulv, (size_t)B * 2 * h->Dp)) return 1;
    if (dev_alloc(w.allocs, &w.h0, rows * h->topp)) return 1;
    // decoder conv widths: reversed hidden, then hidden[0] again, then C
    std::vector<int> outs;
    for (int i = cfg->n_hidden - 2; i >= 0; --i) outs.push_back(cfg->hidden[i]);
    outs.push_back(cfg->hidden[0]);
    outs.push_back(h->C);
    w.dec_act.resize(outs.size());
    w.dec_grad.resize(outs.size());
    int cin = h->top;
    for (size_t i = 0; i < outs.size(); ++i) {
        if (dev_alloc(w.allocs, &w.dec_act[i], rows * pad64(outs[i]))) return 1;
        if (dev_alloc(w.allocs, &w.dec_grad[i], rows * pad64(cin))) return 1;
        cin = outs[i];
    }
    if (dev_alloc(w.allocs, &w.dXp, rows * PAD)) return 1;
    // bf16 twins (gemm_bf16a.h / decoder_bf16.hip)
    w.dec_act_b.assign(outs.size(), nullptr);
    w.dec_grad_b.assign(outs.size(), nullptr);
    {
        int ci = h->top;
        for (size_t i = 0; i < outs.size(); ++i) {
            if (i + 1 < outs.size() && dev_alloc(w.allocs, &w.dec_act_b[i], rows * pad64(outs[i]))) return 1;
            if (dev_alloc(w.allocs, &w.dec_grad_b[i], rows * pad64(ci))) return 1;
            ci = outs[i];
        }
    }
    if (dev_alloc(w.allocs, &w.trial_b, (size_t)B * h->Dp) || dev_alloc(w.allocs, &w.h0_b, rows * h->topp) ||
        dev_alloc(w.allocs, &w.dXp_b, rows * PAD) || dev_alloc(w.allocs, &w.zero16, (size_t)128)) return 1;
    if (dev_alloc(w.allocs, &w.dz, (size_t)B * h->Dp)) return 1;
    float** vecs[] = {&w.x, &w.d, &w.g, &w.gp, &w.bg0, &w.bg1, &w.trial};
    for (float** v : vecs)
        if (dev_alloc(w.allocs, v, (size_t)B * h->Dp)) return 1;
    w.hist_cap = 32;     // >= max_iter - 1 pairs for the reference's max_iter = 25 (checked per call); a power of two:
                         // lbfgs.hip wraps ring indices with a mask
    static_assert(MAX_HIST >= 32, "ring capacity");
    if (dev_env("GEM_LBFGS_CLK")) {
        if (dev_alloc(w.allocs, &w.lbfgs_clk, (size_t)32)) return 1;
        GEM_HIP(hipMemset(w.lbfgs_clk, 0, 32 * sizeof(unsigned long long)));
    }
    if (dev_alloc(w.allocs, &w.S, (size_t)B * w.hist_cap * h->Dp)) return 1;
    if (dev_alloc(w.allocs, &w.Y, (size_t)B * w.hist_cap * h->Dp)) return 1;
    if (dev_alloc(w.allocs, &w.state, (size_t)B) || dev_alloc(w.allocs, &w.phase, (size_t)B)) return 1;
    if (dev_alloc(w.allocs, &w.f, (size_t)B)) return 1;
    if (dev_alloc(w.allocs, &w.parts, (size_t)B * 5)) return 1;
    if (dev_alloc(w.allocs, &w.trace, (size_t)TRACE_ROUNDS * B)) return 1;
    if ((size_t)cfg->heat_h * cfg->heat_w <= 32768) {        // (the texel-block key packs two texel indices into 32 bits)
        if (dev_alloc(w.allocs, &w.tex_key, rows * h->J) || dev_alloc(w.allocs, &w.tex_val, rows * h->J * 4)) return 1;
    }
    if (dev_alloc(w.allocs, &w.pose_a, rows * h->C)) return 1;
    if (dev_alloc(w.allocs, &w.pose_b, rows * h->C)) return 1;
    if (dev_alloc(w.allocs, &w.n_log, (size_t)N_LOG)) return 1;
    if (dev_alloc(w.allocs, &w.perm2, (size_t)B) || dev_alloc(w.allocs, &w.slot_of2, (size_t)B)) return 1;
    if (dev_alloc(w.allocs, &w.perm, (size_t)B) || dev_alloc(w.allocs, &w.slot_of, (size_t)B) || dev_alloc(w.allocs, &w.n_active, 2))
        return 1;
    // split-K slabs: only launches with few output tiles cut K; 64 MB, more when mid-size batches need it for the
    // decoder_input backward product (rows x Dp x up to 4 slices)
    w.splitk_elems = std::max((size_t)16 << 20, (size_t)std::min(B, 4096) * h->Dp * 4);
    if (dev_alloc(w.allocs, &w.splitk, w.splitk_elems)) return 1;
    std::vector<int> parents(cfg->parents, cfg->parents + cfg->n_joints);
    std::vector<int> children((size_t)GEM_MAX_JOINTS * GEM_MAX_JOINTS, -1);
    for (int j = 0; j < cfg->n_joints; ++j) {
        if (parents[j] < 0 || parents[j] >= cfg->n_joints) { set_error("gem_create: bad parent index"); return 1; }
        int n = 0;
        for (int c = 0; c < cfg->n_joints; ++c)
            if (c != j && parents[c] == j) children[(size_t)j * GEM_MAX_JOINTS + n++] = c;
    }
    if (upload(w.allocs, &h->d_parents, parents) || upload(w.allocs, &h->d_children, children)) return 1;
    *out = h.release();
    return 0;
}

void gem_destroy(gem_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    for (auto& r : h->prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    if (h->ws.lbfgs_clk) {
        unsigned long long c[32];
        if (hipMemcpy(c, h->ws.lbfgs_clk, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess && c[31]) {
            fprintf(stderr, "[GEM_LBFGS_CLK] %llu window-rounds with a new direction from the ring, mean pairs %.1f; us per phase:", c[31], (double)c[30] / c[31]);
            double tot = 0;
            for (int i = 1; i < 10; ++i) { fprintf(stderr, " %d:%.2f", i, c[i] / 100.0 / c[31]); tot += c[i] / 100.0 / c[31]; }
            fprintf(stderr, " total %.2f\n", tot);
        }
    }
    drop_graphs(h);
    for (gem_gemm_debug_layer* l : h->dbg_layers) { free_all(l->allocs); delete l; }
    free_all(h->net[0].allocs);
    free_all(h->net[1].allocs);
    free_all(h->ws.allocs);
    if (h->post_work) (void)hipFree(h->post_work);
    delete h;
}

int gem_mean_bone_length(gem_handle* h, const float* d_pose, int n_frames, float* d_out, void* stream) {
    if (!h || !d_pose || !d_out || n_frames < 1) { set_error("gem_mean_bone_length: bad argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    return launch_mean_bone(h, d_pose, n_frames, d_out, (hipStream_t)stream);
}

int gem_set_texel_cache(gem_handle* h, int on) {
    if (!h) { set_error("gem_set_texel_cache: null handle"); return 1; }
    h->tex_cache = on != 0;
    return 0;
}

int gem_graph_enable(gem_handle* h, int on) {
    if (!h) { set_error("gem_graph_enable: null handle"); return 1; }
    if (!on && !h->graphs.empty()) {
        // switching replay off drops the captured calls: they hold the ADDRESSES of the caller's tensors, and a caller about to free
        // those tensors must be able to make sure no graph is ever replayed on whatever is allocated there next (bench.py's shards)
        GEM_HIP(hipSetDevice(h->cfg.device));
        GEM_HIP(hipDeviceSynchronize());
        drop_graphs(h);
    }
    h->graphs_on = on != 0;
    return 0;
}

int gem_graph_stats(gem_handle* h, int64_t* n_captures, int64_t* n_replays) {
    if (!h) { set_error("gem_graph_stats: null handle"); return 1; }
    if (n_captures) *n_captures = h->graph_captures;
    if (n_replays) *n_replays = h->graph_replays;
    return 0;
}

// accepted for compatibility: every call runs as one lane (include/gem_hip.h)
int gem_set_lanes(gem_handle* h, int min_windows) {
    if (!h || min_windows < 0) { set_error("gem_set_lanes: min_windows must be >= 0"); return 1; }
    return 0;
}

int gem_set_precision(gem_handle* h, int mode) {
    if (!h || mode < 0 || mode > 2) { set_error("gem_set_precision: mode must be 0 (f32), 1 (bf16x3) or 2 (bf16)"); return 1; }
    h->precision = mode;
    return 0;
}

int gem_merge_windows(gem_handle* h, const double* d_windows, int n_chunks, int windows_per_chunk, int overlap, int smooth,
                      double* d_out, void* stream) {
    if (!h) { set_error("gem_merge_windows: null handle"); return 1; }
    if (n_chunks < 0 || windows_per_chunk < 1 || overlap < 0 || 2 * overlap > h->T) {
        set_error("gem_merge_windows: need windows_per_chunk >= 1 and 0 <= 2*overlap <= seq_len"); return 1;
    }
    if (n_chunks == 0) return 0;
    if (!d_windows || !d_out) { set_error("gem_merge_windows: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    const int fpc = windows_per_chunk * (h->T - overlap) + overlap;
    const size_t n = (size_t)n_chunks * fpc * h->C;
    if (smooth && post_scratch(h, n)) return 1;
    return launch_merge(d_windows, h->post_work, d_out, n_chunks, windows_per_chunk, h->T, h->C, overlap, smooth, (hipStream_t)stream);
}

int gem_calculate_errors(gem_handle* h, const double* d_est, const double* d_mid, const double* d_opt, const double* d_gt,
                         int n_frames, const double* h_bone_mm, double* d_out, void* stream) {
    if (!h) { set_error("gem_calculate_errors: null handle"); return 1; }
    if (h->J < 12) { set_error("gem_calculate_errors: the hip-midpoint error needs joints 7 and 11 (n_joints >= 12)"); return 1; }
    if (n_frames < 1) { set_error("gem_calculate_errors: n_frames must be >= 1"); return 1; }
    if (!d_est || !d_mid || !d_opt || !d_gt || !h_bone_mm || !d_out) { set_error("gem_calculate_errors: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    if (post_scratch(h, (size_t)(11 + MAXJ_ERR) * n_frames)) return 1;
    return launch_errors(h, d_est, d_mid, d_opt, d_gt, n_frames, h_bone_mm, h->post_work, d_out, (hipStream_t)stream, 1);
}

int gem_calculate_errors_chunks(gem_handle* h, const double* d_est, const double* d_mid, const double* d_opt, const double* d_gt,
                                int n_chunks, int frames_per_chunk, const double* h_bone_mm, double* d_out, void* stream) {
    if (!h) { set_error("gem_calculate_errors_chunks: null handle"); return 1; }
    if (h->J < 12) { set_error("gem_calculate_errors_chunks: the hip-midpoint error needs joints 7 and 11 (n_joints >= 12)"); return 1; }
    if (n_chunks < 0 || frames_per_chunk < 1) { set_error("gem_calculate_errors_chunks: need n_chunks >= 0 and frames_per_chunk >= 1"); return 1; }
    if (n_chunks == 0) return 0;
    if (!d_est || !d_mid || !d_opt || !d_gt || !h_bone_mm || !d_out) { set_error("gem_calculate_errors_chunks: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    const size_t per = (size_t)(11 + MAXJ_ERR) * frames_per_chunk;
    if (post_scratch(h, per * n_chunks)) return 1;           // (every sequence its own scratch: blockIdx.y picks the sequence)
    if (n_chunks > 65535) { set_error("gem_calculate_errors_chunks: at most 65535 sequences per call"); return 1; }
    return launch_errors(h, d_est, d_mid, d_opt, d_gt, frames_per_chunk, h_bone_mm, h->post_work, d_out, (hipStream_t)stream, n_chunks);
}

int gem_lift_skeleton(gem_handle* h, const float* d_heat, const double* d_depth, int n_frames, const double* h_poly_c2w,
                      int n_poly_c2w, int upscale, int pad_x, int pad_y, double* d_out64, float* d_out32, void* stream) {
    if (!h) { set_error("gem_lift_skeleton: null handle"); return 1; }
    if (n_frames < 0 || n_poly_c2w < 1 || n_poly_c2w > GEM_MAX_POLY || upscale < 1 || pad_x < 0 || pad_y < 0) {
        set_error("gem_lift_skeleton: need n_frames >= 0, 1 <= n_poly_c2w <= 16, upscale >= 1, pads >= 0"); return 1;
    }
    if (n_frames == 0) return 0;
    if (!d_heat || !d_depth || !h_poly_c2w || (!d_out64 && !d_out32)) { set_error("gem_lift_skeleton: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    return launch_lift(h, d_heat, d_depth, n_frames, h_poly_c2w, n_poly_c2w, upscale, pad_x, pad_y, d_out64, d_out32,
                       (hipStream_t)stream);
}

int gem_profile_enable(gem_handle* h, int on) {
    if (!h) { set_error("gem_profile_enable: null handle"); return 1; }
    h->prof.on = on != 0;
    return 0;
}

int gem_profile_kernels(gem_handle* h, int family, char* buf, int buf_len) {
    if (!h || family < 0 || family > 3 || !buf || buf_len < 1) { set_error("gem_profile_kernels: bad argument"); return 1; }
    std::string out;
    for (const auto& n : h->prof.names[family]) {
        if (!out.empty()) out += "; ";
        out += n;
    }
    h->prof.names[family].clear();
    snprintf(buf, (size_t)buf_len, "%s", out.c_str());
    return 0;
}

int gem_profile_read(gem_handle* h, int family, double* total_ms, int64_t* n_launches, double* flops) {
    if (!h || family < 0 || family > 3) { set_error("gem_profile_read: bad argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    Profile& p = h->prof;
    // fold finished event pairs into the totals (caller has synchronised the stream)
    std::vector<int> nlog;
    for (auto& r : p.recs) {
        float ms = 0.f;
        GEM_HIP(hipEventSynchronize(r.b));
        GEM_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.log_idx >= 0) {          // compacted round: FLOPs of the rows that were actually active
            if (nlog.empty()) {
                nlog.resize(N_LOG);
                GEM_HIP(hipMemcpy(nlog.data(), h->ws.n_log, (size_t)N_LOG * sizeof(int), hipMemcpyDeviceToHost));
            }
            if (h->ws.log_pos - r.log_idx <= N_LOG) r.flops = r.flops_per_window * nlog[r.log_idx % N_LOG];
        }
        static const char* dump = dev_env("GEM_PROFILE_DUMP");          // developer aid: one line per timed launch
        if (dump) {
            if (FILE* f = fopen(dump, "a")) {
                fprintf(f, "%d %d %.3f\n", r.family, r.log_idx >= 0 && !nlog.empty() ? nlog[r.log_idx % N_LOG] : -1, ms * 1e3);
                fclose(f);
            }
        }
        p.total_ms[r.family] += ms;
        p.n[r.family] += 1;
        p.flops[r.family] += r.flops;
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    p.recs.clear();
    if (total_ms) *total_ms = p.total_ms[family];
    if (n_launches) *n_launches = p.n[family];
    if (flops) *flops = p.flops[family];
    p.total_ms[family] = 0; p.n[family] = 0; p.flops[family] = 0;
    return 0;
}

}  // extern "C"

#include "slam_bridge.h"          // gem_slam_bridge_work, gem_slam_bridge
