// Loading a motion VAE (gem_load_vae): BatchNorm folded into the convolutions, every layer padded and packed the way its kernels read
// it (fp32, bf16 hi / lo images, the fused tails' layouts), decoder_input o conv 0 composed into one linear layer.  Host code and one
// load-time kernel; nothing here runs during an optimisation call.
#include <cmath>
#include <cstring>

#include "gem_internal.h"

namespace gem {

static uint16_t host_f2bf(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static float host_bf2f(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// bf16 hi / lo images of a packed fp32 weight array (same [taps][N][K] layout)
static int upload_bf16(std::vector<void*>& owner, Layer* L, const std::vector<float>& w) {
    std::vector<uint16_t> hi(w.size()), lo(w.size());
    for (size_t i = 0; i < w.size(); ++i) {
        hi[i] = host_f2bf(w[i]);
        lo[i] = host_f2bf(w[i] - host_bf2f(hi[i]));
    }
    return upload(owner, &L->wb_hi, hi) || upload(owner, &L->wb_lo, lo);
}

int make_layer_images(std::vector<void*>& owner, Layer* L, int taps, int N, int K, const float* w, const float* bias) {
    const std::vector<float> wv(w, w + (size_t)taps * N * K), bv(bias, bias + N);
    L->taps = taps; L->N = N; L->K = K;
    return upload(owner, &L->w, wv) || upload(owner, &L->bias, bv) || upload_bf16(owner, L, wv);
}

// taps[k][ci][co] in double, BatchNorm folded
struct FoldedConv {
    int ci, co;
    std::vector<double> taps, bias;
};

static FoldedConv fold_conv(const float* w, const float* b, const float* const* bnp /* 4 blobs or null */, int ci, int co, bool transposed) {
    FoldedConv f;
    f.ci = ci; f.co = co;
    f.taps.assign((size_t)3 * ci * co, 0.0);
    f.bias.assign(co, 0.0);
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < ci; ++i)
            for (int o = 0; o < co; ++o) {
                // Conv1d weight [co][ci][3]: out[t] = sum_k in[t+k-1] w[:, :, k]
                // ConvTranspose1d (s=1,p=1) weight [ci][co][3]: out[t] = sum_k in[t+1-k] w[:, :, k]  -> tap k' = 2-k
                const double v = transposed ? (double)w[((size_t)i * co + o) * 3 + (2 - k)] : (double)w[((size_t)o * ci + i) * 3 + k];
                f.taps[((size_t)k * ci + i) * co + o] = v;
            }
    for (int o = 0; o < co; ++o) f.bias[o] = b[o];
    if (bnp) {
        const float *gamma = bnp[0], *beta = bnp[1], *mean = bnp[2], *var = bnp[3];
        for (int o = 0; o < co; ++o) {
            const double s = (double)gamma[o] / std::sqrt((double)var[o] + BN_EPS);
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < ci; ++i) f.taps[((size_t)k * ci + i) * co + o] *= s;
            f.bias[o] = (f.bias[o] - (double)mean[o]) * s + (double)beta[o];
        }
    }
    return f;
}

static int make_conv_layers(StageNet& net, const FoldedConv& f, Layer* fwd, Layer* bwd, std::vector<float>* keep_fwd = nullptr,
                            std::vector<float>* keep_bwd = nullptr) {
    const int Kp = pad64(f.ci), Np = pad64(f.co);
    std::vector<float> wf((size_t)3 * Np * Kp, 0.f), bf(Np, 0.f);
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < f.ci; ++i)
            for (int o = 0; o < f.co; ++o) wf[((size_t)k * Np + o) * Kp + i] = (float)f.taps[((size_t)k * f.ci + i) * f.co + o];
    for (int o = 0; o < f.co; ++o) bf[o] = (float)f.bias[o];
    fwd->taps = 3; fwd->K = Kp; fwd->N = Np;
    if (upload(net.allocs, &fwd->w, wf) || upload(net.allocs, &fwd->bias, bf) || upload_bf16(net.allocs, fwd, wf)) return 1;
    auto to_w4 = [](const std::vector<float>& w, int N, int K) {      // [tap][N][K] -> [tap][K/4][N][4]
        std::vector<float> o(w.size());
        for (int t = 0; t < 3; ++t)
            for (int n = 0; n < N; ++n)
                for (int k = 0; k < K; ++k) o[(((size_t)t * (K / 4) + k / 4) * N + n) * 4 + (k & 3)] = w[((size_t)t * N + n) * K + k];
        return o;
    };
    if (bwd && upload(net.allocs, &fwd->w4, to_w4(wf, Np, Kp))) return 1;
    if (bwd) {
        // adjoint: dIn[r] = sum_tap' dOut[r + tap' - 1] . taps[2-tap']^T   ->  W[tap'][n=ci][k=co]
        std::vector<float> wb((size_t)3 * Kp * Np, 0.f);
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < f.ci; ++i)
                for (int o = 0; o < f.co; ++o) wb[((size_t)k * Kp + i) * Np + o] = (float)f.taps[((size_t)(2 - k) * f.ci + i) * f.co + o];
        bwd->taps = 3; bwd->K = Np; bwd->N = Kp;
        if (upload(net.allocs, &bwd->w, wb) || upload(net.allocs, &bwd->w4, to_w4(wb, Kp, Np)) || upload_bf16(net.allocs, bwd, wb))
            return 1;
        bwd->bias = nullptr;
        if (keep_bwd) *keep_bwd = std::move(wb);
    }
    if (keep_fwd) *keep_fwd = std::move(wf);
    return 0;
}

// ---- decoder_input o conv 0 as ONE linear layer -----------------------------------------------------------------------------
// h0 = Wd z + bd (decoder_input, rows (t', ci)) feeds ConvTranspose1d 0 + BatchNorm with NO activation in between
// (SeqConvVAE.py:62, 67-75, 131-135), so
//     pre0[(t, co)] = sum_tap sum_ci taps[tap][ci][co] h0[(t + tap - 1, ci)] + bc[co]      (frames outside the window: zero)
//                   = (Wf z + bf)[(t, co)],   Wf[(t, co)][k] = sum_tap sum_ci taps[tap][ci][co] Wd[(t + tap - 1, ci)][k].
// Wf is [T*C1p, Dp]: 2 x 2048 x 2560 FLOP per window instead of 2 x 2048 x 5120 + 2 x 3 x 512 x 256 x 10 (a third of the
// matrix work of the two layers, half their weight bytes), one launch instead of two (three in the backward direction, where
// its transpose replaces the conv adjoint, the split-K reduce behind it and the decoder_input backward product).  Built once
// per gem_load_vae in fp64 from the fp64 folded conv taps and the fp32 decoder_input weights, rounded to fp32 once.
__global__ __launch_bounds__(256) void compose_front_kernel(const double* __restrict__ taps /* [3][ci][co] */, const float* __restrict__ Wd /* [T*Cip][Dp] */,
                                                            int T, int Ci, int Cip, int Co, int Cop, int Dp, float* __restrict__ Wf /* [T*Cop][Dp] */,
                                                            float* __restrict__ WfT /* [Dp][T*Cop] */) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y, t = n / Cop, co = n - t * Cop;
    if (k >= Dp) return;
    double acc = 0.0;
    if (co < Co) {
        for (int tap = 0; tap < 3; ++tap) {
            const int ts = t + tap - 1;
            if (ts < 0 || ts >= T) continue;
            const double* tp = taps + (size_t)tap * Ci * Co + co;
            const float* wd = Wd + (size_t)ts * Cip * Dp + k;
            for (int ci = 0; ci < Ci; ++ci) acc += tp[(size_t)ci * Co] * (double)wd[(size_t)ci * Dp];
        }
    }
    Wf[(size_t)n * Dp + k] = (float)acc;
    WfT[(size_t)k * ((size_t)T * Cop) + n] = (float)acc;
}

static int compose_front(gem_handle* h, StageNet& net, const FoldedConv& f, const float* dec_in_bias_host /* time-major, padded */) {
    const int T = h->T, Dp = h->Dp, Cip = h->topp, Cop = pad64(f.co), Nf = T * Cop;
    double* d_taps = nullptr;
    std::vector<void*> tmp;
    if (upload(tmp, &d_taps, f.taps)) { free_all(tmp); return 1; }
    float *Wf = nullptr, *WfT = nullptr;
    if (dev_alloc(net.allocs, &Wf, (size_t)Nf * Dp) || dev_alloc(net.allocs, &WfT, (size_t)Dp * Nf)) { free_all(tmp); return 1; }
    hipLaunchKernelGGL(compose_front_kernel, dim3((Dp + 255) / 256, Nf), dim3(256), 0, 0, d_taps, net.dec_in.w, T, f.ci, Cip, f.co, Cop, Dp, Wf, WfT);
    if (!hip_ok(hipGetLastError(), "compose_front_kernel") || !hip_ok(hipDeviceSynchronize(), "compose_front_kernel")) { free_all(tmp); return 1; }
    free_all(tmp);
    std::vector<float> bf((size_t)Nf, 0.f), zb((size_t)Dp, 0.f);
    for (int t = 0; t < T; ++t)
        for (int co = 0; co < f.co; ++co) {
            double acc = f.bias[co];
            for (int tap = 0; tap < 3; ++tap) {
                const int ts = t + tap - 1;
                if (ts < 0 || ts >= T) continue;
                for (int ci = 0; ci < f.ci; ++ci) acc += f.taps[((size_t)tap * f.ci + ci) * f.co + co] * (double)dec_in_bias_host[(size_t)ts * Cip + ci];
            }
            bf[(size_t)t * Cop + co] = (float)acc;
        }
    net.front.taps = 1; net.front.K = Dp; net.front.N = Nf; net.front.w = Wf;
    net.front_bwd.taps = 1; net.front_bwd.K = Nf; net.front_bwd.N = Dp; net.front_bwd.w = WfT;
    // bf16 images for the bf16 decoder mode (rounded once from the fp64-composed weights)
    if (dev_alloc(net.allocs, &net.front.wb_hi, (size_t)Nf * Dp) || dev_alloc(net.allocs, &net.front_bwd.wb_hi, (size_t)Dp * Nf) ||
        dev_alloc(net.allocs, &net.front.wb_lo, (size_t)Nf * Dp) || dev_alloc(net.allocs, &net.front_bwd.wb_lo, (size_t)Dp * Nf) ||
        launch_f32_split_bf16(Wf, net.front.wb_hi, net.front.wb_lo, (size_t)Nf * Dp, nullptr) ||
        launch_f32_split_bf16(WfT, net.front_bwd.wb_hi, net.front_bwd.wb_lo, (size_t)Dp * Nf, nullptr))
        return 1;
    GEM_HIP(hipDeviceSynchronize());
    return upload(net.allocs, &net.front.bias, bf) || upload(net.allocs, &net.front_bwd.bias, zb);
}

}  // namespace gem

using namespace gem;

extern "C" {

int gem_load_vae(gem_handle* h, int stage, int n_blobs, const float* const* blobs, const int64_t* n_elem) {
    if (!h || stage < 0 || stage > 1 || !blobs || !n_elem) { set_error("gem_load_vae: bad argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    const gem_config& c = h->cfg;
    const int nh = c.n_hidden, T = h->T, D = h->D, Dp = h->Dp, C = h->C;
    const int flat = h->top * T;
    // expected blob list (globalegomocap_amd.vae.VAEShape.schema order)
    std::vector<int64_t> expect;
    auto conv_bn = [&](int ci, int co, bool bn) {
        expect.push_back((int64_t)ci * co * 3); expect.push_back(co);
        if (bn) for (int q = 0; q < 4; ++q) expect.push_back(co);
    };
    { int ci = C; for (int i = 0; i < nh; ++i) { conv_bn(ci, c.hidden[i], true); ci = c.hidden[i]; } }
    for (int q = 0; q < 2; ++q) { expect.push_back((int64_t)D * flat); expect.push_back(D); }
    expect.push_back((int64_t)flat * D); expect.push_back(flat);
    for (int i = nh - 1; i >= 1; --i) conv_bn(c.hidden[i], c.hidden[i - 1], true);
    conv_bn(c.hidden[0], c.hidden[0], true);
    conv_bn(c.hidden[0], C, false);
    if ((int)expect.size() != n_blobs) { set_error("gem_load_vae: expected " + std::to_string(expect.size()) + " blobs, got " + std::to_string(n_blobs)); return 1; }
    for (int i = 0; i < n_blobs; ++i)
        if (expect[i] != n_elem[i] || !blobs[i]) { set_error("gem_load_vae: size mismatch for blob " + std::to_string(i)); return 1; }

    StageNet& net = h->net[stage];
    if (net.loaded) GEM_HIP(hipDeviceSynchronize());      // reloading: launches that still read the old weights must be done
    drop_graphs(h);                                       // captured calls hold pointers to the weights freed below
    free_all(net.allocs);
    net = StageNet();
    int bi = 0;
    // ---- encoder convs
    { int ci = C;
      for (int i = 0; i < nh; ++i) {
          FoldedConv f = fold_conv(blobs[bi], blobs[bi + 1], blobs + bi + 2, ci, c.hidden[i], false);
          bi += 6;
          Layer L;
          if (make_conv_layers(net, f, &L, nullptr)) return 1;
          net.enc.push_back(L);
          ci = c.hidden[i];
      } }
    // ---- fc_mu | fc_var  ->  N = 2*Dp, K = T*topp, k = t*topp + c  <-  reference index c*T + t
    { const int Kp = T * h->topp;
      std::vector<float> wv((size_t)2 * Dp * Kp, 0.f), bv((size_t)2 * Dp, 0.f);
      for (int q = 0; q < 2; ++q) {
          const float* W = blobs[bi + 2 * q]; const float* b = blobs[bi + 2 * q + 1];
          for (int n = 0; n < D; ++n) {
              for (int cc = 0; cc < h->top; ++cc)
                  for (int t = 0; t < T; ++t) wv[((size_t)q * Dp + n) * Kp + (size_t)t * h->topp + cc] = W[(size_t)n * flat + (size_t)cc * T + t];
              bv[(size_t)q * Dp + n] = b[n];
          }
      }
      bi += 4;
      net.fc.taps = 1; net.fc.K = Kp; net.fc.N = 2 * Dp;
      if (upload(net.allocs, &net.fc.w, wv) || upload(net.allocs, &net.fc.bias, bv) || upload_bf16(net.allocs, &net.fc, wv)) return 1; }
    // ---- decoder_input: forward N = T*topp (n = t*topp + c), K = Dp; backward-data is the transpose
    std::vector<float> dec_in_bias_tm;      // time-major, padded (for compose_front)
    { const int Np = T * h->topp;
      const float* W = blobs[bi]; const float* b = blobs[bi + 1];
      bi += 2;
      std::vector<float> wf((size_t)Np * Dp, 0.f), bf(Np, 0.f), wb((size_t)Dp * Np, 0.f), zb(Dp, 0.f);
      for (int cc = 0; cc < h->top; ++cc)
          for (int t = 0; t < T; ++t) {
              const size_t n = (size_t)t * h->topp + cc, src = (size_t)cc * T + t;
              bf[n] = b[src];
              for (int k = 0; k < D; ++k) {
                  const float v = W[src * D + k];
                  wf[n * Dp + k] = v;
                  wb[(size_t)k * Np + n] = v;
              }
          }
      net.dec_in.taps = 1; net.dec_in.K = Dp; net.dec_in.N = Np;
      net.dec_in_bwd.taps = 1; net.dec_in_bwd.K = Np; net.dec_in_bwd.N = Dp;
      if (upload(net.allocs, &net.dec_in.w, wf) || upload(net.allocs, &net.dec_in.bias, bf) || upload_bf16(net.allocs, &net.dec_in, wf))
          return 1;
      if (upload(net.allocs, &net.dec_in_bwd.w, wb) || upload(net.allocs, &net.dec_in_bwd.bias, zb) ||
          upload_bf16(net.allocs, &net.dec_in_bwd, wb)) return 1;
      dec_in_bias_tm = bf; }
    // ---- decoder convs
    FoldedConv first_conv;
    auto add_dec = [&](int ci, int co, bool transposed, bool bn) -> int {
        FoldedConv f = fold_conv(blobs[bi], blobs[bi + 1], bn ? blobs + bi + 2 : nullptr, ci, co, transposed);
        bi += bn ? 6 : 2;
        if (net.dec.empty()) first_conv = f;
        Layer Lf, Lb;
        net.host_fwd.emplace_back();
        net.host_bwd.emplace_back();
        if (make_conv_layers(net, f, &Lf, &Lb, &net.host_fwd.back(), &net.host_bwd.back())) return 1;
        net.dec.push_back(Lf);
        net.dec_bwd.push_back(Lb);
        return 0;
    };
    for (int i = nh - 1; i >= 1; --i)
        if (add_dec(c.hidden[i], c.hidden[i - 1], true, true)) return 1;
    if (add_dec(c.hidden[0], c.hidden[0], true, true)) return 1;
    if (add_dec(c.hidden[0], C, false, false)) return 1;
    // fuse as many trailing decoder convs as fit the LDS of one CU (tail.hip); GEM_NO_TAIL=1 disables it
    net.tail_start = -1;
    // The chain starts at conv 1 at the earliest: from conv 0, its 512x256 weights (3 MB per workgroup and round from L2) cost
    // more than the batched GEMM they replace (measured: 13.4 k vs 14.3 k windows/s at 240 windows).
    if (!dev_env("GEM_NO_TAIL"))
        for (int st = 1; st < (int)net.dec.size(); ++st) {
            const size_t bytes = plan_tail(net.dec, st, T, h->J, nullptr);
            if (bytes && bytes <= 160 * 1024) { net.tail_start = st; net.tail_lds = bytes; break; }
        }
    // decoder_input o conv 0 as one layer, when the tail takes over right behind conv 0 (GEM_NO_FRONT=1 keeps the two layers)
    if (net.tail_start == 1 && !dev_env("GEM_NO_FRONT") && compose_front(h, net, first_conv, dec_in_bias_tm.data())) return 1;
    // the same tail layers as per-wave bf16 fragment streams for the multi-window bf16 tail (tail_bf16.hip)
    if (build_tail_bf16_stream(h, net)) return 1;
    net.host_fwd.clear(); net.host_fwd.shrink_to_fit();
    net.host_bwd.clear(); net.host_bwd.shrink_to_fit();
    net.loaded = true;
    return 0;
}

}  // extern "C"
