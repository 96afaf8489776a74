// The camera's view: the heat-maps the reprojection term samples, with the reprojected skeletons drawn over
// them -- what `render_camera=DIR` / `--render_camera DIR` writes.  Included from errors.hip.
//
//   gem_project_sequence  [n,J,3] joints (behind a similarity, through the frames' cameras) -> their fisheye image points [n,J,2]
//   gem_render_camera     heat-maps + image points of up to 8 sequences -> every image's uncompressed PNG scanline stream
//
// The projection is sequence_quality_kernel's: X_cam = R^T (X - t) in float64, rounded once, then energy_device.h's fisheye_uv.
// The drawing keeps render_capsules_kernel's shape: one workgroup per band of 16 rows of one image, walked in tiles of 16 x 16
// pixels, the band's bytes assembled in LDS and streamed out as aligned 16-byte stores (the ragged end of an image's last band
// singly).  Per band the image's primitives (30 per sequence: 15 discs, 15 thick segments) are culled ONCE against the band's rows
// and compacted into an LDS list in priority order (higher sequence first, then joints before lines, then the lower index), so a
// pixel walks the list with a two-compare reject in x and stops at its first hit: no atomics at all, the same bytes on every call.
// The background reads its 4 x 15 texels straight from global memory: at 512 x 512 a tile of 16 x 16 pixels lies over at most
// 3 x 3 texels (540 bytes), which the vector cache serves; at small sizes a band spans more texel rows than LDS holds.
// Overlay arithmetic is float64 on the widened fp32 image points, the background fp32 (heat_tap / heat_bilinear).
#pragma once
#include "energy_device.h"

namespace gem {

constexpr int CAM_MAX_SEQ = 8;
constexpr int CAM_PRIMS = RND_CAPSULES;                         // per sequence and image
constexpr int CAM_MAX_PRIMS = CAM_MAX_SEQ * CAM_PRIMS;          // 240: one per thread of the cull pass
static_assert(CAM_MAX_PRIMS <= RND_THREADS, "the cull pass gives every primitive one thread");
constexpr double CAM_CROP_X0 = 128.0, CAM_CROP = 1024.0;        // the square of the 1280 x 1024 image the heat-maps cover

struct CamPrim {            // a disc (a == b) or a thick segment in image pixels: 48 bytes
    double ax, ay, dx, dy, r;
    int32_t id;             // s * 30 + c
    uint32_t rgb;
};

struct CameraViewArgs {
    const float* heat;          // [n_images,H,W,J] or nullptr
    const float* uv;            // [S,n_images,J,2]
    const uint32_t* rgb;        // [S]
    unsigned char* out;
    int64_t stride;
    int32_t* ids;               // [n_images,N,N] or nullptr
    float* response;            // [n_images,N,N] or nullptr
    double joint_r, line_r;
    int N, S, n_images, H, W;
    uint32_t joint_mask, rgb_heat;
    int lines[MESH_L][2];
};

struct ProjectArgs {
    const double* seq;          // [n,J,3]
    const double* crt;          // [13] or nullptr
    const double* cams;         // [n,4,4] or nullptr
    float* uv;                  // [n,J,2]
    int64_t n;                  // frames * J
    int J, n_poly;
    float poly[GEM_MAX_POLY];
    float cx, cy;
};

__global__ __launch_bounds__(256) void project_sequence_kernel(ProjectArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n) return;
    const int64_t f = k / a.J;
    const double* p = a.seq + k * 3;
    double q[3] = {p[0], p[1], p[2]};
    if (a.crt) {          // c * (p . R) + t, as skeleton_capsules_kernel moves its joints
        const double s = a.crt[0];
        const double* R = a.crt + 1;
        const double* t = a.crt + 10;
        const double p0 = q[0], p1 = q[1], p2 = q[2];
        for (int d = 0; d < 3; ++d) q[d] = s * (p0 * R[d] + p1 * R[3 + d] + p2 * R[6 + d]) + t[d];
    }
    float xc[3];
    if (a.cams) {          // X_cam = R^T (X - t), float64, rounded once: sequence_quality_kernel's arithmetic
#pragma clang fp contract(off)
        const double* M = a.cams + f * 16;
        const double d0 = q[0] - M[3], d1 = q[1] - M[7], d2 = q[2] - M[11];
        for (int r = 0; r < 3; ++r) xc[r] = (float)(M[r] * d0 + M[4 + r] * d1 + M[8 + r] * d2);
    } else {
        for (int r = 0; r < 3; ++r) xc[r] = (float)q[r];
    }
    const FisheyeUV w = fisheye_uv(a.poly, a.n_poly, a.cx, a.cy, xc[0], xc[1], xc[2]);
    a.uv[k * 2] = w.u;          // a joint on the optical axis: 0 * inf, not finite
    a.uv[k * 2 + 1] = w.v;
}

// Is the pixel centre (u, v) within r of the primitive?  Plain IEEE float64, like the numpy it is checked against.
__device__ inline bool camera_covers(const CamPrim& c, double u, double v) {
#pragma clang fp contract(off)
    const double wx = u - c.ax, wy = v - c.ay;
    const double dd = c.dx * c.dx + c.dy * c.dy;
    double t = 0.0;
    if (dd > 0.0) t = fmin(fmax((wx * c.dx + wy * c.dy) / dd, 0.0), 1.0);
    const double ex = wx - t * c.dx, ey = wy - t * c.dy;
    return ex * ex + ey * ey <= c.r * c.r;
}

__global__ __launch_bounds__(RND_THREADS) void render_camera_kernel(CameraViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char camera_lds[];
    // the carve: the band's bytes (16 rows: a multiple of 16), then the list, then the four waves' counts
    CamPrim* list = reinterpret_cast<CamPrim*>(camera_lds + RND_BAND * (1 + 3 * a.N));
    int* counts = reinterpret_cast<int*>(list + CAM_MAX_PRIMS);
    unsigned char* band = camera_lds;
    const int tid = threadIdx.x, ty = tid / RND_TILE, tx = tid % RND_TILE;
    const int N = a.N, row_bytes = 1 + 3 * N;
    const int img = blockIdx.y, y0 = blockIdx.x * RND_BAND, rows = min(RND_BAND, N - y0);
    const int py = y0 + ty;
    const double scale = CAM_CROP / (double)N;
    const float scale_f = 1024.f / (float)N;
    if (tid < rows) band[tid * row_bytes] = 0;          // the filter byte of every scanline

    // the band's primitives, in priority order: thread k looks at sequence S-1 - k/30, primitive k % 30
    const int n_prims = a.S * CAM_PRIMS;
    bool keep = false;
    CamPrim mine;
    if (tid < n_prims) {
        const int s = a.S - 1 - tid / CAM_PRIMS, c = tid % CAM_PRIMS;
        const int ja = c < MESH_J ? c : a.lines[c - MESH_J][0];
        const int jb = c < MESH_J ? c : a.lines[c - MESH_J][1];
        const float* pa = a.uv + (((int64_t)s * a.n_images + img) * MESH_J + ja) * 2;
        const float* pb = a.uv + (((int64_t)s * a.n_images + img) * MESH_J + jb) * 2;
        const double ax = (double)pa[0], ay = (double)pa[1], bx = (double)pb[0], by = (double)pb[1];
        const double r = c < MESH_J ? a.joint_r : a.line_r, m = r * 1.000001 + 1e-9;          // (the box is a little larger: it only saves work)
        const double vlo = (y0 + 0.5) * scale, vhi = (y0 + rows - 1 + 0.5) * scale;
        const bool finite = isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by);          // a primitive with a non-finite coordinate is never drawn
        keep = finite && !(fmin(ay, by) - m > vhi || fmax(ay, by) + m < vlo);
        mine.ax = ax; mine.ay = ay; mine.dx = bx - ax; mine.dy = by - ay; mine.r = r;
        mine.id = s * CAM_PRIMS + c; mine.rgb = a.rgb[s];
    }
    const unsigned long long kept = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) counts[wave] = __popcll(kept);
    __syncthreads();
    int at = __popcll(kept & ((1ull << lane) - 1ull)), n_list = 0;
    for (int w = 0; w < RND_THREADS / 64; ++w) {
        if (w < wave) at += counts[w];
        n_list += counts[w];
    }
    if (keep) list[at] = mine;
    __syncthreads();

    const float* hm = a.heat ? a.heat + (int64_t)img * a.H * a.W * MESH_J : nullptr;
    for (int x0 = 0; x0 < N; x0 += RND_TILE) {
        const int px = x0 + tx;
        if (!(ty < rows && px < N)) continue;
        // background: the largest bilinear sample over the masked joints, fp32
        float m = 0.f;
        if (hm && a.joint_mask) {
            float uf, vf;
            {
#pragma clang fp contract(off)
                uf = 128.f + ((float)px + 0.5f) * scale_f;
                vf = ((float)py + 0.5f) * scale_f;
            }
            const HeatTap k = heat_tap(uf, vf, a.H, a.W);
            const float* t_nw = hm + ((int64_t)k.ya * a.W + k.xa) * MESH_J;
            const float* t_ne = hm + ((int64_t)k.ya * a.W + k.xb) * MESH_J;
            const float* t_sw = hm + ((int64_t)k.yc * a.W + k.xa) * MESH_J;
            const float* t_se = hm + ((int64_t)k.yc * a.W + k.xb) * MESH_J;
            for (int j = 0; j < MESH_J; ++j) {
                if (!((a.joint_mask >> j) & 1u)) continue;
                float nw = t_nw[j], ne = t_ne[j], sw = t_sw[j], se = t_se[j];
                m = fmaxf(m, heat_bilinear(k, nw, ne, sw, se));
            }
            m = fminf(m, 1.f);
        }
        // overlay: the first primitive of the list that covers the pixel's centre
        double u, v;
        {
#pragma clang fp contract(off)
            u = CAM_CROP_X0 + (px + 0.5) * scale;
            v = (py + 0.5) * scale;
        }
        int best = -1;
        uint32_t best_rgb = 0;
        for (int i = 0; i < n_list; ++i) {
            const CamPrim& c = list[i];
            const double mr = c.r * 1.000001 + 1e-9, bx = c.ax + c.dx;
            if (fmin(c.ax, bx) - mr > u || fmax(c.ax, bx) + mr < u) continue;
            if (camera_covers(c, u, v)) { best = c.id; best_rgb = c.rgb; break; }
        }
        unsigned char* o = band + ty * row_bytes + 1 + 3 * px;
        if (best >= 0) {
            for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)((best_rgb >> (8 * ch)) & 255u);
        } else {
#pragma clang fp contract(off)
            for (int ch = 0; ch < 3; ++ch) {
                const double c = (double)((a.rgb_heat >> (8 * ch)) & 255u);
                o[ch] = (unsigned char)(int)floor(255.0 + (c - 255.0) * (double)m + 0.5);
            }
        }
        const int64_t px_at = ((int64_t)img * N + py) * N + px;
        if (a.ids) a.ids[px_at] = best;
        if (a.response) a.response[px_at] = m;
    }
    __syncthreads();
    // the band's bytes: whole 16-byte runs as aligned stores, the ragged end of an image's last band singly
    typedef uint32_t camera_u4 __attribute__((ext_vector_type(4)));
    const int total = rows * row_bytes;
    unsigned char* dst = a.out + (int64_t)img * a.stride + (int64_t)y0 * row_bytes;
    const camera_u4* src = reinterpret_cast<const camera_u4*>(band);
    for (int i = tid; i < total / 16; i += RND_THREADS) __builtin_nontemporal_store(src[i], reinterpret_cast<camera_u4*>(dst) + i);
    for (int i = total / 16 * 16 + tid; i < total; i += RND_THREADS) dst[i] = band[i];
}

}  // namespace gem

extern "C" {

int gem_project_sequence(gem_handle* h, const double* d_seq, const double* d_crt, const double* d_cams, int64_t n_frames, float* d_uv,
                         void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_project_sequence: null handle"); return 1; }
    if (n_frames < 0) { set_error("gem_project_sequence: n_frames < 0"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_seq || !d_uv) { set_error("gem_project_sequence: null argument"); return 1; }
    if (n_frames > 0x7fffffffll / GEM_MAX_JOINTS) { set_error("gem_project_sequence: too many frames for one launch"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    ProjectArgs a;
    a.seq = d_seq; a.crt = d_crt; a.cams = d_cams; a.uv = d_uv; a.J = h->J; a.n = n_frames * h->J; a.n_poly = h->cfg.n_poly;
    for (int i = 0; i < GEM_MAX_POLY; ++i) a.poly[i] = i < a.n_poly ? (float)h->cfg.poly[i] : 0.f;
    a.cx = (float)h->cfg.cx; a.cy = (float)h->cfg.cy;
    hipLaunchKernelGGL(project_sequence_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_render_camera(gem_handle* h, const float* d_heat, const float* d_uv, const uint32_t* d_rgb, int n_sequences, int n_images,
                      const gem_camera_view* view, void* d_out, int64_t image_stride_bytes, int32_t* d_ids, float* d_response,
                      void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_render_camera: null handle"); return 1; }
    if (h->J != MESH_J) { set_error("gem_render_camera: the skeleton drawn has 15 joints; this handle has another n_joints"); return 1; }
    if (!view) { set_error("gem_render_camera: null view"); return 1; }
    const gem_camera_view& v = *view;
    if (v.size < 1 || v.size > RND_MAX_WIDTH) { set_error("gem_render_camera: size must be 1 .. 1024 pixels"); return 1; }
    if (v.joint_mask >> MESH_J) { set_error("gem_render_camera: joint_mask names a joint at or above 15"); return 1; }
    if (!(v.joint_radius >= 0.0) || !(v.line_radius >= 0.0) || !std::isfinite(v.joint_radius) || !std::isfinite(v.line_radius)) {
        set_error("gem_render_camera: joint_radius and line_radius must be finite and not negative"); return 1;
    }
    if (n_sequences < 0 || n_sequences > CAM_MAX_SEQ) { set_error("gem_render_camera: between 0 and 8 sequences per call"); return 1; }
    if (n_images < 0 || n_images > 65535) { set_error("gem_render_camera: between 0 and 65535 images per call"); return 1; }
    int64_t lay[3];
    if (gem_render_layout(v.size, v.size, lay)) return 1;
    if (image_stride_bytes < lay[1] || image_stride_bytes % 16) {
        set_error("gem_render_camera: the image stride must be at least the image's bytes, N (1 + 3 N), and a multiple of 16"); return 1;
    }
    if (reinterpret_cast<uintptr_t>(d_out) % 16) { set_error("gem_render_camera: the output must be 16-byte aligned"); return 1; }
    if (n_images == 0) return 0;
    if (!d_out || (n_sequences > 0 && (!d_uv || !d_rgb))) { set_error("gem_render_camera: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    CameraViewArgs a;
    a.heat = d_heat; a.uv = d_uv; a.rgb = d_rgb; a.out = static_cast<unsigned char*>(d_out); a.stride = image_stride_bytes;
    a.ids = d_ids; a.response = d_response; a.joint_r = v.joint_radius; a.line_r = v.line_radius;
    a.N = v.size; a.S = n_sequences; a.n_images = n_images; a.H = h->cfg.heat_h; a.W = h->cfg.heat_w;
    a.joint_mask = v.joint_mask; a.rgb_heat = v.rgb_heat & 0xffffffu;
    for (int l = 0; l < MESH_L; ++l) { a.lines[l][0] = MESH_LINES[l][0]; a.lines[l][1] = MESH_LINES[l][1]; }
    const size_t lds = (size_t)RND_BAND * (size_t)lay[0] + CAM_MAX_PRIMS * sizeof(CamPrim) + 16;
    hipLaunchKernelGGL(render_camera_kernel, dim3((unsigned)((v.size + RND_BAND - 1) / RND_BAND), (unsigned)n_images), dim3(RND_THREADS),
                       lds, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
