// Skeleton sequences as PNG scanlines from the device: what `render=DIR` / `--render DIR` writes.  Included
// from errors.hip.
//
//   gem_render_layout      row bytes, image bytes and image stride of a width x height image                     (host)
//   gem_skeleton_capsules  [F,15,3] joints -> the 30 capsules of every frame (15 spheres, the 15 MESH_LINES) and their colours
//   gem_render_capsules    capsule ranges through one orthographic view -> every image's uncompressed PNG scanline stream
//
// A scene is a list of capsules (segment a-b, radius r, one colour); image i draws the range first[i] .. first[i+1] of it.  One
// workgroup renders one band of 16 rows of one image: its output is one contiguous run of 16 (1 + 3 W) bytes of the scanline
// stream -- a multiple of 16 that starts 16-byte aligned -- which the threads assemble byte by byte in LDS and the workgroup then
// streams out as aligned 16-byte stores (the last band of an image is shorter: its last few bytes go out singly).  The band is
// walked in tiles of 16 x 16 pixels, one pixel per thread.  Per tile the image's capsules are projected into view space 128 at a
// time, cooperatively, and only those whose 2-D box, grown by r, touches the tile are kept in an LDS list; each pixel walks that list
// with a four-compare reject before the intersection.  The winner is the smallest (t, index) in lexicographic order, so the order
// in which the list was filled does not matter: no floating-point atomics, the same bytes on every call.  All arithmetic float64.
#pragma once
#include <cmath>
#include <vector>

namespace gem {

constexpr int RND_BAND = 16, RND_TILE = 16, RND_THREADS = RND_BAND * RND_TILE;
constexpr int RND_CHUNK = 128;                    // capsules projected per round
constexpr int RND_MAX_WIDTH = 1024;               // 16 (1 + 3 W) bytes of band + the list stay below 64 KB of LDS
constexpr int RND_CAPSULES = 30;                  // per skeleton frame
constexpr double RND_JOINT_R = SPH_R, RND_LINE_R = CYL_R;
constexpr double RND_PARALLEL = 1e-24;            // an axis counts as parallel to `forward` when sin^2 of the angle is at most this
constexpr double RND_AMBIENT = 0.3, RND_DIFFUSE = 0.7;

struct RenderCap {          // a capsule in view coordinates: 64 bytes
    double ax, ay, az, dx, dy, dz, r;
    int32_t idx;            // its index in the whole list
    uint32_t rgb;
};

struct RenderArgs {
    const double* geom;         // [n,7] a, b, r in world coordinates
    const uint32_t* rgb;        // [n]
    const int32_t* first;       // [n_images + 1]
    gem_view v;
    unsigned char* out;
    int64_t stride;
    int32_t* ids;               // [n_images,H,W] or nullptr
    double* depth;              // [n_images,H,W] or nullptr
};

struct CapsuleArgs {
    const double* seq;          // [F,15,3]
    const double* crt;          // [13] or nullptr
    double* geom;               // [F*30,7]
    uint32_t* rgb;              // [F*30]
    int64_t n;                  // F*30
    uint32_t rgb_joint, rgb_line;
    int lines[MESH_L][2];
};

__global__ __launch_bounds__(256) void skeleton_capsules_kernel(CapsuleArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n) return;
    const int64_t f = k / RND_CAPSULES;
    const int c = (int)(k - f * RND_CAPSULES);
    const int ja = c < MESH_J ? c : a.lines[c - MESH_J][0];
    const int jb = c < MESH_J ? c : a.lines[c - MESH_J][1];
    double* o = a.geom + k * 7;
    for (int e = 0; e < 2; ++e) {
        const double* p = a.seq + (f * MESH_J + (e ? jb : ja)) * 3;
        double q[3] = {p[0], p[1], p[2]};
        if (a.crt) {          // c * (p . R) + t, as skeleton_mesh_kernel moves its joints
            const double s = a.crt[0];
            const double* R = a.crt + 1;
            const double* t = a.crt + 10;
            const double p0 = q[0], p1 = q[1], p2 = q[2];
            for (int d = 0; d < 3; ++d) q[d] = s * (p0 * R[d] + p1 * R[3 + d] + p2 * R[6 + d]) + t[d];
        }
        for (int d = 0; d < 3; ++d) o[3 * e + d] = q[d];
    }
    o[6] = c < MESH_J ? RND_JOINT_R : RND_LINE_R;
    a.rgb[k] = c < MESH_J ? a.rgb_joint : a.rgb_line;
}

// The entry of the pixel's line (u, v, .) into capsule c: false on a miss; t and the vector n from the closest point of the segment
// to the hit otherwise ("Hit").
__device__ inline bool render_hit(const RenderCap& c, double u, double v, double* t_out, double* n) {
    const double wx = u - c.ax, wy = v - c.ay;
    const double dxy2 = c.dx * c.dx + c.dy * c.dy, dd = dxy2 + c.dz * c.dz;
    const double r2 = c.r * c.r;
    double cx = wx, cy = wy, cz = c.az;          // the end sphere at a, as seen from the pixel: (cx, cy) = pixel - centre
    if (dxy2 <= RND_PARALLEL * dd) {             // a sphere, or an axis along `forward`: the nearer end
        if (c.dz < 0.0) { cx = wx - c.dx; cy = wy - c.dy; cz = c.az + c.dz; }
    } else {
        const double q = wx * c.dy - wy * c.dx;              // |q| / sqrt(dxy2): the distance of the two lines
        const double disc = r2 * dxy2 - q * q;
        if (!(disc >= 0.0)) return false;
        const double e = wx * c.dx + wy * c.dy;
        const double tc = (c.dz * e - sqrt(dd * disc)) / dxy2;          // the entry into the infinite cylinder, relative to a's depth
        const double s = (e + tc * c.dz) / dd;                          // its foot on the axis
        if (s > 0.0 && s < 1.0) {
            n[0] = wx - s * c.dx; n[1] = wy - s * c.dy; n[2] = tc - s * c.dz;
            *t_out = c.az + tc;
            return true;
        }
        if (!(s <= 0.0)) { cx = wx - c.dx; cy = wy - c.dy; cz = c.az + c.dz; }
    }
    const double h2 = r2 - (cx * cx + cy * cy);
    if (!(h2 >= 0.0)) return false;
    const double h = sqrt(h2);
    n[0] = cx; n[1] = cy; n[2] = -h;
    *t_out = cz - h;
    return true;
}

__global__ __launch_bounds__(RND_THREADS) void render_capsules_kernel(RenderArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char render_lds[];
    __shared__ int n_list;
    RenderCap* list = reinterpret_cast<RenderCap*>(render_lds);
    unsigned char* band = render_lds + RND_CHUNK * sizeof(RenderCap);
    const int tid = threadIdx.x, ty = tid / RND_TILE, tx = tid % RND_TILE;
    const int W = a.v.width, H = a.v.height, row_bytes = 1 + 3 * W;
    const int img = blockIdx.y, y0 = blockIdx.x * RND_BAND, rows = min(RND_BAND, H - y0);
    const int c0 = a.first[img], c1 = a.first[img + 1];
    const double s = 2.0 * a.v.half_width / W;
    const int py = y0 + ty;
    const double v = (py + 0.5 - 0.5 * H) * s;
    const double vlo = (y0 + 0.5 - 0.5 * H) * s, vhi = (y0 + rows - 1 + 0.5 - 0.5 * H) * s;
    if (tid < rows) band[tid * row_bytes] = 0;          // the filter byte of every scanline
    for (int x0 = 0; x0 < W; x0 += RND_TILE) {
        const int px = x0 + tx;
        const bool active = ty < rows && px < W;
        const double u = (px + 0.5 - 0.5 * W) * s;
        const double ulo = (x0 + 0.5 - 0.5 * W) * s, uhi = (min(x0 + RND_TILE, W) - 1 + 0.5 - 0.5 * W) * s;
        double best_t = INFINITY, bn[3] = {0.0, 0.0, -1.0};
        int best = -1;
        uint32_t best_rgb = 0;
        for (int cb = c0; cb < c1; cb += RND_CHUNK) {
            if (tid == 0) n_list = 0;
            __syncthreads();
            if (tid < RND_CHUNK && cb + tid < c1) {
                const double* g = a.geom + (int64_t)(cb + tid) * 7;
                double p[2][3];
                for (int e = 0; e < 2; ++e) {
                    const double x = g[3 * e] - a.v.centre[0], y = g[3 * e + 1] - a.v.centre[1], z = g[3 * e + 2] - a.v.centre[2];
                    p[e][0] = x * a.v.right[0] + y * a.v.right[1] + z * a.v.right[2];
                    p[e][1] = x * a.v.down[0] + y * a.v.down[1] + z * a.v.down[2];
                    p[e][2] = x * a.v.forward[0] + y * a.v.forward[1] + z * a.v.forward[2];
                }
                const double r = g[6], m = r * 1.000001 + 1e-9;          // (the box is a little larger than the capsule: it only saves work)
                const bool outside = fmin(p[0][0], p[1][0]) - m > uhi || fmax(p[0][0], p[1][0]) + m < ulo ||
                                     fmin(p[0][1], p[1][1]) - m > vhi || fmax(p[0][1], p[1][1]) + m < vlo;
                if (!outside) {
                    RenderCap c;
                    c.ax = p[0][0]; c.ay = p[0][1]; c.az = p[0][2];
                    c.dx = p[1][0] - p[0][0]; c.dy = p[1][1] - p[0][1]; c.dz = p[1][2] - p[0][2];
                    c.r = r; c.idx = cb + tid; c.rgb = a.rgb[cb + tid];
                    list[atomicAdd(&n_list, 1)] = c;
                }
            }
            __syncthreads();
            const int n = n_list;
            if (active)
                for (int k = 0; k < n; ++k) {
                    const RenderCap& c = list[k];
                    const double m = c.r * 1.000001 + 1e-9;
                    const double bx = c.ax + c.dx, by = c.ay + c.dy;
                    if (fmin(c.ax, bx) - m > u || fmax(c.ax, bx) + m < u || fmin(c.ay, by) - m > v || fmax(c.ay, by) + m < v) continue;
                    double t, nn[3];
                    if (!render_hit(c, u, v, &t, nn)) continue;
                    if (t < best_t || (t == best_t && c.idx < best)) {
                        best_t = t; best = c.idx; best_rgb = c.rgb;
                        bn[0] = nn[0]; bn[1] = nn[1]; bn[2] = nn[2];
                    }
                }
            __syncthreads();
        }
        if (active) {
            unsigned char* o = band + ty * row_bytes + 1 + 3 * px;
            if (best < 0) {
                o[0] = 255; o[1] = 255; o[2] = 255;
            } else {
                const double len = sqrt(bn[0] * bn[0] + bn[1] * bn[1] + bn[2] * bn[2]);
                const double L = RND_AMBIENT + RND_DIFFUSE * fmax(0.0, -bn[2] / len);
                for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)(int)floor((double)((best_rgb >> (8 * ch)) & 255u) * L + 0.5);
            }
            const int64_t at = ((int64_t)img * H + py) * W + px;
            if (a.ids) a.ids[at] = best < 0 ? -1 : best - c0;
            if (a.depth) a.depth[at] = best_t;
        }
    }
    __syncthreads();
    // the band's bytes: whole 16-byte runs as aligned stores, the ragged end of an image's last band singly
    typedef uint32_t render_u4 __attribute__((ext_vector_type(4)));
    const int total = rows * row_bytes;
    unsigned char* dst = a.out + (int64_t)img * a.stride + (int64_t)y0 * row_bytes;
    const render_u4* src = reinterpret_cast<const render_u4*>(band);
    for (int i = tid; i < total / 16; i += RND_THREADS) __builtin_nontemporal_store(src[i], reinterpret_cast<render_u4*>(dst) + i);
    for (int i = total / 16 * 16 + tid; i < total; i += RND_THREADS) dst[i] = band[i];
}

inline int64_t render_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

}  // namespace gem

extern "C" {

int gem_render_layout(int width, int height, int64_t* out) {
    using namespace gem;
    if (!out) { set_error("gem_render_layout: null argument"); return 1; }
    if (width < 1 || height < 1) { set_error("gem_render_layout: width and height must be at least 1"); return 1; }
    out[0] = 1 + 3 * (int64_t)width;
    out[1] = out[0] * height;
    out[2] = render_round_up(out[1], 16);
    return 0;
}

int gem_skeleton_capsules(const double* d_seq, int64_t n_frames, const double* d_crt, uint32_t rgb_joint, uint32_t rgb_line,
                          double* d_geom, uint32_t* d_rgb, void* stream) {
    using namespace gem;
    if (n_frames < 0) { set_error("gem_skeleton_capsules: n_frames < 0"); return 1; }
    if (n_frames == 0) return 0;
    if (!d_seq || !d_geom || !d_rgb) { set_error("gem_skeleton_capsules: null argument"); return 1; }
    if (n_frames > 0x7fffffffll / RND_CAPSULES) { set_error("gem_skeleton_capsules: too many frames for one launch"); return 1; }
    CapsuleArgs a;
    a.seq = d_seq; a.crt = d_crt; a.geom = d_geom; a.rgb = d_rgb; a.n = n_frames * RND_CAPSULES;
    a.rgb_joint = rgb_joint & 0xffffffu; a.rgb_line = rgb_line & 0xffffffu;
    for (int l = 0; l < MESH_L; ++l) { a.lines[l][0] = MESH_LINES[l][0]; a.lines[l][1] = MESH_LINES[l][1]; }
    hipLaunchKernelGGL(skeleton_capsules_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_render_capsules(const double* d_geom, const uint32_t* d_rgb, int64_t n_capsules, const int32_t* d_first, int n_images,
                        const gem_view* view, void* d_out, int64_t image_stride_bytes, int32_t* d_ids, double* d_depth, void* stream) {
    using namespace gem;
    if (!view) { set_error("gem_render_capsules: null view"); return 1; }
    const gem_view& v = *view;
    if (v.width < 1 || v.height < 1) { set_error("gem_render_capsules: width and height must be at least 1"); return 1; }
    if (v.width > RND_MAX_WIDTH) { set_error("gem_render_capsules: images wider than 1024 pixels are not supported"); return 1; }
    if (n_images < 0 || n_images > 65535) { set_error("gem_render_capsules: between 0 and 65535 images per call"); return 1; }
    if (n_capsules < 0 || n_capsules > 0x7fffffffll) { set_error("gem_render_capsules: the capsule count must fit 31 bits"); return 1; }
    const double* ax[3] = {v.right, v.down, v.forward};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double dot = ax[i][0] * ax[j][0] + ax[i][1] * ax[j][1] + ax[i][2] * ax[j][2];
            if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-9)) {
                set_error("gem_render_capsules: right, down and forward of the view must be orthonormal (to 1e-9)"); return 1;
            }
        }
    if (!(v.half_width > 0.0) || !std::isfinite(v.half_width) || !std::isfinite(v.centre[0] + v.centre[1] + v.centre[2])) {
        set_error("gem_render_capsules: the view needs a finite centre and a positive, finite half_width"); return 1;
    }
    int64_t lay[3];
    if (gem_render_layout(v.width, v.height, lay)) return 1;
    if (image_stride_bytes < lay[1] || image_stride_bytes % 16) {
        set_error("gem_render_capsules: the image stride must be at least the image's bytes, H (1 + 3 W), and a multiple of 16"); return 1;
    }
    if (reinterpret_cast<uintptr_t>(d_out) % 16) { set_error("gem_render_capsules: the output must be 16-byte aligned"); return 1; }
    if (n_images == 0) return 0;
    if (!d_out || !d_first || (n_capsules > 0 && (!d_geom || !d_rgb))) { set_error("gem_render_capsules: null argument"); return 1; }
    // the ranges are read back and checked before anything is launched: a kernel must not be handed an index it cannot trust
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<int32_t> first((size_t)n_images + 1);
    GEM_HIP(hipMemcpyAsync(first.data(), d_first, first.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GEM_HIP(hipStreamSynchronize(s));
    if (first[0] < 0 || first[n_images] > n_capsules) { set_error("gem_render_capsules: first[] leaves the capsule list"); return 1; }
    for (int i = 0; i < n_images; ++i)
        if (first[i] > first[i + 1]) { set_error("gem_render_capsules: first[] must be ascending"); return 1; }
    RenderArgs a;
    a.geom = d_geom; a.rgb = d_rgb; a.first = d_first; a.v = v; a.out = static_cast<unsigned char*>(d_out); a.stride = image_stride_bytes;
    a.ids = d_ids; a.depth = d_depth;
    const size_t lds = RND_CHUNK * sizeof(RenderCap) + (size_t)RND_BAND * (size_t)lay[0];
    hipLaunchKernelGGL(render_capsules_kernel, dim3((unsigned)((v.height + RND_BAND - 1) / RND_BAND), (unsigned)n_images), dim3(RND_THREADS),
                       lds, s, a);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
