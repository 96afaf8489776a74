// Recordings as the pose network leaves them: one `heatmap` .mat and one `depth` .mat per frame
// (MakeDataForOptimization/process_test_data.py:52-68 reads them with scipy.io.loadmat, one by one).  Included at the end of
// chunk_io.hip: it shares that file's unaligned word reader, its LDS transpose (tile_in / tile_out / transpose_tile) and pread_all.
//
//   gem_mat_scan        host, no GIL: a bounds-checked interpreter of a Level-5 MAT file that LOCATES the numeric array of a given
//                       name and copies nothing (the pickle scanner's sibling)
//   gem_files_sizes     host: the sizes of many files in one call
//   gem_mat_read        host: many files -> one (pinned) block at given positions, each scanned on the way
//   gem_mat_frames      device: ONE launch turns the block's image in HBM into heat [n,H,W,J] f32 and depth [n,J] f64, the payload type
//                       being a per-frame table entry
//   gem_prepare_global  device: est_global = R . est_local + t in float64 without fused multiply-adds, and mean_j |gt - est_global|
//                       per frame, for all chunks of a batch in one launch
#pragma once

namespace gem {
namespace {

// ------------------------------------------------------------------------------------------------------------ the MAT-file interpreter
enum { MI_INT8 = 1, MI_UINT8 = 2, MI_INT32 = 5, MI_UINT32 = 6, MI_SINGLE = 7, MI_DOUBLE = 9, MI_MATRIX = 14, MI_COMPRESSED = 15 };
enum { MX_CELL = 1, MX_STRUCT = 2, MX_OBJECT = 3, MX_CHAR = 4, MX_SPARSE = 5, MX_DOUBLE = 6, MX_SINGLE = 7, MX_UINT64 = 15 };

struct MatScanner {
    const uint8_t* p;
    int64_t len;
    std::string why;

    int refuse(const std::string& m, int64_t at) { if (why.empty()) why = m + " at byte " + std::to_string(at); return GEM_MAT_UNSUPPORTED; }
    uint32_t u32(int64_t at) const { return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24; }

    // One data element's tag at `at`, inside [at, end): its type, where its data lie and how long they are, where the next element
    // starts (`padded`: data are padded to 8 bytes -- everything but miCOMPRESSED).  Every figure is checked against `end` before use.
    bool tag(int64_t at, int64_t end, uint32_t& type, int64_t& data, int64_t& n, int64_t& next) {
        if (at < 0 || at + 8 > end) { refuse("truncated: no room for a data element's tag", at); return false; }
        const uint32_t w0 = u32(at);
        if (w0 >> 16) {                                   // small data element: type in the low half, length in the high half, data in the tag
            type = w0 & 0xffffu; n = (int64_t)(w0 >> 16); data = at + 4; next = at + 8;
            if (n > 4) { refuse("small data element longer than 4 bytes", at); return false; }
            return true;
        }
        type = w0; n = (int64_t)u32(at + 4); data = at + 8;
        if (n > end - data) { refuse("a data element reaches past its container", at); return false; }
        next = data + (type == MI_COMPRESSED ? n : (n + 7) / 8 * 8);
        if (next > end) next = end;                       // (the last element's padding may be cut off)
        return true;
    }

    // The miMATRIX element whose data are [at, end): is it called `name`?  If so, fills `out` (0), or refuses (reason).  `mine` tells
    // the caller whether the name matched at all.
    int matrix(int64_t at, int64_t end, const char* name, gem_mat_array& out, bool& mine) {
        mine = false;
        uint32_t type; int64_t data, n, next;
        if (!tag(at, end, type, data, n, next)) return GEM_MAT_UNSUPPORTED;
        if (type != MI_UINT32 || n != 8) return refuse("array flags are not two miUINT32 words", at);
        const uint32_t flags = u32(data);
        const int cls = (int)(flags & 0xffu);
        const bool is_complex = flags & 0x0800u, is_logical = flags & 0x0200u;
        at = next;
        if (!tag(at, end, type, data, n, next)) return GEM_MAT_UNSUPPORTED;
        if (type != MI_INT32 || n < 4 || n % 4) return refuse("the dimensions are not miINT32", at);
        const int64_t ndim = n / 4, dims_at = data;
        at = next;
        if (!tag(at, end, type, data, n, next)) return GEM_MAT_UNSUPPORTED;
        if (type != MI_INT8) return refuse("the array's name is not miINT8", at);
        const size_t want = strlen(name);
        if ((size_t)n != want || memcmp(p + data, name, want) != 0) return 0;          // another variable: skipped by the caller
        mine = true;
        if (cls == MX_CELL || cls == MX_STRUCT || cls == MX_OBJECT) return refuse("the variable is a cell, struct or object array", at);
        if (cls == MX_SPARSE) return refuse("the variable is sparse", at);
        if (cls == MX_CHAR) return refuse("the variable is a character array", at);
        if (cls != MX_DOUBLE && cls != MX_SINGLE) return refuse("the variable's class is neither double nor single", at);
        if (is_complex) return refuse("the variable is complex", at);
        if (is_logical) return refuse("the variable is logical", at);
        if (ndim > 4) return refuse("more than four dimensions", dims_at);
        int64_t count = 1;
        for (int k = 0; k < 4; ++k) out.dims[k] = 1;
        for (int64_t k = 0; k < ndim; ++k) {
            const int32_t d = (int32_t)u32(dims_at + 4 * k);
            if (d < 0) return refuse("negative dimension", dims_at + 4 * k);
            out.dims[k] = d;
            if (d && count > (1ll << 40) / d) return refuse("dimensions overflow", dims_at);
            count *= d;
        }
        at = next;
        if (!tag(at, end, type, data, n, next)) return GEM_MAT_UNSUPPORTED;
        // MATLAB stores a double array whose values all fit a narrower integer type in that type; loadmat then returns the STORAGE
        // type, which the reference would pickle: left to the caller's loadmat
        if (!((cls == MX_SINGLE && type == MI_SINGLE) || (cls == MX_DOUBLE && type == MI_DOUBLE)))
            return refuse("the data are stored in another type than the array's class (miSINGLE for single, miDOUBLE for double)", at);
        const int64_t item = type == MI_SINGLE ? 4 : 8;
        if (n != count * item) return refuse("the data's length is not the product of the dimensions", at);
        if (data < 0 || data + n > len) return refuse("the data lie outside the file", at);          // (tag() checked it against `end` already)
        out.offset = data; out.nbytes = n; out.mat_class = cls; out.storage = (int32_t)type; out.ndim = (int32_t)ndim; out.compressed = 0;
        return 0;
    }

    int run(const char* name, gem_mat_array& out) {
        int64_t at = out.start;
        if (!out.bare) {
            if (len >= 8 && memcmp(p, "\x89HDF\r\n\x1a\n", 8) == 0) return refuse("an HDF5 file (MAT v7.3)", 0);
            if (len < 4) return refuse("truncated: no header", 0);
            if (!p[0] || !p[1] || !p[2] || !p[3]) return refuse("a zero among the first four bytes: a v4 MAT file", 0);
            if (len < 128) return refuse("truncated: the header has 128 bytes", 0);
            if (p[126] == 'M' && p[127] == 'I') return refuse("big-endian file", 126);
            if (p[126] != 'I' || p[127] != 'M') return refuse("no endian marker", 126);
            if (p[125] == 2) return refuse("version 0x0200: an HDF5 file (MAT v7.3)", 124);
            if (p[124] != 0 || p[125] != 1) return refuse("version is not 0x0100", 124);
            if (at == 0) at = 128;
            if (at < 128) return refuse("resume position inside the header", at);
        }
        bool found = false;
        gem_mat_array hit = out;
        while (at < len) {
            uint32_t type; int64_t data, n, next;
            if (!tag(at, len, type, data, n, next)) return GEM_MAT_UNSUPPORTED;
            if (type == MI_COMPRESSED) {
                // (loadmat keeps the LAST variable of a name: what a later compressed element holds is not known here)
                if (found) return refuse("a compressed element follows the variable", at);
                out.offset = data; out.nbytes = n; out.next = next; out.compressed = 1;
                out.mat_class = out.storage = out.ndim = 0;
                for (int k = 0; k < 4; ++k) out.dims[k] = 0;
                return 0;
            }
            if (type != MI_MATRIX) return refuse("a top-level element that is neither miMATRIX nor miCOMPRESSED", at);
            bool mine = false;
            gem_mat_array a = out;
            const int rc = matrix(data, data + n, name, a, mine);
            if (rc) return rc;
            if (mine) { found = true; hit = a; hit.next = next; }
            if (next <= at) return refuse("a data element of no length", at);
            at = next;
        }
        if (!found) { if (why.empty()) why = std::string("no variable called '") + name + "'"; return GEM_MAT_NOT_FOUND; }
        out = hit;
        return 0;
    }
};

int mat_scan(const void* h_image, int64_t len, const char* name, gem_mat_array* out, const char* who) {
    if (!h_image || len < 0 || !name || !out || out->start < 0 || out->start > len) { set_error(std::string(who) + ": bad argument"); return 1; }
    MatScanner s;
    s.p = static_cast<const uint8_t*>(h_image);
    s.len = len;
    gem_mat_array a = *out;
    const int rc = s.run(name, a);
    if (rc) { set_error(std::string(who) + ": " + s.why); return rc; }
    *out = a;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ the device side
struct MatArgs {
    HeatArgs h;                     // image, heat payload offsets, out [n][H][W][J], geometry
    const int64_t* depth_offsets;   // byte offset of every frame's depth payload in the image
    const int32_t* kinds;           // per frame: GEM_MAT_HEAT_F64 | GEM_MAT_DEPTH_F32
    double* depth;                  // [n][J]
    int tiles;                      // workgroups per frame
};

// The LDS transpose of heat_transpose_kernel (chunk_io.hip: tile_in / tile_out) with the payload type read from a per-frame table
// -- uniform per workgroup, so the choice costs one scalar branch -- and the frame's J depths converted by the frame's first
// workgroup.  1-D grid: frame = block / tiles.
template <int HC, int WC, int JC, int WTC>
__global__ __launch_bounds__(256) void mat_frames_kernel(MatArgs m) {
    extern __shared__ float tile[];
    const HeatArgs& a = m.h;
    const int W = WC ? WC : a.W, J = JC ? JC : a.J, WT = WTC ? WTC : a.TH;
    const int f = blockIdx.x / m.tiles, t = blockIdx.x - f * m.tiles;
    const int w0 = t * WT, wn = WTC ? WTC : min(WT, W - w0);
    const int kind = m.kinds[f];
    const int64_t payload = a.offsets[f];
    if (kind & GEM_MAT_HEAT_F64) tile_in<true, HC, WC, JC, WTC>(a, tile, payload, w0, wn);
    else tile_in<false, HC, WC, JC, WTC>(a, tile, payload, w0, wn);
    if (m.depth && t == 0 && (int)threadIdx.x < J) {          // (a recording without depth files: heat-maps only)
        const int64_t at = m.depth_offsets[f];
        m.depth[(int64_t)f * J + threadIdx.x] = (kind & GEM_MAT_DEPTH_F32) ? (double)__uint_as_float(word_at(a, at + 4 * threadIdx.x))      // widened exactly
                                                                            : double_at(a, at + 8 * threadIdx.x);
    }
    __syncthreads();
    tile_out<HC, WC, JC, WTC>(a, tile, f, w0, wn);
}

// est_global[f][j] = R_f . est_local[f][j] + t_f, every product and sum rounded on its own (no fused multiply-add: __dmul_rn /
// __dadd_rn are not contracted), summed left to right as `p @ R.T + t` does; err[f] = mean_j |gt - est_global|.  16 lanes per frame.
__global__ __launch_bounds__(256) void prepare_global_kernel(const double* __restrict__ local, const double* __restrict__ cams,
                                                             const double* __restrict__ gt, int64_t n, int J, double* __restrict__ out,
                                                             double* __restrict__ err) {
    const int64_t f = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int j = threadIdx.x & 15;
    double d = 0.0;
    if (f < n) {
        const double* M = cams + f * 16;
        for (int jj = j; jj < J; jj += 16) {
            const double* p = local + (f * J + jj) * 3;
            const double x = p[0], y = p[1], z = p[2];
            double dd = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double v = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, M[4 * r]), __dmul_rn(y, M[4 * r + 1])), __dmul_rn(z, M[4 * r + 2])), M[4 * r + 3]);
                out[(f * J + jj) * 3 + r] = v;
                if (gt) { const double e = __dadd_rn(gt[(f * J + jj) * 3 + r], -v); dd = __dadd_rn(dd, __dmul_rn(e, e)); }
            }
            d += sqrt(dd);
        }
    }
    for (int s = 8; s; s >>= 1) d += __shfl_xor(d, s, 16);
    if (f < n && j == 0 && err) err[f] = d / (double)J;
}

}  // namespace
}  // namespace gem

extern "C" {

int gem_mat_scan(const void* h_image, int64_t len, const char* name, gem_mat_array* out) {
    return mat_scan(h_image, len, name, out, "gem_mat_scan");
}

int gem_files_sizes(const char* const* paths, int64_t n, int64_t* sizes) {
    if (!paths || !sizes || n < 0) { set_error("gem_files_sizes: bad argument"); return 1; }
    for (int64_t i = 0; i < n; ++i) {
        struct stat st;
        if (!paths[i] || stat(paths[i], &st) != 0) { set_error(std::string("gem_files_sizes: ") + (paths[i] ? paths[i] : "(null)") + ": " + strerror(errno)); return 1; }
        sizes[i] = (int64_t)st.st_size;
    }
    return 0;
}

int gem_mat_read(const char* const* paths, int64_t n, const int64_t* at, const int64_t* sizes, const char* name, void* h_block,
                 int64_t block_bytes, gem_mat_array* out, int32_t* rc_out) {
    if (!paths || !at || !sizes || !name || !h_block || !out || !rc_out || n < 0) { set_error("gem_mat_read: bad argument"); return 1; }
    uint8_t* block = static_cast<uint8_t*>(h_block);
    for (int64_t i = 0; i < n; ++i) {
        if (at[i] < 0 || sizes[i] < 0 || at[i] > block_bytes || sizes[i] > block_bytes - at[i]) { set_error("gem_mat_read: a file's place lies outside the block"); return 1; }
        const int fd = open(paths[i], O_RDONLY | O_CLOEXEC);
        if (fd < 0) { set_error(std::string("gem_mat_read: ") + paths[i] + ": " + strerror(errno)); return 1; }
        const int64_t got = pread_all(fd, block + at[i], sizes[i], 0);
        close(fd);
        if (got != sizes[i]) { set_error(std::string("gem_mat_read: ") + paths[i] + ": short read (the file shrank)"); return 1; }
        memset(&out[i], 0, sizeof out[i]);
        rc_out[i] = mat_scan(block + at[i], sizes[i], name, &out[i], "gem_mat_read");
    }
    return 0;
}

int gem_mat_frames(const void* d_image, int64_t image_len, const int64_t* d_heat_offsets, const int64_t* d_depth_offsets,
                   const int32_t* d_kinds, int64_t n, int heat_h, int heat_w, int n_joints, float* d_heat, double* d_depth, void* stream) {
    if (n == 0) return 0;
    if (!d_image || !d_heat_offsets || !d_depth_offsets != !d_depth || !d_kinds || !d_heat || n < 0 || heat_h < 1 || heat_w < 1 ||
        n_joints < 1 || n_joints > 256 || image_len < 4) {
        set_error("gem_mat_frames: bad argument (at most 256 joints)"); return 1;
    }
    if (reinterpret_cast<uintptr_t>(d_image) & 3) { set_error("gem_mat_frames: the image must start on a 4-byte boundary"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_heat) & 15) { set_error("gem_mat_frames: the heat-map output must start on a 16-byte boundary"); return 1; }
    if ((int64_t)heat_h * heat_w * n_joints > (1ll << 30)) { set_error("gem_mat_frames: heat-maps too large"); return 1; }
    MatArgs m;
    m.h.image = static_cast<const uint32_t*>(d_image); m.h.offsets = d_heat_offsets; m.h.out = d_heat; m.h.image_len = (image_len + 3) & ~3ll;
    m.h.H = heat_h; m.h.W = heat_w; m.h.J = n_joints;
    m.depth_offsets = d_depth_offsets; m.kinds = d_kinds; m.depth = d_depth;
    int WT;
    const size_t lds = transpose_tile(heat_h, heat_w, n_joints, WT);
    if (!lds) { set_error("gem_mat_frames: a heat-map column of H * J floats does not fit the transposing tile"); return 1; }
    m.h.TH = WT;
    m.tiles = (heat_w + WT - 1) / WT;
    if (n * m.tiles > 0x7fffffffll) { set_error("gem_mat_frames: too many frames for one launch"); return 1; }
    const dim3 grid((unsigned)(n * m.tiles));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (heat_h == 64 && heat_w == 64 && n_joints == 15) hipLaunchKernelGGL((mat_frames_kernel<64, 64, 15, 8>), grid, dim3(256), lds, s, m);
    else hipLaunchKernelGGL((mat_frames_kernel<0, 0, 0, 0>), grid, dim3(256), lds, s, m);
    GEM_HIP(hipGetLastError());
    return 0;
}

int gem_prepare_global(const double* d_est_local, const double* d_cams, const double* d_gt, int64_t n_frames, int n_joints,
                       double* d_est_global, double* d_frame_error, void* stream) {
    if (n_frames == 0) return 0;
    if (!d_est_local || !d_cams || !d_est_global || n_frames < 0 || n_joints < 1 || (d_frame_error && !d_gt)) {
        set_error("gem_prepare_global: bad argument"); return 1;
    }
    const int64_t blocks = (n_frames + 15) / 16;
    if (blocks > 0x7fffffffll) { set_error("gem_prepare_global: too many frames for one launch"); return 1; }
    hipLaunchKernelGGL(prepare_global_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_est_local, d_cams,
                       d_gt, n_frames, n_joints, d_est_global, d_frame_error);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
