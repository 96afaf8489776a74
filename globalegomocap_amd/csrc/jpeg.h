// Rendered frames as baseline JPEG images from the device: what `video=PATH` / `--video DIR` writes.  Included
// from errors.hip.
//
//   gem_jpeg_header   the 629 bytes in front of an image's entropy data: SOI, APP0, two DQT, SOF0, four DHT, DRI, SOS        (host)
//   gem_jpeg_bound    the most bytes one image's JPEG file can take                                                          (host)
//   gem_jpeg_encode   PNG scanline streams (gem_render_capsules / gem_render_camera) -> JPEG files or AVI `00dc` chunks
//
// Everything is integer arithmetic: the bytes are a function of the pixels and the quality alone.  Four launches:
//   jpeg_blocks_kernel    one workgroup per 8 MCUs of an MCU row: the pixels once through LDS (edge replication, JFIF colour), the
//                         8 x 8 DCT as two exact integer passes (int32 rows, int64 columns), quantisation (round half away from
//                         zero), zigzag; int16 coefficients [n,3,Hp/8,Wp/8,64] into the workspace (or straight into d_coef)
//   jpeg_segments_kernel  (count)  one workgroup per restart segment (one MCU row, at most 384 blocks, one thread each): bit counts
//                         from the coefficients, an exclusive scan, the bits deposited with atomic OR into a zeroed LDS buffer, the
//                         segment padded with 1-bits, its 0xFF bytes counted: the stuffed length goes into a table
//   jpeg_offsets_kernel   one workgroup: every segment's place in its image and every image's place in the output (d_offsets)
//   jpeg_segments_kernel  (write)  the same bits again, scattered with stuffing to their final place, with the headers, the RST
//                         markers, EOI and the chunk's pad byte; an image that does not fit below the capacity is left out whole
// The bit buffer lives in LDS and the segments are coded twice; the alternative, one pass into a global buffer sized for the worst
// case and a gather, costs 3 x 208 bytes per block of workspace (6j, "Where the bits wait").
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

namespace gem {

constexpr int JPG_MAX_WIDTH = 1024, JPG_MAX_HEIGHT = 16384;
constexpr int JPG_HEADER = 629;
constexpr int JPG_BLOCK_BITS = 22 + 63 * 26;              // DC: 11-bit code + 11 bits; AC: 16-bit code + 10 bits
constexpr int JPG_THREADS = 384;                          // one thread per block of the widest segment (3 * 1024 / 8)
constexpr int JPG_WAVES = JPG_THREADS / 64;
constexpr int JPG_MCUS = 8;                               // MCUs per workgroup of jpeg_blocks_kernel
constexpr int JPG_HUFF = 2 * 12 + 2 * 256;                // DC 0, DC 1, AC 0, AC 1: (code << 8) | length

static const unsigned char JPG_Q_LUMA[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char JPG_Q_CHROMA[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const unsigned char JPG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const unsigned char JPG_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char JPG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const unsigned char JPG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

struct JpegTables {
    int32_t dct[64];               // C[u][x]
    unsigned char zigzag[64];      // zigzag index -> natural index
    unsigned char quant[2][64];    // natural order
    uint32_t huff[JPG_HUFF];       // symbol -> (code << 8) | length; 0 where the table has no such symbol
};

inline void jpeg_zigzag(unsigned char* zz) {
    int k = 0;
    for (int d = 0; d < 15; ++d)
        for (int i = 0; i <= d; ++i) {
            const int y = (d & 1) ? i : d - i, x = d - y;          // odd diagonals with y ascending, even ones with x ascending
            if (y < 8 && x < 8) zz[k++] = (unsigned char)(y * 8 + x);
        }
}

inline void jpeg_canonical(const unsigned char* bits, const unsigned char* vals, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = (code++ << 8) | (uint32_t)len;
        code <<= 1;
    }
}

inline void jpeg_tables(int quality, JpegTables* t) {
    std::memset(t, 0, sizeof(*t));
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x)
            t->dct[u * 8 + x] = (int32_t)std::rint(16384.0 * ((u == 0 ? std::sqrt(0.5) : 1.0) / 2.0) * std::cos((2 * x + 1) * u * pi / 16.0));
    jpeg_zigzag(t->zigzag);
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            const int v = ((c ? JPG_Q_CHROMA[i] : JPG_Q_LUMA[i]) * s + 50) / 100;
            t->quant[c][i] = (unsigned char)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    jpeg_canonical(JPG_DC_BITS[0], JPG_DC_VALS, t->huff);
    jpeg_canonical(JPG_DC_BITS[1], JPG_DC_VALS, t->huff + 12);
    jpeg_canonical(JPG_AC_BITS[0], JPG_AC_VALS[0], t->huff + 24);
    jpeg_canonical(JPG_AC_BITS[1], JPG_AC_VALS[1], t->huff + 24 + 256);
}

inline int jpeg_write_header(int width, int height, const JpegTables& t, unsigned char* o) {
    int n = 0;
    auto put = [&](std::initializer_list<int> b) { for (int v : b) o[n++] = (unsigned char)v; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int k = 0; k < 64; ++k) o[n++] = t.quant[c][t.zigzag[k]];
    }
    put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c)
        for (int ac = 0; ac < 2; ++ac) {
            const unsigned char* bits = ac ? JPG_AC_BITS[c] : JPG_DC_BITS[c];
            const unsigned char* vals = ac ? JPG_AC_VALS[c] : JPG_DC_VALS;
            const int count = ac ? 162 : 12;
            put({0xFF, 0xC4, 0, 19 + count, (ac << 4) | c});
            for (int i = 0; i < 16; ++i) o[n++] = bits[i];
            for (int i = 0; i < count; ++i) o[n++] = vals[i];
        }
    const int mcus = (width + 7) / 8;
    put({0xFF, 0xDD, 0, 4, mcus >> 8, mcus & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0});
    return n;
}

// bytes of one restart segment of `blocks` blocks before stuffing, at most
inline int64_t jpeg_segment_raw(int64_t blocks) { return (blocks * JPG_BLOCK_BITS + 7) / 8; }

struct JpegBlocksArgs {
    const unsigned char* scan;
    int16_t* coef;              // [n,3,nby,nbx,64]
    int64_t in_stride;
    int W, H, nbx, nby;
    int32_t dct[64];
    unsigned char zigzag[64];
    unsigned char quant[2][64];
};

struct JpegSegmentsArgs {
    const int16_t* coef;
    int32_t* seg_len;           // [n,nby] stuffed bytes of every segment (count pass: written; write pass: unused)
    const int32_t* seg_off;     // [n,nby] the segment's first byte, counted from its image's first byte in the output
    const int32_t* jpeg_len;    // [n] bytes of every image's JPEG file
    const int64_t* offsets;     // [n+1]
    unsigned char* out;
    int64_t capacity;
    int nbx, nby, write, avi, buf_words;
    uint32_t huff[JPG_HUFF];
    unsigned char header[JPG_HEADER + 3];
};

struct JpegOffsetsArgs {
    const int32_t* seg_len;
    int32_t* seg_off;
    int32_t* jpeg_len;
    int64_t* offsets;
    int n, nby, avi;
};

__global__ __launch_bounds__(256) void jpeg_blocks_kernel(JpegBlocksArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jpeg_lds[];
    int32_t* dct = reinterpret_cast<int32_t*>(jpeg_lds);                           // [64]
    int32_t* rows = dct + 64;                                                      // [3][8 MCUs][8 y][8 u]: the row pass
    int16_t* samples = reinterpret_cast<int16_t*>(rows + 3 * JPG_MCUS * 64);       // [3][8 MCUs][8 y][8 x]
    unsigned char* zigzag = reinterpret_cast<unsigned char*>(samples + 3 * JPG_MCUS * 64);
    unsigned char* quant = zigzag + 64;                                            // [2][64]
    const int tid = threadIdx.x;
    const int bx0 = blockIdx.x * JPG_MCUS, by = blockIdx.y, img = blockIdx.z;
    const int nb = min(JPG_MCUS, a.nbx - bx0);
    if (tid < 64) { dct[tid] = a.dct[tid]; zigzag[tid] = a.zigzag[tid]; }
    if (tid < 128) quant[tid] = a.quant[tid >> 6][tid & 63];
    // the pixels, once: column and row clamped to the image (edge replication), JFIF colour in 16-bit fixed point
    const unsigned char* image = a.scan + (int64_t)img * a.in_stride;
    const int row_bytes = 1 + 3 * a.W;
    for (int q = tid; q < 8 * 8 * JPG_MCUS; q += 256) {
        const int y = q / (8 * JPG_MCUS), xl = q % (8 * JPG_MCUS), m = xl >> 3;
        if (m >= nb) continue;
        const int sx = min(bx0 * 8 + xl, a.W - 1), sy = min(by * 8 + y, a.H - 1);
        const unsigned char* p = image + (int64_t)sy * row_bytes + 1 + 3 * sx;
        const int R = p[0], G = p[1], B = p[2];
        const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        const int Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32768) >> 16;
        const int Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32768) >> 16;
        const int at = m * 64 + y * 8 + (xl & 7);
        samples[at] = (int16_t)(min(max(Y, 0), 255) - 128);
        samples[JPG_MCUS * 64 + at] = (int16_t)(min(max(Cb, 0), 255) - 128);
        samples[2 * JPG_MCUS * 64 + at] = (int16_t)(min(max(Cr, 0), 255) - 128);
    }
    __syncthreads();
    // rows: t[y][u] = sum_x C[u][x] p[y][x], below 2^23 in magnitude
    for (int o = tid; o < 3 * JPG_MCUS * 64; o += 256) {
        if (((o >> 6) & (JPG_MCUS - 1)) >= nb) continue;
        const int u = o & 7;
        const int16_t* p = samples + (o & ~7);
        int32_t acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += dct[u * 8 + x] * (int32_t)p[x];
        rows[o] = acc;
    }
    __syncthreads();
    // columns, exactly (below 2^40), quantisation and zigzag: thread -> zigzag position k of a block
    for (int o = tid; o < 3 * JPG_MCUS * 64; o += 256) {
        const int blk = o >> 6, k = o & 63, c = blk / JPG_MCUS, m = blk % JPG_MCUS;
        if (m >= nb) continue;
        const int nat = zigzag[k], v = nat >> 3, u = nat & 7;
        const int32_t* t = rows + blk * 64 + u;
        int64_t F = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) F += (int64_t)dct[v * 8 + y] * (int64_t)t[y * 8];
        const uint32_t q = quant[(c ? 64 : 0) + nat];
        const uint64_t mag = (uint64_t)(F < 0 ? -F : F);
        // (|F| + D / 2) / D with D = q << 28: the shift first, then a 32-bit division (floor of a floor)
        const uint32_t level = (uint32_t)((mag + ((uint64_t)q << 27)) >> 28) / q;
        a.coef[((((int64_t)img * 3 + c) * a.nby + by) * a.nbx + bx0 + m) * 64 + k] = (int16_t)(F < 0 ? -(int32_t)level : (int32_t)level);
    }
}

// `len` bits (1 .. 26) of v, MSB first, at bit `pos` of the big-endian words of `buf`
__device__ inline void jpeg_put(uint32_t* buf, int pos, uint32_t v, int len) {
    const uint64_t x = (uint64_t)v << (64 - (pos & 31) - len);
    atomicOr(&buf[pos >> 5], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&buf[(pos >> 5) + 1], (uint32_t)x);
}

__device__ inline int jpeg_category(int v) { return v ? 32 - __clz(v < 0 ? -v : v) : 0; }

// One block's symbols from its 64 coefficients (16-byte aligned) and the DC predictor: returns the block's bit count; EMIT deposits
// the bits from bit `pos` on.
template <bool EMIT>
__device__ inline int jpeg_code_block(const int16_t* coef, int pred, const uint32_t* dc, const uint32_t* ac, uint32_t* buf, int pos) {
    typedef uint32_t jpeg_u4 __attribute__((ext_vector_type(4)));
    const int start = pos;
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const jpeg_u4 w = reinterpret_cast<const jpeg_u4*>(coef)[g];
        const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v = (int16_t)(words[i >> 1] >> (16 * (i & 1)));
            uint32_t h;
            if (g == 0 && i == 0) {
                v -= pred;
                h = dc[jpeg_category(v)];
            } else {
                if (v == 0) { ++run; continue; }
                while (run >= 16) {          // ZRL, once per 16 zeros before a non-zero coefficient
                    const uint32_t z = ac[0xF0];
                    if (EMIT) jpeg_put(buf, pos, z >> 8, (int)(z & 255));
                    pos += (int)(z & 255);
                    run -= 16;
                }
                h = ac[(run << 4) | jpeg_category(v)];
                run = 0;
            }
            const int s = jpeg_category(v), len = (int)(h & 255) + s;
            const uint32_t mag = (uint32_t)(v > 0 ? v : v + (1 << s) - 1);
            if (EMIT) jpeg_put(buf, pos, ((h >> 8) << s) | mag, len);
            pos += len;
        }
    }
    if (run > 0) {                           // EOB: the last non-zero index is below 63
        const uint32_t e = ac[0];
        if (EMIT) jpeg_put(buf, pos, e >> 8, (int)(e & 255));
        pos += (int)(e & 255);
    }
    return pos - start;
}

// exclusive prefix of v over the workgroup's threads (wave scans by shuffles, the wave totals through `waves`); *total = the sum
__device__ inline int jpeg_block_scan(int v, int* waves, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) waves[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < JPG_WAVES; ++w) { const int t = waves[w]; if (w < wave) before += t; all += t; }
    __syncthreads();          // (`waves` may be written again at once)
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(JPG_THREADS) void jpeg_segments_kernel(JpegSegmentsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jpeg_lds[];
    uint32_t* huff = reinterpret_cast<uint32_t*>(jpeg_lds);                 // [JPG_HUFF]
    int* waves = reinterpret_cast<int*>(huff + JPG_HUFF);                   // [8]
    uint32_t* buf = reinterpret_cast<uint32_t*>(waves + 8);                 // [buf_words]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.x, img = blockIdx.y;
    const int64_t image_at = a.write ? a.offsets[img] : 0;
    if (a.write && a.offsets[img + 1] > a.capacity) return;          // an image that does not fit entirely is not written
    for (int i = tid; i < JPG_HUFF; i += JPG_THREADS) huff[i] = a.huff[i];
    __syncthreads();
    const int nblk = 3 * a.nbx;                                          // at most JPG_THREADS: one block per thread, MCU by MCU
    const int m = tid / 3, c = tid - 3 * m;
    const int16_t* coef = a.coef + ((((int64_t)img * 3 + c) * a.nby + seg) * a.nbx + m) * 64;
    const uint32_t* dc = huff + (c ? 12 : 0);
    const uint32_t* ac = huff + 24 + (c ? 256 : 0);
    const bool mine = tid < nblk;
    const int pred = mine && m > 0 ? coef[-64] : 0;                     // the block before it of the same component; 0 at the segment's start
    const int bits = mine ? jpeg_code_block<false>(coef, pred, dc, ac, nullptr, 0) : 0;
    int total_bits;
    const int pos = jpeg_block_scan(bits, waves, &total_bits);
    const int n_bytes = (total_bits + 7) >> 3;
    for (int i = tid; i < (n_bytes >> 2) + 2 && i < a.buf_words; i += JPG_THREADS) buf[i] = 0;
    __syncthreads();
    if (mine) jpeg_code_block<true>(coef, pred, dc, ac, buf, pos);
    if (tid == 0 && (total_bits & 7)) jpeg_put(buf, total_bits, (1u << (8 - (total_bits & 7))) - 1u, 8 - (total_bits & 7));
    __syncthreads();
    // stuffing: a zero byte behind every 0xFF.  JPG_THREADS bytes per round, their places from a ballot and the wave totals.
    unsigned char* dst = a.write ? a.out + image_at + a.seg_off[(int64_t)img * a.nby + seg] : nullptr;
    int stuffed = 0;
    for (int i0 = 0; i0 < n_bytes; i0 += JPG_THREADS) {
        const int i = i0 + tid;
        const uint32_t byte = i < n_bytes ? (buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
        const bool ff = byte == 255u;
        const unsigned long long vote = __ballot(ff);
        if (lane == 0) waves[wave] = __popcll(vote);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < JPG_WAVES; ++w) { const int t = waves[w]; if (w < wave) before += t; all += t; }
        __syncthreads();
        if (a.write && i < n_bytes) {
            unsigned char* o = dst + i + stuffed + before + __popcll(vote & ((1ull << lane) - 1ull));
            o[0] = (unsigned char)byte;
            if (ff) o[1] = 0;
        }
        stuffed += all;
    }
    const int seg_bytes = n_bytes + stuffed;
    if (!a.write) {
        if (tid == 0) a.seg_len[(int64_t)img * a.nby + seg] = seg_bytes;
        return;
    }
    unsigned char* image = a.out + image_at;
    const int head = a.avi ? 8 : 0, jpeg_len = a.jpeg_len[img];
    if (seg == 0) {                          // the chunk header and the frame header
        if (a.avi && tid < 8) image[tid] = tid < 4 ? (unsigned char)"00dc"[tid] : (unsigned char)((uint32_t)jpeg_len >> (8 * (tid - 4)));
        for (int i = tid; i < JPG_HEADER; i += JPG_THREADS) image[head + i] = a.header[i];
    }
    if (tid == 0) {
        dst[seg_bytes] = 0xFF;
        if (seg + 1 < a.nby) {
            dst[seg_bytes + 1] = (unsigned char)(0xD0 + (seg & 7));
        } else {                             // EOI, and the chunk's pad byte behind an odd length
            dst[seg_bytes + 1] = 0xD9;
            if (a.avi && (jpeg_len & 1)) dst[seg_bytes + 2] = 0;
        }
    }
}

__global__ __launch_bounds__(1024) void jpeg_offsets_kernel(JpegOffsetsArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = (a.avi ? 8 : 0) + JPG_HEADER;
    // a wave per image: every segment's first byte (a marker of two bytes behind every segment; behind the last it is EOI)
    for (int img = wave; img < a.n; img += 16) {
        int running = head;
        for (int s0 = 0; s0 < a.nby; s0 += 64) {
            const int s = s0 + lane;
            const int len = s < a.nby ? a.seg_len[(int64_t)img * a.nby + s] + 2 : 0;
            int incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (s < a.nby) a.seg_off[(int64_t)img * a.nby + s] = running + incl - len;
            running += __shfl(incl, 63, 64);
        }
        if (lane == 0) a.jpeg_len[img] = running - (a.avi ? 8 : 0);
    }
    __syncthreads();
    if (wave != 0) return;
    int64_t running = 0;
    for (int i0 = 0; i0 < a.n; i0 += 64) {
        const int i = i0 + lane;
        int64_t len = 0;
        if (i < a.n) {
            const int64_t jpeg = a.jpeg_len[i];
            len = a.avi ? 8 + jpeg + (jpeg & 1) : jpeg;
        }
        int64_t incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (i < a.n) a.offsets[i] = running + incl - len;
        running += __shfl(incl, 63, 64);
    }
    if (lane == 0) a.offsets[a.n] = running;
}

inline int64_t jpeg_bound(int width, int height) {
    const int64_t nbx = (width + 7) / 8, nby = (height + 7) / 8;
    return JPG_HEADER + nby * (2 * jpeg_segment_raw(3 * nbx) + 2);
}

}  // namespace gem

extern "C" {

int gem_jpeg_header(int width, int height, int quality, void* buf, int64_t cap) {
    using namespace gem;
    if (width < 1 || width > JPG_MAX_WIDTH) { set_error("gem_jpeg_header: width must be 1 .. 1024"); return -1; }
    if (height < 1 || height > JPG_MAX_HEIGHT) { set_error("gem_jpeg_header: height must be 1 .. 16384"); return -1; }
    if (quality < 1 || quality > 100) { set_error("gem_jpeg_header: quality must be 1 .. 100"); return -1; }
    if (!buf || cap < JPG_HEADER) { set_error("gem_jpeg_header: the buffer must hold 629 bytes"); return -1; }
    JpegTables t;
    jpeg_tables(quality, &t);
    return jpeg_write_header(width, height, t, static_cast<unsigned char*>(buf));
}

int64_t gem_jpeg_bound(int width, int height) {
    using namespace gem;
    if (width < 1 || width > JPG_MAX_WIDTH || height < 1 || height > JPG_MAX_HEIGHT) {
        set_error("gem_jpeg_bound: width must be 1 .. 1024 and height 1 .. 16384"); return -1;
    }
    return jpeg_bound(width, height);
}

int gem_jpeg_encode(gem_handle* h, const void* d_scan, int n_images, int width, int height, int64_t in_stride, int quality, int avi_chunks,
                    void* d_out, int64_t out_capacity, int64_t* d_offsets, int16_t* d_coef, void* stream) {
    using namespace gem;
    if (!h) { set_error("gem_jpeg_encode: null handle"); return 1; }
    if (width < 1 || width > JPG_MAX_WIDTH) { set_error("gem_jpeg_encode: width must be 1 .. 1024"); return 1; }
    if (height < 1 || height > JPG_MAX_HEIGHT) { set_error("gem_jpeg_encode: height must be 1 .. 16384"); return 1; }
    if (quality < 1 || quality > 100) { set_error("gem_jpeg_encode: quality must be 1 .. 100"); return 1; }
    if (n_images < 0 || n_images > 65535) { set_error("gem_jpeg_encode: between 0 and 65535 images per call"); return 1; }
    if (in_stride < (int64_t)height * (1 + 3 * (int64_t)width)) {
        set_error("gem_jpeg_encode: in_stride must be at least the image's bytes, H (1 + 3 W)"); return 1;
    }
    if (out_capacity < 0) { set_error("gem_jpeg_encode: out_capacity < 0"); return 1; }
    if (reinterpret_cast<uintptr_t>(d_coef) % 16) { set_error("gem_jpeg_encode: d_coef must be 16-byte aligned"); return 1; }
    if (n_images > 0 && (!d_scan || !d_out || !d_offsets)) { set_error("gem_jpeg_encode: null argument"); return 1; }
    GEM_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_images == 0) {
        if (d_offsets) GEM_HIP(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));
        return 0;
    }
    const int nbx = (width + 7) / 8, nby = (height + 7) / 8;
    // the workspace: the coefficients unless the caller keeps them, then per segment its length and its place, per image its length
    const int64_t coef_bytes = d_coef ? 0 : (int64_t)n_images * 3 * nby * nbx * 128;
    const int64_t table = ((int64_t)n_images * nby * 4 + 15) / 16 * 16, lens = ((int64_t)n_images * 4 + 15) / 16 * 16;
    if (post_scratch(h, (size_t)((coef_bytes + 2 * table + lens) / 8))) return 1;
    unsigned char* work = reinterpret_cast<unsigned char*>(h->post_work);
    int16_t* coef = d_coef ? d_coef : reinterpret_cast<int16_t*>(work);
    int32_t* seg_len = reinterpret_cast<int32_t*>(work + coef_bytes);
    int32_t* seg_off = reinterpret_cast<int32_t*>(work + coef_bytes + table);
    int32_t* jpeg_len = reinterpret_cast<int32_t*>(work + coef_bytes + 2 * table);

    JpegTables t;
    jpeg_tables(quality, &t);
    JpegBlocksArgs b;
    b.scan = static_cast<const unsigned char*>(d_scan); b.coef = coef; b.in_stride = in_stride;
    b.W = width; b.H = height; b.nbx = nbx; b.nby = nby;
    std::memcpy(b.dct, t.dct, sizeof(b.dct)); std::memcpy(b.zigzag, t.zigzag, sizeof(b.zigzag)); std::memcpy(b.quant, t.quant, sizeof(b.quant));
    const size_t blocks_lds = 64 * 4 + 3 * JPG_MCUS * 64 * 4 + 3 * JPG_MCUS * 64 * 2 + 64 + 128;
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)((nbx + JPG_MCUS - 1) / JPG_MCUS), (unsigned)nby, (unsigned)n_images), dim3(256),
                       blocks_lds, s, b);
    GEM_HIP(hipGetLastError());

    JpegSegmentsArgs g;
    std::memset(&g, 0, sizeof(g));
    g.coef = coef; g.seg_len = seg_len; g.seg_off = seg_off; g.jpeg_len = jpeg_len; g.offsets = d_offsets;
    g.out = static_cast<unsigned char*>(d_out); g.capacity = out_capacity; g.nbx = nbx; g.nby = nby; g.avi = avi_chunks ? 1 : 0;
    g.buf_words = (int)(jpeg_segment_raw(3 * nbx) / 4 + 3);          // (two words of slack: the zeroing and a symbol's second word)
    std::memcpy(g.huff, t.huff, sizeof(g.huff));
    jpeg_write_header(width, height, t, g.header);
    const size_t seg_lds = (size_t)(JPG_HUFF + 8 + g.buf_words) * 4;
    static PerDeviceOnce once;
    if (once.need(h->cfg.device))
        GEM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(jpeg_segments_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    g.write = 0;
    hipLaunchKernelGGL(jpeg_segments_kernel, dim3((unsigned)nby, (unsigned)n_images), dim3(JPG_THREADS), seg_lds, s, g);
    GEM_HIP(hipGetLastError());

    JpegOffsetsArgs o;
    o.seg_len = seg_len; o.seg_off = seg_off; o.jpeg_len = jpeg_len; o.offsets = d_offsets; o.n = n_images; o.nby = nby; o.avi = g.avi;
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(1024), 0, s, o);
    GEM_HIP(hipGetLastError());

    g.write = 1;
    hipLaunchKernelGGL(jpeg_segments_kernel, dim3((unsigned)nby, (unsigned)n_images), dim3(JPG_THREADS), seg_lds, s, g);
    GEM_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
