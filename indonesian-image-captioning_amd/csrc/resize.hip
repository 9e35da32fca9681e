// The first step of the inference path (reference inference.py:33-44 and utils/dataset.py:368-373): a
// decoded photograph H x W x C (uint8, interleaved, C = 1 or 3) -> `scipy.misc.imresize(img, (OH, OW))`, i.e.
// `PIL.Image.resize((OW, OH), BILINEAR)` on the uint8 image -> transpose(2, 0, 1), a grey image replicated to three
// planes.  One launch resizes a whole packed batch of images of different sizes and writes either the uint8 rows
// [N, 3, OH, OW] the dataset builder stores, or the normalised batch through the [3, 256] table of data.hip.
//
// Bit-exactness: Pillow's 8-bit resize (ImagingResampleHorizontal_8bpc, then ImagingResampleVertical_8bpc) is integer
// arithmetic on coefficient tables the host computes in double (scnattn.data.resize_taps): per pass
// clip8((2^21 + sum coeff * byte) >> 22), and the horizontal result is a uint8 before the vertical pass reads it.
// The kernel does exactly that in int32, so the bytes equal Pillow's.  An axis whose size does not change has no pass
// (Pillow skips it).
//
// Work shape: a workgroup of 192 threads owns RT = 8 output rows x CT = 64 output columns of one image; thread t owns
// column t / 3, channel t % 3 of all 8 rows.  It walks the input rows the tile's vertical bounds cover: for each it
// forms the horizontal pass of its own (column, channel) in a register, rounds it to a byte, and adds weight x byte
// into its 8 accumulators; the weights of a row for the 8 output rows (0 outside an output row's bounds) come from a
// table the workgroup fills in LDS for 32 input rows at a time.  Neighbouring lanes read neighbouring bytes of the
// interleaved source row.  Nothing is sized by the scale factor, so a 251-tap row and a 4000-row source run the same
// code.  The finished 8 x 64 x 3 bytes go through LDS once, so that the stores are the 16-value vector stores of
// data.hip whatever the output layout.
//
// Two table layouts share the kernel.  The bilinear entry point derives a table's row length from (in, out); the
// tap-table entry point (any filter of scnattn.data.resize_taps, Pillow's LANCZOS among them: support 3, negative
// weights) reads it from a header word in front of each table, and its host side checks every row of the host copy of
// the tables -- bounds, 24-bit weights, 32-bit sums -- before the launch, so the arithmetic below rests on a checked
// precondition instead of on one filter's shape.
#include <type_traits>
#include <vector>
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

constexpr int RT = 8;        // output rows per workgroup
constexpr int CT = 64;       // output columns per workgroup
constexpr int NT = CT * 3;   // threads: one per (column, channel)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ inline int axis_ksize(int in, int out) {      // 2 * ceil(max(in / out, 1)) + 1
    return 2 * (in > out ? (in + out - 1) / out : 1) + 1;
}
// int32 words of one axis table: xmin[out], n[out], coeff[out][ksize]; an unchanged axis has none
__host__ __device__ inline long axis_table_ints(int in, int out) {
    return in == out ? 0 : (long)out * (2 + axis_ksize(in, out));
}

__device__ __forceinline__ int clip8(int v) { return min(max(v >> 22, 0), 255); }

constexpr int ONE = 1 << 22;     // the weight 1.0
constexpr int KREG = 7;          // horizontal tables of up to 7 taps (a bilinear shrink by up to 3, a Lanczos up-scale)
                                 // live in registers
constexpr int KSIZE_MAX = 2 * 3 * SCNATTN_RESIZE_MAX_DIM + 1;      // header-word tables: support <= 3
constexpr int WR = 32;           // input rows per chunk of the vertical weight table in LDS

// The walk over the input rows [r0, r1) of one chunk by one thread: per row the horizontal pass of its (column,
// channel), rounded to a byte, then weight x byte into the RT accumulators.  wt[r - r0][j] is the weight of input row r
// in output row j of the tile, 0 outside that row's bounds: one broadcast LDS read per row and no branch.  Weights are
// below 2^23 in magnitude (bilinear: at most 2^22; header-word tables: checked on the host) and bytes at most 255, so
// the products are signed 24-bit multiplies (full rate, where a 32-bit one is not).
// The image is a buffer of exactly its bytes: a 32-bit lane offset per tap plus a scalar row offset, range-checked by
// the hardware on top of the clamps of the caller.
// KH > 0: at most KH horizontal taps, weights and byte offsets in registers, the KH loads of a row independent of each
// other (a tap past xn re-reads the last byte with weight 0).  KH == 0: any tap count, a loop.
template <int KH>
__device__ __forceinline__ void walk(__amdgpu_buffer_rsrc_t img, unsigned lane, unsigned row_bytes, int C, int xn,
                                     const int* __restrict__ kh, int one_tap, int r0, int r1, const int (*wt)[RT],
                                     int (&acc)[RT]) {
    constexpr int KN = KH > 0 ? KH : 1;
    int kreg[KN];
    unsigned koff[KN];
#pragma unroll
    for (int k = 0; k < KN; ++k) {
        kreg[k] = k < xn ? (kh ? kh[k] : one_tap) : 0;
        koff[k] = lane + max(min(k, xn - 1), 0) * C;
    }
    for (int r = r0; r < r1; ++r) {
        int ss = 1 << 21;
        if (KH > 0) {
            int b[KN];
#pragma unroll
            for (int k = 0; k < KN; ++k) b[k] = __builtin_amdgcn_raw_buffer_load_b8(img, koff[k], r * row_bytes, 0);
#pragma unroll
            for (int k = 0; k < KN; ++k) ss += __mul24(kreg[k], b[k]);
        } else {
            for (int k = 0; k < xn; ++k) {
                const int b = __builtin_amdgcn_raw_buffer_load_b8(img, lane + k * C, r * row_bytes, 0);
                ss += __mul24(kh ? kh[k] : one_tap, b);
            }
        }
        const int h = clip8(ss);
#pragma unroll
        for (int j = 0; j < RT; ++j) acc[j] += __mul24(wt[r - r0][j], h);
    }
}

template <typename T> struct Out;
template <> struct Out<uint8_t> {
    static __device__ __forceinline__ uint8_t cv(const float*, int v) { return (uint8_t)v; }
    static __device__ __forceinline__ void st16(uint8_t* p, const uint8_t (&v)[16]) {
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = (unsigned)v[4 * q] | ((unsigned)v[4 * q + 1] << 8) | ((unsigned)v[4 * q + 2] << 16) |
                   ((unsigned)v[4 * q + 3] << 24);
        *reinterpret_cast<u32x4*>(p) = o;
    }
};
template <> struct Out<float> {
    static __device__ __forceinline__ float cv(const float* tab, int v) { return tab[v]; }
    static __device__ __forceinline__ void st16(float* p, const float (&v)[16]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            reinterpret_cast<f32x4*>(p)[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    }
};
template <> struct Out<__bf16> {
    static __device__ __forceinline__ __bf16 cv(const float* tab, int v) { return (__bf16)tab[v]; }
    static __device__ __forceinline__ void st16(__bf16* p, const __bf16 (&v)[16]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = v[8 * q + j];
            reinterpret_cast<bf16x8*>(p)[q] = o;
        }
    }
};

// T: uint8_t (planar rows, no table), float or __bf16 (through lut[3][256]); nhwc: channels-last memory.
// `fast`: OW % 16 == 0 and dst 16-byte aligned, so every 16-value group of a row is one aligned vector store.
// HDR: every table is led by a header word holding its row length (scnattn_u8_resize_taps); otherwise the row length
// is the bilinear filter's (scnattn_u8_resize_bilinear).
template <typename T, bool HDR>
__global__ __launch_bounds__(NT) void u8_resize_kernel(const uint8_t* __restrict__ src, long src_bytes,
                                                        const scnattn_image_desc* __restrict__ desc,
                                                        const int* __restrict__ taps, long taps_len, int OH, int OW,
                                                        const float* __restrict__ lut, T* __restrict__ dst, int nhwc,
                                                        int fast) {
    __shared__ float tab[3 * 256];
    __shared__ uint8_t tile[RT][3][CT];
    __shared__ __attribute__((aligned(16))) int wt[WR][RT];
    const int t = threadIdx.x;
    const scnattn_image_desc d = desc[blockIdx.z];
    const int H = d.H, W = d.W, C = d.C;
    // the host refused bad descriptors before the launch; a device copy that differs must still not become a wild read
    if ((C != 1 && C != 3) || H < 1 || W < 1 || H > SCNATTN_RESIZE_MAX_DIM || W > SCNATTN_RESIZE_MAX_DIM ||
        d.offset < 0 || d.offset + (long)H * W * C > src_bytes)
        return;
    const bool hpass = W != OW, vpass = H != OH;
    int ksh = axis_ksize(W, OW), ksv = axis_ksize(H, OH);
    long tab_h = d.tab_h, tab_v = d.tab_v;
    if (HDR) {
        if ((hpass && (tab_h < 0 || tab_h >= taps_len)) || (vpass && (tab_v < 0 || tab_v >= taps_len))) return;
        ksh = hpass ? taps[tab_h++] : 1;
        ksv = vpass ? taps[tab_v++] : 1;
        if (ksh < 1 || ksv < 1 || ksh > KSIZE_MAX || ksv > KSIZE_MAX) return;
    }
    if ((hpass && (tab_h < 0 || tab_h + (long)OW * (2 + ksh) > taps_len)) ||
        (vpass && (tab_v < 0 || tab_v + (long)OH * (2 + ksv) > taps_len)))
        return;
    if (!std::is_same<T, uint8_t>::value) {
        for (int i = t; i < 768; i += NT) tab[i] = lut[i];
    }

    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * RT;
    const int x = x0 + t / 3, c = t - 3 * (t / 3);
    const bool live = x < OW;
    const uint8_t* img = src + d.offset;

    // this thread's horizontal taps: source bytes img[row][(xmin + k) * C + cs] with weights kh[k], k < xn.  An axis
    // without a pass is the one tap 2^22 (clip8(2^21 + 2^22 b) == b); a lane past OW keeps in-range addresses and has
    // no weight.
    const int cs = C == 3 ? c : 0;
    int xmin = (live && !hpass) ? x : 0, xn = 1;
    const int* kh = nullptr;
    if (hpass && live) {
        const int* th = taps + tab_h;
        xmin = min(max(th[x], 0), W - 1);
        xn = min(min(max(th[OW + x], 0), ksh), W - xmin);
        kh = th + 2 * OW + (long)x * ksh;
    }
    const int one_tap = (live && !hpass) ? ONE : 0;
    // the input rows the tile needs (uniform): output row y0 + j takes rows [ymin, ymin + yn) of its table, clamped to
    // the image; without a vertical pass it is row y0 + j itself
    const int* tv = vpass ? taps + tab_v : nullptr;
    int rlo = H, rhi = 0;
#pragma unroll
    for (int j = 0; j < RT; ++j) {
        const int y = min(y0 + j, OH - 1);      // rows past OH repeat the last one and are not stored
        const int ymin = vpass ? min(max(tv[y], 0), H - 1) : y;
        const int yn = vpass ? min(min(max(tv[OH + y], 0), ksv), H - ymin) : 1;
        rlo = min(rlo, ymin);
        rhi = max(rhi, ymin + yn);
    }

    int acc[RT];
#pragma unroll
    for (int j = 0; j < RT; ++j) acc[j] = 1 << 21;
    // the image as a buffer of exactly its H * W * C bytes (< 2^30)
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(img, (unsigned)(H * W * C));
    const unsigned row_bytes = W * C, lane = xmin * C + cs;
    for (int rc = rlo; rc < rhi; rc += WR) {
        // the vertical weights of rows [rc, rc + WR), masked by each output row's bounds, one entry per thread
        __syncthreads();
        for (int e = t; e < WR * RT; e += NT) {
            const int r = rc + e / RT, j = e % RT, y = min(y0 + j, OH - 1);
            int w = 0;
            if (vpass) {
                const int ymin = min(max(tv[y], 0), H - 1);
                const int yn = min(min(max(tv[OH + y], 0), ksv), H - ymin);
                if (r >= ymin && r < ymin + yn) w = tv[2 * OH + (long)y * ksv + (r - ymin)];
            } else if (r == y) {
                w = ONE;
            }
            wt[e / RT][j] = w;
        }
        __syncthreads();
        const int r1 = min(rc + WR, rhi);
        if (ksh <= KREG)
            walk<KREG>(rs, lane, row_bytes, C, xn, kh, one_tap, rc, r1, wt, acc);
        else
            walk<0>(rs, lane, row_bytes, C, xn, kh, one_tap, rc, r1, wt, acc);
    }
#pragma unroll
    for (int j = 0; j < RT; ++j) tile[j][c][t / 3] = (uint8_t)clip8(acc[j]);
    __syncthreads();

    const long n = blockIdx.z;
    const int rows = min(RT, OH - y0), cols = min(CT, OW - x0);
    if (fast) {
        // cols % 16 == 0.  96 groups of 16 consecutive values: planar (j, c, 16 columns) or interleaved (j, 16 of the
        // row's 192 values)
        if (t < 96) {
            T v[16];
            if (!nhwc) {
                const int j = t / 12, cc = (t / 4) % 3, g = t & 3;
                if (j < rows && g * 16 < cols) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[i] = Out<T>::cv(tab + cc * 256, tile[j][cc][g * 16 + i]);
                    Out<T>::st16(dst + ((n * 3 + cc) * OH + y0 + j) * OW + x0 + g * 16, v);
                }
            } else {
                const int j = t / 12, g = t - 12 * (t / 12);
                if (j < rows && g * 16 < cols * 3) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int e = g * 16 + i, px = e / 3, cc = e - 3 * px;
                        v[i] = Out<T>::cv(tab + cc * 256, tile[j][cc][px]);
                    }
                    Out<T>::st16(dst + ((n * OH + y0 + j) * OW + x0) * 3 + g * 16, v);
                }
            }
        }
    } else {
        for (int e = t; e < RT * NT; e += NT) {
            const int j = e / NT, q = e - j * NT;
            const int px = nhwc ? q / 3 : q % CT, cc = nhwc ? q % 3 : q / CT;
            if (j < rows && px < cols) {
                const long o = nhwc ? ((n * OH + y0 + j) * OW + x0 + px) * 3 + cc
                                    : ((n * 3 + cc) * OH + y0 + j) * OW + x0 + px;
                dst[o] = Out<T>::cv(tab + cc * 256, tile[j][cc][px]);
            }
        }
    }
}

}  // namespace

long resize_table_ints(int in, int out) {
    if (in < 1 || out < 1 || in > SCNATTN_RESIZE_MAX_DIM || out > SCNATTN_RESIZE_MAX_DIM) return -1;
    return axis_table_ints(in, out);
}

namespace {

#define RS_ARG(cond, msg)                                                                            \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            scn::set_error("%s:%d: invalid argument: %s: %s", __FILE__, __LINE__, name, msg);        \
            return -1;                                                                               \
        }                                                                                            \
    } while (0)

// One table of the header-word layout, on the host copy: header, extent, then every row's bounds and magnitudes.
int check_table(const char* name, const int* taps, long taps_len, long off, int in, int out, bool vertical) {
    const char* past = vertical ? "a vertical tap table runs past the tap buffer"
                                : "a horizontal tap table runs past the tap buffer";
    RS_ARG(off >= 0 && off < taps_len, past);
    const long ks = taps[off];
    RS_ARG(ks >= 1 && ks <= KSIZE_MAX, "a table's row length (its header word) is outside 1..6 * SCNATTN_RESIZE_MAX_DIM + 1");
    RS_ARG((long)out * (2 + ks) <= taps_len - off - 1, past);
    const int *xmin = taps + off + 1, *n = xmin + out, *coeff = n + out;
    for (int i = 0; i < out; ++i) {
        RS_ARG(n[i] >= 1 && n[i] <= ks, "a table row's tap count n is outside 1..ksize");
        RS_ARG(xmin[i] >= 0 && (long)xmin[i] + n[i] <= in, "a table row's taps leave the source axis");
        long sum = 0;
        for (int k = 0; k < n[i]; ++k) {
            const long c = coeff[i * ks + k], a = c < 0 ? -c : c;
            RS_ARG(a < (1L << 23), "a coefficient does not fit the 24-bit multiply (|coeff| >= 2^23)");
            sum += a;
        }
        RS_ARG(sum * 255 + (1L << 21) < (1L << 31), "a row's sum of |coeff| * 255 + 2^21 does not fit 32 bits");
    }
    return 0;
}

// hdr false: the bilinear layout (row length derived from (in, out), tables range-checked only, taps_host unused); hdr
// true: the header-word layout, every distinct table of the batch checked row by row on the host copy taps_host.
int resize_launch(const char* name, hipStream_t st, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                  const scnattn_image_desc* desc_dev, int N, bool hdr, const int* taps_host, const int* taps, long taps_len,
                  int OH, int OW, const float* lut, void* dst, int dst_kind, int channels_last) {
    RS_ARG(N >= 0 && N <= 65535, "the batch must hold 0..65535 images");
    RS_ARG(OH >= 1 && OW >= 1 && OH <= SCNATTN_RESIZE_MAX_DIM && OW <= SCNATTN_RESIZE_MAX_DIM,
           "target size outside 1..SCNATTN_RESIZE_MAX_DIM");
    RS_ARG(dst_kind >= 0 && dst_kind <= 2, "dst_kind must be 0 (uint8), 1 (fp32) or 2 (bf16)");
    RS_ARG(dst_kind != 0 || !channels_last, "the uint8 rows are planar");
    if (N == 0) return 0;
    RS_ARG(src && desc_host && desc_dev && dst && (lut || dst_kind == 0), "null pointer");
    RS_ARG(src_bytes > 0 && taps_len >= 0 && taps_len < (1L << 31) && (taps || taps_len == 0) &&
               (!hdr || taps_host || taps_len == 0),
           "bad buffer length");
    struct Seen { long off; int in, out; };
    std::vector<Seen> seen;      // header-word tables already checked
    for (int i = 0; i < N; ++i) {
        const scnattn_image_desc& d = desc_host[i];
        RS_ARG(d.C == 1 || d.C == 3, "an image must have 1 or 3 channels");
        RS_ARG(d.H >= 1 && d.W >= 1 && d.H <= SCNATTN_RESIZE_MAX_DIM && d.W <= SCNATTN_RESIZE_MAX_DIM,
               "image size outside 1..SCNATTN_RESIZE_MAX_DIM");
        RS_ARG(d.offset >= 0 && d.offset <= src_bytes && (long)d.H * d.W * d.C <= src_bytes - d.offset,
               "an image runs past the packed buffer");
        if (!hdr) {
            RS_ARG(d.W == OW || (d.tab_h >= 0 && d.tab_h + axis_table_ints(d.W, OW) <= taps_len),
                   "a horizontal tap table runs past the tap buffer");
            RS_ARG(d.H == OH || (d.tab_v >= 0 && d.tab_v + axis_table_ints(d.H, OH) <= taps_len),
                   "a vertical tap table runs past the tap buffer");
            continue;
        }
        for (int v = 0; v < 2; ++v) {
            const int in = v ? d.H : d.W, out = v ? OH : OW;
            const long off = v ? d.tab_v : d.tab_h;
            if (in == out) continue;
            bool done = false;
            for (const Seen& q : seen) done = done || (q.off == off && q.in == in && q.out == out);
            if (done) continue;
            SCN_TRY(check_table(name, taps_host, taps_len, off, in, out, v != 0));
            seen.push_back({off, in, out});
        }
    }
    const int fast = OW % 16 == 0 && aligned16(dst);
    const dim3 grid(cdiv(OW, CT), cdiv(OH, RT), N);
#define RS_LAUNCH(T, HDR, cl)                                                                                            \
    hipLaunchKernelGGL((u8_resize_kernel<T, HDR>), grid, dim3(NT), 0, st, src, src_bytes, desc_dev, taps, taps_len, OH, OW, \
                       lut, (T*)dst, cl, fast)
    if (dst_kind == 0) {
        if (hdr) RS_LAUNCH(uint8_t, true, 0); else RS_LAUNCH(uint8_t, false, 0);
    } else if (dst_kind == 1) {
        if (hdr) RS_LAUNCH(float, true, channels_last); else RS_LAUNCH(float, false, channels_last);
    } else {
        if (hdr) RS_LAUNCH(__bf16, true, channels_last); else RS_LAUNCH(__bf16, false, channels_last);
    }
#undef RS_LAUNCH
    SCN_LAUNCH_CHECK();
    return 0;
}
#undef RS_ARG

}  // namespace

int u8_resize_bilinear(hipStream_t st, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                       const scnattn_image_desc* desc_dev, int N, const int* taps, long taps_len, int OH, int OW,
                       const float* lut, void* dst, int dst_kind, int channels_last) {
    return resize_launch("u8_resize_bilinear", st, src, src_bytes, desc_host, desc_dev, N, false, nullptr, taps, taps_len,
                         OH, OW, lut, dst, dst_kind, channels_last);
}

int u8_resize_taps(hipStream_t st, const uint8_t* src, long src_bytes, const scnattn_image_desc* desc_host,
                   const scnattn_image_desc* desc_dev, int N, const int* taps_host, const int* taps_dev, long taps_len,
                   int OH, int OW, const float* lut, void* dst, int dst_kind, int channels_last) {
    return resize_launch("u8_resize_taps", st, src, src_bytes, desc_host, desc_dev, N, true, taps_host, taps_dev, taps_len,
                         OH, OW, lut, dst, dst_kind, channels_last);
}

}  // namespace scn
