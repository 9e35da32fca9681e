// The last step of the reference's inference script (utils/vizualize.py:11-51, `visualize_att`): per word, the word's
// h x w attention map blown up to the photograph's size and smoothed -- `skimage.transform.pyramid_expand(alpha,
// upscale=24, sigma=8)`, defined here as `scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True)` followed by
// `gaussian_filter(sigma, mode='reflect', truncate=4)` -- and laid over the photograph.  Zoom and Gaussian are linear and
// separable, so the whole thing is S = Mv . a . Mh^T with one small operator per axis that the host builds in fp64
// (scnattn.viz.expand_operator) and uploads as fp32; its entries are >= 0 and its rows sum to 1.
//
// Fixed order, fp32, one fused multiply-add per term:
//   U[i][X] = sum_j a[i][j] * Mh[X][j]   (j ascending),      S[Y][X] = sum_i Mv[Y][i] * U[i][X]   (i ascending).
// A map whose entries are all equal is returned as that value: the rows of the operators sum to one, so that is its
// exact result, and its overlay is the dimmed photograph instead of rounding noise stretched to full contrast.
//
// Work shape: a workgroup of 256 threads owns one map and a strip of SR = 16 output rows; the map, the strip's rows of
// Mv and all of Mh (transposed, so that neighbouring lanes read neighbouring words) sit in LDS; a thread owns a column X
// and keeps the strip's 16 sums in registers.  The expand launch leaves min / max of its strip (and, if asked, the fp32
// maps); the overlay launch reduces the strips' partials in a fixed order, takes S -- read back from the stored maps, or
// RECOMPUTED with the same inlined code: the same bits either way, so (S - lo) / (hi - lo) cannot leave [0, 1] -- blends,
// and stores the strip's bytes (one contiguous range of the output) 16 per lane from LDS.  Reading back measured 0.27 ms
// against 0.34 ms recomputing for 384 maps of 336 x 336 (profiles/overlay_bench.txt): the sums of a strip, dense along
// the row, cost more than the 450 KB round trip per map, so scnattn.viz stores the maps by default.  No atomics; plain vector
// stores only.
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {

namespace {

constexpr int SR = 16;       // output rows per workgroup
constexpr int NT = 256;      // threads per workgroup
constexpr int LDS_MAX = 65536 - 256;     // dynamic LDS; the kernels keep up to 160 bytes of their own

__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }
// floats of LDS in front of the byte tile: a[h][w], mv[SR][h], mh[w][OW]
__host__ __device__ inline int lds_floats(int h, int w, int OW) { return pad4(h * w) + pad4(SR * h) + pad4(OW * w); }

// Fills the three LDS tables of (map m, strip at Y0) and act[i] = whether any of the strip's rows of Mv has a non-zero
// entry for map row i; returns whether the map is flat (all entries equal), uniformly.
__device__ __forceinline__ bool load_strip(const float* __restrict__ am, const float* __restrict__ Mv,
                                           const float* __restrict__ Mh, int h, int w, int OH, int OW, int Y0, float* a,
                                           float* mv, float* mh, int* act) {
    const int t = threadIdx.x;
    const float a0 = am[0];
    int same = 1;
    for (int e = t; e < h * w; e += NT) {
        const float v = am[e];
        a[e] = v;
        same &= v == a0;
    }
    for (int e = t; e < SR * h; e += NT) {
        const int r = e / h, i = e - r * h;
        mv[e] = Y0 + r < OH ? Mv[(long)(Y0 + r) * h + i] : 0.f;      // rows past OH are not stored
    }
    for (int e = t; e < OW * w; e += NT) {
        const int X = e / w, j = e - X * w;
        mh[j * OW + X] = Mh[e];
    }
    const bool flat = __syncthreads_and(same) != 0;
    if (t < h) {
        int any = 0;
        for (int r = 0; r < SR; ++r) any |= mv[r * h + t] != 0.f;
        act[t] = any;
    }
    __syncthreads();
    return flat;
}

// The strip's SR values of column X, in the documented order.  A map row that no row of the strip weighs (the operators
// are banded: the Gaussian reaches 32 of 336 rows) is skipped: its terms are exact zeros, the bits do not change.
__device__ __forceinline__ void strip_column(const float* a, const float* mv, const float* mh, const int* act, int h, int w,
                                             int OW, int X, bool flat, float (&acc)[SR]) {
#pragma unroll
    for (int r = 0; r < SR; ++r) acc[r] = flat ? a[0] : 0.f;
    if (flat) return;
    for (int i = 0; i < h; ++i) {
        if (!act[i]) continue;
        float u = 0.f;
        for (int j = 0; j < w; ++j) u = __fmaf_rn(a[i * w + j], mh[j * OW + X], u);
#pragma unroll
        for (int r = 0; r < SR; ++r) acc[r] = __fmaf_rn(mv[r * h + i], u, acc[r]);
    }
}

__global__ __launch_bounds__(NT) void attn_expand_kernel(const float* __restrict__ alphas, int h, int w,
                                                          const float* __restrict__ Mv, const float* __restrict__ Mh,
                                                          int OH, int OW, float* __restrict__ S,
                                                          float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[2][NT / 64];
    __shared__ int act[SCNATTN_OVERLAY_MAX_MAP];
    float *a = smem, *mv = a + pad4(h * w), *mh = mv + pad4(SR * h);
    const int t = threadIdx.x, strip = blockIdx.x, Y0 = strip * SR;
    const long m = blockIdx.y;
    const bool flat = load_strip(alphas + m * h * w, Mv, Mh, h, w, OH, OW, Y0, a, mv, mh, act);
    const int rows = min(SR, OH - Y0);
    float lo = INFINITY, hi = -INFINITY;
    for (int X = t; X < OW; X += NT) {
        float acc[SR];
        strip_column(a, mv, mh, act, h, w, OW, X, flat, acc);
#pragma unroll
        for (int r = 0; r < SR; ++r) {
            if (r < rows) {
                lo = fminf(lo, acc[r]);
                hi = fmaxf(hi, acc[r]);
                if (S) S[(m * OH + Y0 + r) * OW + X] = acc[r];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((t & 63) == 0) {
        red[0][t >> 6] = lo;
        red[1][t >> 6] = hi;
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < NT / 64; ++k) {
            lo = fminf(lo, red[0][k]);
            hi = fmaxf(hi, red[1][k]);
        }
        partial[(m * gridDim.x + strip) * 2] = lo;
        partial[(m * gridDim.x + strip) * 2 + 1] = hi;
    }
}

// {lo, hi} of map m from its strips' partials, strips ascending
__device__ __forceinline__ void reduce_strips(const float* __restrict__ partial, long m, int strips, float& lo, float& hi) {
    lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < strips; ++k) {
        lo = fminf(lo, partial[(m * strips + k) * 2]);
        hi = fmaxf(hi, partial[(m * strips + k) * 2 + 1]);
    }
}

__global__ __launch_bounds__(NT) void attn_lohi_kernel(const float* __restrict__ partial, int n_maps, int strips,
                                                        float* __restrict__ lohi) {
    const long m = (long)blockIdx.x * NT + threadIdx.x;
    if (m >= n_maps) return;
    float lo, hi;
    reduce_strips(partial, m, strips, lo, hi);
    lohi[2 * m] = lo;
    lohi[2 * m + 1] = hi;
}

// `fast`: OW * 3 % 16 == 0 and out 16-byte aligned, so the strip's bytes are whole aligned 16-byte groups.
__global__ __launch_bounds__(NT) void attn_overlay_kernel(const float* __restrict__ alphas, int h, int w,
                                                           const float* __restrict__ Mv, const float* __restrict__ Mh,
                                                           int OH, int OW, const float* __restrict__ S,
                                                           const float* __restrict__ partial,
                                                           const uint8_t* __restrict__ img, int n_img,
                                                           const int* __restrict__ img_index,
                                                           const float* __restrict__ beta, uint8_t* __restrict__ out,
                                                           int fast) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int act[SCNATTN_OVERLAY_MAX_MAP];
    float *a = smem, *mv = a + pad4(h * w), *mh = mv + pad4(SR * h);
    uint8_t* tile = reinterpret_cast<uint8_t*>(mh + pad4(OW * w));      // [SR][OW][3]
    const int t = threadIdx.x, strip = blockIdx.x, Y0 = strip * SR;
    const long m = blockIdx.y;
    // S given: the maps the expand launch stored are read back; otherwise they are recomputed here (the same bits)
    const bool flat = S ? false : load_strip(alphas + m * h * w, Mv, Mh, h, w, OH, OW, Y0, a, mv, mh, act);
    const int rows = min(SR, OH - Y0);
    float lo, hi;
    reduce_strips(partial, m, gridDim.x, lo, hi);
    const bool ramp = hi > lo;
    const float span = hi - lo, b = beta[m], keep = 1.f - b, b255 = __fmul_rn(b, 255.f);
    // the host refused an index out of range; a device copy that differs must still not become a wild read
    const long im = min(max(img_index[m], 0), n_img - 1);
    const uint8_t* photo = img + im * 3 * OH * OW;
    for (int X = t; X < OW; X += NT) {
        float acc[SR];
        if (S) {
#pragma unroll
            for (int r = 0; r < SR; ++r) acc[r] = r < rows ? S[(m * OH + Y0 + r) * OW + X] : 0.f;
        } else {
            strip_column(a, mv, mh, act, h, w, OW, X, flat, acc);
        }
#pragma unroll
        for (int r = 0; r < SR; ++r) {
            if (r < rows) {
                const float nrm = ramp ? fminf(fmaxf(__fdiv_rn(acc[r] - lo, span), 0.f), 1.f) : 0.f;
                const float grey = __fmul_rn(b255, nrm);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float p = (float)photo[((long)c * OH + Y0 + r) * OW + X];
                    const float v = __fadd_rn(__fmul_rn(keep, p), grey);
                    tile[(r * OW + X) * 3 + c] = (uint8_t)min(max((int)(v + 0.5f), 0), 255);
                }
            }
        }
    }
    __syncthreads();
    const long base = (m * OH + Y0) * OW * 3;
    const int nbytes = rows * OW * 3;
    if (fast) {
        for (int q = t; q < nbytes / 16; q += NT)
            *reinterpret_cast<u32x4*>(out + base + 16 * q) = *reinterpret_cast<const u32x4*>(tile + 16 * q);
    } else {
        for (int q = t; q < nbytes; q += NT) out[base + q] = tile[q];
    }
}

int check_shape(const char* name, int n_maps, int h, int w, int OH, int OW, size_t lds) {
#define OV_ARG(cond, msg)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            scn::set_error("%s:%d: invalid argument: %s: %s", __FILE__, __LINE__, name, msg);      \
            return -1;                                                                             \
        }                                                                                          \
    } while (0)
    OV_ARG(n_maps >= 0 && n_maps <= 65535, "the call must hold 0..65535 maps");
    OV_ARG(h >= 1 && w >= 1 && h <= SCNATTN_OVERLAY_MAX_MAP && w <= SCNATTN_OVERLAY_MAX_MAP,
           "map size outside 1..SCNATTN_OVERLAY_MAX_MAP");
    OV_ARG(OH >= 1 && OW >= 1 && OH <= SCNATTN_OVERLAY_MAX_OUT && OW <= SCNATTN_OVERLAY_MAX_OUT,
           "output size outside 1..SCNATTN_OVERLAY_MAX_OUT");
    OV_ARG(lds <= (size_t)LDS_MAX, "the map, the operators and the byte tile of a strip exceed the LDS budget (see SCNATTN_OVERLAY_MAX_OUT)");
#undef OV_ARG
    return 0;
}

}  // namespace

int attn_strips(int OH) { return OH >= 1 && OH <= SCNATTN_OVERLAY_MAX_OUT ? cdiv(OH, SR) : -1; }

int attn_expand(hipStream_t st, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh, int OH,
                int OW, float* S, float* lohi, float* partial) {
    const size_t lds = h >= 1 && w >= 1 && OW >= 1 ? sizeof(float) * (size_t)lds_floats(h, w, OW) : 0;
    SCN_TRY(check_shape("attn_expand", n_maps, h, w, OH, OW, lds));
    if (n_maps == 0) return 0;
    SCN_ARG(alphas && Mv && Mh && partial, "attn_expand: null pointer");
    const int strips = cdiv(OH, SR);
    hipLaunchKernelGGL(attn_expand_kernel, dim3(strips, n_maps), dim3(NT), lds, st, alphas, h, w, Mv, Mh, OH, OW, S,
                       partial);
    SCN_LAUNCH_CHECK();
    if (lohi) {
        hipLaunchKernelGGL(attn_lohi_kernel, dim3(cdiv(n_maps, NT)), dim3(NT), 0, st, partial, n_maps, strips, lohi);
        SCN_LAUNCH_CHECK();
    }
    return 0;
}

int attn_overlay(hipStream_t st, const float* alphas, int n_maps, int h, int w, const float* Mv, const float* Mh, int OH,
                 int OW, const float* S, const float* partial, const uint8_t* img, int n_img, const int* idx_host,
                 const int* idx_dev, const float* beta, uint8_t* out) {
    const size_t lds = h >= 1 && w >= 1 && OW >= 1 ? sizeof(float) * (size_t)lds_floats(h, w, OW) + (size_t)SR * OW * 3 : 0;
    SCN_TRY(check_shape("attn_overlay", n_maps, h, w, OH, OW, lds));
    SCN_ARG(n_img >= 1 && (long)n_img * 3 * OH * OW < (1L << 40), "attn_overlay: the call needs at least one photograph");
    if (n_maps == 0) return 0;
    SCN_ARG(alphas && Mv && Mh && partial && img && idx_host && idx_dev && beta && out, "attn_overlay: null pointer");
    for (int m = 0; m < n_maps; ++m)
        SCN_ARG(idx_host[m] >= 0 && idx_host[m] < n_img, "attn_overlay: an img_index is outside 0..n_img-1");
    const int fast = (OW * 3) % 16 == 0 && aligned16(out);
    hipLaunchKernelGGL(attn_overlay_kernel, dim3(cdiv(OH, SR), n_maps), dim3(NT), lds, st, alphas, h, w, Mv, Mh, OH, OW,
                       S, partial, img, n_img, idx_dev, beta, out, fast);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace scn
