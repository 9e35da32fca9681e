// Image augmentation inside the input assembly: random resized crop, horizontal flip and colour jitter in the
// launch that gathers the batch rows, so an augmented batch still costs no host work and no PCIe traffic.  The reference has
// no augmentation (it feeds `Normalize` only); the semantics are this project's own and are stated in include/scnattn.h.
//   u8_mean_grey        per source image the exact integer byte sums of R, G, B and
//                       grey = (0.299 SR + 0.587 SG + 0.114 SB) / (255 HW), formed in fp64 and rounded once to fp32.  One
//                       workgroup per image, 16-byte loads, integer sums (any order gives the same bits).
//   augment_draw        one thread per sample: the record (x0, y0, w, h, flip, bright, contr, sat) from eight uniforms
//                       u_k = (word_k >> 8) * 2^-24 of Philox4x32-10 with key (seed low, seed high) and counter
//                       (q, sid low, sid high, epoch), q = 0, 1.  Evaluated in fp64, each value rounded once to fp32; the
//                       record depends on (seed, epoch, sid) alone.
//   u8_gather_augment   one lane = 4 consecutive output pixels x 3 channels of one image; a workgroup = 256 such groups in
//                       row-major order (whole output rows at the real row size), the image's record read once (uniform
//                       over the workgroup).  Per pixel: mirror, half-pixel source coordinates clamped to the border,
//                       bilinear blend of four bytes read through the cache, /255, brightness, contrast about the SOURCE
//                       image's brightened mean grey, saturation, normalise, store 16 bytes (fp32) / 8 bytes (bf16) at a time.
//                       The coordinates are clamped whatever the record holds (a NaN becomes 0), so a hand-made table cannot
//                       make a lane read outside its image.
// Plain vector loads and stores; no atomics; no kernel waits for another workgroup; no inline assembly.
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include "../../include/scnattn.h"

namespace scn {

namespace {

struct Norm { float mean[3], std[3]; };

// ---- mean grey ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned byte_sum(unsigned w) { return (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24); }

__global__ __launch_bounds__(256) void u8_mean_grey_kernel(const uint8_t* __restrict__ src, long HW, int vec,
                                                            long long* __restrict__ sums, float* __restrict__ grey) {
    __shared__ unsigned long long red[3][256];
    const long i = blockIdx.x;
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* p = src + (i * 3 + c) * HW;
        unsigned long long s = 0;
        if (vec) {
            const long groups = HW / 16;
#pragma unroll 4
            for (long g = tid; g < groups; g += 256) {
                const u32x4 r = reinterpret_cast<const u32x4*>(p)[g];
                s += byte_sum(r[0]) + byte_sum(r[1]) + byte_sum(r[2]) + byte_sum(r[3]);
            }
        } else {
            for (long k = tid; k < HW; k += 256) s += p[k];
        }
        red[c][tid] = s;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double sr = (double)red[0][0], sg = (double)red[1][0], sb = (double)red[2][0];
        if (sums) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sums[i * 3 + c] = (long long)red[c][0];
        }
        grey[i] = (float)((0.299 * sr + 0.587 * sg + 0.114 * sb) / (255.0 * (double)HW));
    }
}

// ---- the draw ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void augment_draw_kernel(long n, const long long* __restrict__ sid, unsigned epoch, unsigned k0,
                                                            unsigned k1, scnattn_augment_config c, int H, int W,
                                                            float* __restrict__ params) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long s = (unsigned long long)sid[i];
    const u32q a = philox4x32_10(0u, (unsigned)s, (unsigned)(s >> 32), epoch, k0, k1);
    const u32q b = philox4x32_10(1u, (unsigned)s, (unsigned)(s >> 32), epoch, k0, k1);
    double u[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u[k] = (double)(a.w[k] >> 8) * 0x1p-24;
        u[4 + k] = (double)(b.w[k] >> 8) * 0x1p-24;
    }
    const double area = (double)c.scale_lo + u[0] * ((double)c.scale_hi - (double)c.scale_lo);
    const double ll = log((double)c.ratio_lo), lh = log((double)c.ratio_hi);
    const double r = exp(ll + u[1] * (lh - ll));
    const double w = fmin((double)W, (double)W * sqrt(area * r));
    const double h = fmin((double)H, (double)H * sqrt(area / r));
    float* o = params + 8 * i;
    o[0] = (float)(u[2] * ((double)W - w));
    o[1] = (float)(u[3] * ((double)H - h));
    o[2] = (float)w;
    o[3] = (float)h;
    o[4] = (float)u[4] < c.flip_p ? 1.f : 0.f;       // u has 24 bits: exact in fp32
    o[5] = (float)(1.0 + (2.0 * u[5] - 1.0) * (double)c.brightness);
    o[6] = (float)(1.0 + (2.0 * u[6] - 1.0) * (double)c.contrast);
    o[7] = (float)(1.0 + (2.0 * u[7] - 1.0) * (double)c.saturation);
}

// ---- gather + augment --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// four consecutive values: one 16-byte (fp32) / 8-byte (bf16) store
__device__ __forceinline__ void st4(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void st4(__bf16* p, const float* v) {
    *reinterpret_cast<u32x2*>(p) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(__bf16* p, float v) { *p = (__bf16)v; }

// source coordinate of output position o along an axis of `size` pixels: half-pixel convention, border clamp.  fmaxf / fminf
// return the other operand for a NaN, so the result is in [0, size - 1] whatever the record holds.
__device__ __forceinline__ void tap(float off, float k, int o, int size, int& i0, int& i1, float& f) {
    float s = off + ((float)o + 0.5f) * k - 0.5f;
    s = fminf(fmaxf(s, 0.f), (float)(size - 1));
    i0 = (int)s;                      // s >= 0: truncation is floor
    f = s - (float)i0;                // exact
    i1 = min(i0 + 1, size - 1);
}

template <typename T, bool NHWC, bool VEC>
__global__ __launch_bounds__(256) void u8_augment_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ idx,
                                                          long n_src, int H, int W, int bpi, const float* __restrict__ params,
                                                          const float* __restrict__ grey, Norm nm, T* __restrict__ dst) {
    const int n = blockIdx.x / bpi;                                   // uniform over the workgroup: scalar loads below
    const int gpr = (W + 3) >> 2;                                     // groups of 4 pixels per output row
    const int gid = (blockIdx.x - n * bpi) * 256 + threadIdx.x;
    if (gid >= H * gpr) return;
    const int oy = gid / gpr, ox0 = (gid - oy * gpr) * 4;
    const long HW = (long)H * W;
    long row = idx ? (long)idx[n] : (long)n;
    if (row < 0 || row >= n_src) row = -1;
    float o[3][4];
    if (row >= 0) {
        const float* p = params + 8 * (long)n;
        const float x0 = p[0], y0 = p[1], kx = p[2] / (float)W, ky = p[3] / (float)H;
        const bool flip = p[4] != 0.f;
        const float bright = p[5], contr = p[6], sat = p[7];
        const float m = grey ? fminf(1.f, bright * grey[row]) : 0.f;
        int iy, iy1;
        float fy;
        tap(y0, ky, oy, H, iy, iy1, fy);
        const uint8_t* r0 = src + row * 3 * HW + (long)iy * W;
        const uint8_t* r1 = src + row * 3 * HW + (long)iy1 * W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = min(ox0 + j, W - 1);                       // a lane past the row end repeats the last pixel (not stored)
            int ix, ix1;
            float fx;
            tap(x0, kx, flip ? W - 1 - ox : ox, W, ix, ix1, fx);
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float b00 = (float)r0[c * HW + ix], b01 = (float)r0[c * HW + ix1];
                const float b10 = (float)r1[c * HW + ix], b11 = (float)r1[c * HW + ix1];
                const float top = b00 + fx * (b01 - b00), bot = b10 + fx * (b11 - b10);
                float t = (top + fy * (bot - top)) / 255.f;
                t = clamp01(bright * t);
                if (grey) t = clamp01(contr * t + (1.f - contr) * m);
                v[c] = t;
            }
            const float g = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c][j] = (clamp01(sat * v[c] + (1.f - sat) * g) - nm.mean[c]) / nm.std[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[c][j] = __builtin_nanf("");       // an index outside the dataset poisons the row, visibly
    }
    if (NHWC) {
        T* q = dst + (((long)n * H + oy) * W + ox0) * 3;
        if (VEC) {
            float e[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) e[k] = o[k % 3][k / 3];
#pragma unroll
            for (int k = 0; k < 3; ++k) st4(q + 4 * k, e + 4 * k);
        } else {
            for (int j = 0; j < 4 && ox0 + j < W; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) st1(q + 3 * j + c, o[c][j]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T* q = dst + (((long)n * 3 + c) * H + oy) * W + ox0;
            if (VEC) {
                st4(q, o[c]);
            } else {
                for (int j = 0; j < 4 && ox0 + j < W; ++j) st1(q + j, o[c][j]);
            }
        }
    }
}

template <typename T>
int launch_augment(hipStream_t st, const uint8_t* src, long n_src, const long long* idx, long n_out, int H, int W,
                   const float* params, const float* grey, const Norm& nm, T* dst, int nhwc) {
    const long bpi = cdiv((long)H * ((W + 3) / 4), 256);
    SCN_ARG(n_out * bpi < (1L << 31), "u8_gather_augment: batch too large");
    const dim3 grid((unsigned)(n_out * bpi)), block(256);
    const bool vec = W % 4 == 0 && aligned16(dst);
#define SCN_AUG(NHWC_, VEC_)                                                                                              \
    hipLaunchKernelGGL((u8_augment_kernel<T, NHWC_, VEC_>), grid, block, 0, st, src, idx, n_src, H, W, (int)bpi, params, \
                       grey, nm, dst)
    if (nhwc) {
        if (vec) SCN_AUG(true, true); else SCN_AUG(true, false);
    } else {
        if (vec) SCN_AUG(false, true); else SCN_AUG(false, false);
    }
#undef SCN_AUG
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int u8_mean_grey(hipStream_t st, const uint8_t* src, long N, long HW, long long* sums, float* grey) {
    SCN_ARG(N >= 0 && N < (1L << 31) && HW > 0 && HW <= (1L << 28), "u8_mean_grey: bad shape");
    SCN_ARG((src && grey) || N == 0, "u8_mean_grey: null pointer");
    if (N == 0) return 0;
    hipLaunchKernelGGL(u8_mean_grey_kernel, dim3((unsigned)N), dim3(256), 0, st, src, HW, (int)(HW % 16 == 0 && aligned16(src)),
                       sums, grey);
    SCN_LAUNCH_CHECK();
    return 0;
}

int augment_draw(hipStream_t st, long n, const long long* sid, int epoch, unsigned long long seed,
                 const scnattn_augment_config* cfg, int H, int W, float* params) {
    SCN_ARG(n >= 0 && n < (1L << 31) && H > 0 && W > 0 && H <= 16384 && W <= 16384 && epoch >= 0, "augment_draw: bad shape");
    SCN_ARG(cfg && ((sid && params) || n == 0), "augment_draw: null pointer");
    const scnattn_augment_config& c = *cfg;
    SCN_ARG(c.scale_lo > 0.f && c.scale_lo <= c.scale_hi && c.scale_hi <= 1.f, "augment_draw: 0 < scale_lo <= scale_hi <= 1 is required");
    SCN_ARG(c.ratio_lo > 0.f && c.ratio_lo <= c.ratio_hi && c.ratio_hi < INFINITY, "augment_draw: 0 < ratio_lo <= ratio_hi is required");
    SCN_ARG(c.flip_p >= 0.f && c.flip_p <= 1.f, "augment_draw: flip_p must be in [0, 1]");
    SCN_ARG(c.brightness >= 0.f && c.brightness <= 1.f && c.contrast >= 0.f && c.contrast <= 1.f && c.saturation >= 0.f &&
                c.saturation <= 1.f, "augment_draw: colour strengths must be in [0, 1]");
    if (n == 0) return 0;
    hipLaunchKernelGGL(augment_draw_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, sid, (unsigned)epoch,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), c, H, W, params);
    SCN_LAUNCH_CHECK();
    return 0;
}

int u8_gather_augment(hipStream_t st, const uint8_t* src, long n_src, const long long* idx, long n_out, int H, int W,
                      const float* params, const float* grey, const float* mean, const float* std, void* dst, int dst_bf16,
                      int channels_last) {
    SCN_ARG(n_src > 0 && n_out >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "u8_gather_augment: bad shape");
    SCN_ARG(src && mean && std && ((params && dst) || n_out == 0), "u8_gather_augment: null pointer");
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c];
        nm.std[c] = std[c];
        SCN_ARG(std[c] != 0.f && std[c] == std[c] && mean[c] == mean[c], "u8_gather_augment: std must be non-zero, mean and std not NaN");
    }
    if (n_out == 0) return 0;
    if (dst_bf16)
        return launch_augment<__bf16>(st, src, n_src, idx, n_out, H, W, params, grey, nm, (__bf16*)dst, channels_last);
    return launch_augment<float>(st, src, n_src, idx, n_out, H, W, params, grey, nm, (float*)dst, channels_last);
}

}  // namespace scn
