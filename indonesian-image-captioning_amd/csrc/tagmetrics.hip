// Tagger evaluation over tag probabilities: per-image and per-tag average precision in the tie-invariant counting form,
// hits@k, tp / fp / fn per threshold and tag, and the summary vector.  Definitions and layouts: include/scnattn.h.
//
// AP needs no sort: for a positive i, N(i) = #{j : s_j >= s_i} and TP(i) = #{j positive : s_j >= s_i} are plain counts, exact
// integers whatever the order of ties, and terms are needed at the positives only (about 1 % of a tagger's targets).
//   tag_rows_kernel      two kinds of workgroup in one launch.  ROW workgroups: one wave64 per image (4 images), its row of
//                        S <= 4096 scores in registers (element j * 64 + lane in register j); positives are enumerated in
//                        index order by ballot, and for each one every lane compares its slice: a compare IS a ballot, so N,
//                        TP and the rank for hits@k are population counts on the scalar unit, with no cross-lane traffic.
//                        TRANSPOSE workgroups: 16 images x 256 tags each into the tag-major store through LDS: reads run
//                        along tags, writes along images, sixteen loads in flight per thread, one barrier.
//   tag_cols_kernel      one workgroup per tag over its n stored entries: one pass for npos and the threshold counts, then the
//                        positives are compacted (in index order) into LDS, up to 512 at a time, and counted eight at a time
//                        against the whole column.
//   tag_finalize_kernel  one workgroup: integer totals, and every floating-point mean summed in index order by one thread.
// Every floating-point sum has one fixed order and there is no floating-point atomic, so results are the same bits from run to
// run and however the same images, in the same order, are split into batches (a row's values depend on its row alone, a
// column's on the store alone).  The only atomics are integer adds in LDS.
#include "../../include/scnattn.h"
#include "common.h"
#include "kernels.h"

namespace scn {
namespace {

constexpr int TG_NT = 256;                         // threads of every workgroup here
constexpr int TG_TILE = 16;                        // images of one transpose workgroup (64 bytes of a store row)
constexpr int TG_TAGS = 256;                       // tags of one transpose workgroup
constexpr int TG_LD = TG_TAGS + 2;                 // LDS row of the tile: 2 * img + tag is a distinct bank per half wave
constexpr int TG_MAXK = SCNATTN_TAG_MAX_K;
constexpr int TG_MAXT = SCNATTN_TAG_MAX_THRESHOLDS;
constexpr int TG_PLIST = 512;                      // positives of a column staged at a time
constexpr int TG_GROUP = 8;                        // positives counted per walk over the column
static_assert(TG_TILE == 16 && TG_TAGS == TG_NT, "the transpose maps thread t to tag t on the way in and to image t & 15 on the way out");
static_assert(TG_MAXK == 4 && TG_MAXT == 8 && SCNATTN_TAG_SUMMARY_LEN == 64, "the summary layout below assumes these");

struct Ks {
    int n;
    int k[TG_MAXK];
};
struct Thr {
    int n;
    float v[TG_MAXT];
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool positive(const void* tg, bool u8, long i) {
    return u8 ? static_cast<const uint8_t*>(tg)[i] != 0 : static_cast<const float*>(tg)[i] >= 0.5f;
}

// One image on one wave.  p / tg point at the image's row.
template <int NPL>
__device__ void tag_row_wave(const float* __restrict__ p, const void* __restrict__ tg, bool u8, int S, const Ks& ks, double* ap,
                             int32_t* npos_out, int32_t* hits_out, int32_t* flag) {
    const int lane = threadIdx.x & 63;
    float s[NPL];
    unsigned long long pb = 0;                     // bit j: element j * 64 + lane is positive
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int i = j * 64 + lane;
        float v = __builtin_nanf("");              // beyond S: compares false against everything
        if (i < S) {
            v = p[i];
            bad |= !(v >= 0.f && v <= 1.f);
            pb |= (unsigned long long)positive(tg, u8, i) << j;
        }
        s[j] = v;
    }
    if (__any(bad) && lane == 0) *flag = 1;
    int npos = 0, hits[TG_MAXK] = {0, 0, 0, 0};
    double sum = 0.0;
    // positives in ascending index: register j, then lane.  The score of the next one is loaded while this one is counted.
    // Everything below is wave-uniform: masks and counts live in scalar registers.
    int j = -1;
    unsigned long long m = 0;
    auto next = [&]() -> int {
        while (m == 0) {
            if (++j >= NPL) return -1;
            m = __ballot((pb >> j) & 1ull);
        }
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        return j * 64 + l;
    };
    int cur = next();
    float si = cur >= 0 ? p[cur] : 0.f;
    while (cur >= 0) {
        const int nxt = next();
        const float sn = nxt >= 0 ? p[nxt] : 0.f;
        const int jc = cur >> 6;
        const unsigned long long below = (1ull << (cur & 63)) - 1ull;      // the lanes of register jc with a lower index
        int N = 0, TP = 0, rk = 0;
#pragma unroll
        for (int jj = 0; jj < NPL; ++jj) {
            const unsigned long long ge = __ballot(s[jj] >= si), gt = __ballot(s[jj] > si);
            const unsigned long long pm = __ballot((pb >> jj) & 1ull);
            const unsigned long long low = jj < jc ? ~0ull : (jj == jc ? below : 0ull);
            N += __popcll(ge);
            TP += __popcll(ge & pm);
            rk += __popcll(gt) + __popcll(ge & ~gt & low);
        }
        sum += (double)TP / (double)N;
        ++npos;
#pragma unroll
        for (int q = 0; q < TG_MAXK; ++q) hits[q] += (q < ks.n) & (rk < ks.k[q]);
        cur = nxt;
        si = sn;
    }
    if (lane == 0) {
        *ap = npos ? sum / (double)npos : 0.0;
        *npos_out = npos;
        for (int q = 0; q < ks.n; ++q) hits_out[q] = hits[q];
    }
}

// Workgroups [0, nrow): rows, 4 images each.  Workgroups [nrow, nrow + tiles * chunks): tile (b - nrow) / chunks of 16 images,
// chunk (b - nrow) % chunks of 256 tags, into the store.
template <int NPL>
__global__ __launch_bounds__(TG_NT) void tag_rows_kernel(int B, int S, int nrow, int chunks, const float* __restrict__ probs,
                                                         long ldp, const void* __restrict__ targets, int u8, long ldt, long row0,
                                                         long cap, Ks ks, float* __restrict__ st_sc, uint8_t* __restrict__ st_lb,
                                                         double* __restrict__ row_ap, int32_t* __restrict__ row_npos,
                                                         int32_t* __restrict__ row_hits, int32_t* __restrict__ flag) {
    __shared__ float tsc[TG_TILE][TG_LD];
    __shared__ unsigned char tlb[TG_TILE][TG_TAGS + 4];
    const int t = threadIdx.x;
    const size_t tsz = u8 ? 1 : 4;
    if ((int)blockIdx.x < nrow) {
        const long r = (long)blockIdx.x * (TG_NT / 64) + (t >> 6);
        if (r < B)
            tag_row_wave<NPL>(probs + r * ldp, static_cast<const char*>(targets) + (size_t)(r * ldt) * tsz, u8 != 0, S, ks,
                              row_ap + row0 + r, row_npos + row0 + r, row_hits + (row0 + r) * ks.n, flag);
        return;
    }
    const int b = (int)blockIdx.x - nrow;
    const int tile0 = (b / chunks) * TG_TILE, c0 = (b % chunks) * TG_TAGS;
    const int nimg = min(TG_TILE, B - tile0);
    const int tag_in = c0 + t;
    if (tag_in < S) {
#pragma unroll
        for (int img = 0; img < TG_TILE; ++img) {
            if (img < nimg) {
                const long r = tile0 + img;
                tsc[img][t] = probs[r * ldp + tag_in];
                tlb[img][t] = positive(static_cast<const char*>(targets) + (size_t)(r * ldt) * tsz, u8 != 0, tag_in);
            }
        }
    }
    __syncthreads();
    const int img = t & 15;
#pragma unroll
    for (int q = 0; q < TG_TAGS / 16; ++q) {
        const int tl = (t >> 4) + 16 * q, tag = c0 + tl;
        if (img < nimg && tag < S) {
            const long at = (long)tag * cap + row0 + tile0 + img;
            st_sc[at] = tsc[img][tl];
            st_lb[at] = tlb[img][tl];
        }
    }
}

__global__ __launch_bounds__(TG_NT) void tag_cols_kernel(int n, long cap, const float* __restrict__ st_sc,
                                                         const uint8_t* __restrict__ st_lb, Thr th, double* __restrict__ col_ap,
                                                         int32_t* __restrict__ col_npos, int32_t* __restrict__ col_counts,
                                                         int32_t* __restrict__ col_agree) {
    __shared__ int tot[2 * (TG_MAXT + 1) + 1];     // predicted and tp per threshold (the last one is 0.5), then npos
    __shared__ float plist[TG_PLIST + TG_GROUP];
    __shared__ int wcnt[TG_NT / 64];
    __shared__ int red[TG_NT / 64][2 * TG_GROUP];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tag = blockIdx.x;
    const float* __restrict__ x = st_sc + (long)tag * cap;
    const uint8_t* __restrict__ y = st_lb + (long)tag * cap;
    constexpr int NC = TG_MAXT + 1;
    if (t < 2 * NC + 1) tot[t] = 0;
    __syncthreads();
    {   // pass 1: integer counts
        int pred[NC], tp[NC], npos = 0;
#pragma unroll
        for (int q = 0; q < NC; ++q) pred[q] = tp[q] = 0;
        for (int j = t; j < n; j += TG_NT) {
            const float v = x[j];
            const int l = y[j];
            npos += l;
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const bool pr = v >= (q < TG_MAXT ? th.v[q] : 0.5f);
                pred[q] += pr;
                tp[q] += pr & l;
            }
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int a = wave_sum_i(pred[q]), b = wave_sum_i(tp[q]);
            if (lane == 0) { atomicAdd(&tot[q], a); atomicAdd(&tot[NC + q], b); }
        }
        npos = wave_sum_i(npos);
        if (lane == 0) atomicAdd(&tot[2 * NC], npos);
    }
    __syncthreads();
    const int m = tot[2 * NC];
    if (t < th.n) {
        const int tp = tot[NC + t], pr = tot[t];
        int32_t* c = col_counts + ((long)tag * th.n + t) * 3;
        c[0] = tp; c[1] = pr - tp; c[2] = m - tp;
    }
    if (t == 0) {
        col_npos[tag] = m;
        const int tp = tot[NC + TG_MAXT], pr = tot[TG_MAXT];
        col_agree[tag] = n - (pr - tp) - (m - tp);
        if (m == 0) col_ap[tag] = 0.0;
    }
    if (m == 0) return;
    // pass 2: AP.  Positives in index order into plist, then eight at a time against the whole column.
    double sum = 0.0;                              // thread 0's
    int scan = 0;
    while (scan < n) {
        int cnt = 0;
        while (scan < n && cnt <= TG_PLIST - TG_NT) {
            const int j = scan + t;
            const bool pos = j < n && y[j] != 0;
            const float v = pos ? x[j] : 0.f;
            const unsigned long long bal = __ballot(pos);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int off = cnt, total = 0;
#pragma unroll
            for (int w = 0; w < TG_NT / 64; ++w) {
                off += w < wave ? wcnt[w] : 0;
                total += wcnt[w];
            }
            if (pos) plist[off + __popcll(bal & ((1ull << lane) - 1ull))] = v;
            cnt += total;
            scan += TG_NT;
            __syncthreads();
        }
        if (t < TG_GROUP) plist[cnt + t] = __builtin_nanf("");      // the last group's tail compares false
        __syncthreads();
        for (int g = 0; g < cnt; g += TG_GROUP) {
            float v[TG_GROUP];
            int ge[TG_GROUP], tp[TG_GROUP];
#pragma unroll
            for (int q = 0; q < TG_GROUP; ++q) { v[q] = plist[g + q]; ge[q] = tp[q] = 0; }
#pragma unroll 4
            for (int j = t; j < n; j += TG_NT) {
                const float xs = x[j];
                const int l = y[j];
#pragma unroll
                for (int q = 0; q < TG_GROUP; ++q) {
                    const bool b = xs >= v[q];
                    ge[q] += b;
                    tp[q] += b & l;
                }
            }
#pragma unroll
            for (int q = 0; q < TG_GROUP; ++q) {
                const int a = wave_sum_i(ge[q]), b = wave_sum_i(tp[q]);
                if (lane == 0) { red[wave][q] = a; red[wave][TG_GROUP + q] = b; }
            }
            __syncthreads();
            if (t == 0) {
                for (int q = 0; q < TG_GROUP && g + q < cnt; ++q) {
                    int N = 0, TP = 0;
                    for (int w = 0; w < TG_NT / 64; ++w) { N += red[w][q]; TP += red[w][TG_GROUP + q]; }
                    sum += (double)TP / (double)N;
                }
            }
            __syncthreads();
        }
    }
    if (t == 0) col_ap[tag] = sum / (double)m;
}

__device__ __forceinline__ double ratio(unsigned long long a, unsigned long long b) { return b ? (double)a / (double)b : 0.0; }

__global__ __launch_bounds__(TG_NT) void tag_finalize_kernel(int S, int n, Ks ks, int nt, const double* __restrict__ row_ap,
                                                             const int32_t* __restrict__ row_npos,
                                                             const int32_t* __restrict__ row_hits,
                                                             const double* __restrict__ col_ap, const int32_t* __restrict__ col_npos,
                                                             const int32_t* __restrict__ col_counts,
                                                             const int32_t* __restrict__ col_agree, const int32_t* __restrict__ flag,
                                                             double* __restrict__ out) {
    constexpr int NSEQ = 1 + 3 * TG_MAXT;          // sums one thread each keeps in index order
    __shared__ double buf[NSEQ][TG_NT];
    __shared__ double res[2][NSEQ];
    __shared__ unsigned long long isum[7 + 3 * TG_MAXT];   // images with a positive, hits per k, tags with a positive, agree, tp/fp/fn
    const int t = threadIdx.x;
    if (t < 7 + 3 * TG_MAXT) isum[t] = 0;
    __syncthreads();
    unsigned long long li[1 + TG_MAXK] = {0, 0, 0, 0, 0};
    double acc = 0.0;
    for (int base = 0; base < n; base += TG_NT) {          // images: AP and recall@k
        const int i = base + t;
        const int np = i < n ? row_npos[i] : 0;
        const bool valid = np > 0;
        buf[0][t] = valid ? row_ap[i] : 0.0;
        li[0] += valid;
#pragma unroll
        for (int q = 0; q < TG_MAXK; ++q) {
            if (q >= ks.n) break;
            const int h = valid ? row_hits[(long)i * ks.n + q] : 0;
            buf[1 + q][t] = valid ? (double)h / (double)np : 0.0;
            li[1 + q] += h;
        }
        __syncthreads();
        if (t < 1 + ks.n) {
#pragma unroll 8
            for (int e = 0; e < TG_NT; ++e) acc += buf[t][e];      // + 0.0 for the rows left out: the sum keeps its bits
        }
        __syncthreads();
    }
    if (t < 1 + ks.n) res[0][t] = acc;
#pragma unroll
    for (int q = 0; q < 1 + TG_MAXK; ++q)
        if (li[q]) atomicAdd(&isum[q], li[q]);
    unsigned long long lt[2 + 3 * TG_MAXT];
#pragma unroll
    for (int q = 0; q < 2 + 3 * TG_MAXT; ++q) lt[q] = 0;
    acc = 0.0;
    for (int base = 0; base < S; base += TG_NT) {          // tags: AP and P / R / F1 per threshold
        const int i = base + t;
        const bool valid = i < S && col_npos[i] > 0;
        buf[0][t] = valid ? col_ap[i] : 0.0;
        lt[0] += valid;
        lt[1] += i < S ? (unsigned long long)col_agree[i] : 0ull;
#pragma unroll
        for (int q = 0; q < TG_MAXT; ++q) {
            if (q >= nt) break;
            unsigned long long tp = 0, fp = 0, fn = 0;
            if (i < S) {
                const int32_t* c = col_counts + ((long)i * nt + q) * 3;
                tp = c[0]; fp = c[1]; fn = c[2];
            }
            lt[2 + 3 * q] += tp; lt[3 + 3 * q] += fp; lt[4 + 3 * q] += fn;
            buf[1 + 3 * q][t] = valid ? ratio(tp, tp + fp) : 0.0;
            buf[2 + 3 * q][t] = valid ? ratio(tp, tp + fn) : 0.0;
            buf[3 + 3 * q][t] = valid ? ratio(2 * tp, 2 * tp + fp + fn) : 0.0;
        }
        __syncthreads();
        if (t < 1 + 3 * nt) {
#pragma unroll 8
            for (int e = 0; e < TG_NT; ++e) acc += buf[t][e];
        }
        __syncthreads();
    }
    if (t < 1 + 3 * nt) res[1][t] = acc;
#pragma unroll
    for (int q = 0; q < 2 + 3 * TG_MAXT; ++q)
        if (lt[q]) atomicAdd(&isum[5 + q], lt[q]);
    __syncthreads();
    if (t != 0) return;
    const double nan = __builtin_nan("");
    const unsigned long long ni = isum[0], ntag = isum[5];
    for (int q = 0; q < SCNATTN_TAG_SUMMARY_LEN; ++q) out[q] = 0.0;
    out[0] = ntag ? res[1][0] / (double)ntag : nan;
    out[1] = ni ? res[0][0] / (double)ni : nan;
    for (int q = 0; q < ks.n; ++q) {
        out[2 + q] = ni ? (double)isum[1 + q] / ((double)ks.k[q] * (double)ni) : nan;      // integers: exact up to the division
        out[6 + q] = ni ? res[0][1 + q] / (double)ni : nan;
    }
    for (int q = 0; q < nt; ++q) {
        const unsigned long long tp = isum[7 + 3 * q], fp = isum[8 + 3 * q], fn = isum[9 + 3 * q];
        double* o = out + 10 + 6 * q;
        o[0] = ratio(tp, tp + fp);
        o[1] = ratio(tp, tp + fn);
        o[2] = ratio(2 * tp, 2 * tp + fp + fn);
        for (int r = 0; r < 3; ++r) o[3 + r] = ntag ? res[1][1 + 3 * q + r] / (double)ntag : nan;
    }
    out[58] = 100.0 * (double)isum[6] / ((double)n * (double)S);
    out[59] = (double)n;
    out[60] = (double)((unsigned long long)n - ni);
    out[61] = (double)((unsigned long long)S - ntag);
    out[62] = (double)*flag;
}

int make_ks(const char* who, int S, const int32_t* ks, int nk, Ks& out) {
    if (nk < 0 || nk > TG_MAXK || (nk > 0 && !ks)) {
        set_error("%s: invalid argument: at most SCNATTN_TAG_MAX_K (4) values of k", who);
        return -1;
    }
    out.n = nk;
    for (int q = 0; q < TG_MAXK; ++q) out.k[q] = 0;
    for (int q = 0; q < nk; ++q) {
        if (ks[q] < 1) { set_error("%s: invalid argument: k < 1", who); return -1; }
        out.k[q] = ks[q] < S ? ks[q] : S;
    }
    return 0;
}

int check_store(const char* who, int S, long n, long cap) {
    if (S < 1 || S > SCNATTN_TAG_MAX_S) { set_error("%s: invalid argument: S outside 1..SCNATTN_TAG_MAX_S", who); return -1; }
    if (cap < 1 || cap > SCNATTN_TAG_MAX_IMAGES) {
        set_error("%s: invalid argument: capacity outside 1..SCNATTN_TAG_MAX_IMAGES", who);
        return -1;
    }
    if (n < 0 || n > cap) { set_error("%s: invalid argument: more images than the capacity of the store", who); return -1; }
    return 0;
}

}  // namespace

int tag_store_size(int S, long cap, size_t* score_bytes, size_t* label_bytes) {
    const char* who = "scnattn_tag_store_size";
    if (!(score_bytes && label_bytes)) { set_error("%s: invalid argument: null pointer", who); return -1; }
    SCN_TRY(check_store(who, S, 0, cap));
    *score_bytes = (size_t)S * (size_t)cap * sizeof(float);
    *label_bytes = (size_t)S * (size_t)cap;
    return 0;
}

int tag_rows(hipStream_t st, int B, int S, const float* probs, long ld_probs, const void* targets, int targets_u8, long ld_targets,
             long row0, long cap, const int32_t* ks, int nk, float* store_scores, uint8_t* store_labels, double* row_ap,
             int32_t* row_npos, int32_t* row_hits, int32_t* flag) {
    const char* who = "scnattn_tag_rows";
    if (!(probs && targets && store_scores && store_labels && row_ap && row_npos && flag) || (nk > 0 && !row_hits)) {
        set_error("%s: invalid argument: null pointer", who);
        return -1;
    }
    if (B < 0 || row0 < 0) { set_error("%s: invalid argument: B < 0 or row0 < 0", who); return -1; }
    SCN_TRY(check_store(who, S, 0, cap));
    if (row0 + B > cap) { set_error("%s: invalid argument: row0 + B exceeds the capacity of the store", who); return -1; }
    if (ld_probs < S || ld_targets < S) { set_error("%s: invalid argument: a leading dimension below S", who); return -1; }
    Ks k;
    SCN_TRY(make_ks(who, S, ks, nk, k));
    if (B == 0) return 0;
    const int nrow = cdiv(B, TG_NT / 64), chunks = cdiv(S, TG_TAGS);
    const dim3 grid(nrow + cdiv(B, TG_TILE) * chunks), block(TG_NT);
#define TG_ROWS(NPL)                                                                                                          \
    hipLaunchKernelGGL(tag_rows_kernel<NPL>, grid, block, 0, st, B, S, nrow, chunks, probs, ld_probs, targets,                \
                       targets_u8 != 0 ? 1 : 0, ld_targets, row0, cap, k, store_scores, store_labels, row_ap, row_npos,       \
                       row_hits, flag)
    if (S <= 256) TG_ROWS(4);
    else if (S <= 1024) TG_ROWS(16);
    else TG_ROWS(64);
#undef TG_ROWS
    SCN_LAUNCH_CHECK();
    return 0;
}

int tag_cols(hipStream_t st, int S, long n, long cap, const float* store_scores, const uint8_t* store_labels,
             const float* thresholds, int nt, double* col_ap, int32_t* col_npos, int32_t* col_counts, int32_t* col_agree) {
    const char* who = "scnattn_tag_cols";
    if (!(store_scores && store_labels && col_ap && col_npos && col_agree) || (nt > 0 && !col_counts)) {
        set_error("%s: invalid argument: null pointer", who);
        return -1;
    }
    if (nt < 0 || nt > TG_MAXT || (nt > 0 && !thresholds)) {
        set_error("%s: invalid argument: at most SCNATTN_TAG_MAX_THRESHOLDS (8) thresholds", who);
        return -1;
    }
    SCN_TRY(check_store(who, S, n, cap));
    if (n < 1) { set_error("%s: invalid argument: no images", who); return -1; }
    Thr th;
    th.n = nt;
    for (int q = 0; q < TG_MAXT; ++q) th.v[q] = q < nt ? thresholds[q] : 0.5f;
    hipLaunchKernelGGL(tag_cols_kernel, dim3(S), dim3(TG_NT), 0, st, (int)n, cap, store_scores, store_labels, th, col_ap,
                       col_npos, col_counts, col_agree);
    SCN_LAUNCH_CHECK();
    return 0;
}

int tag_finalize(hipStream_t st, int S, long n, const int32_t* ks, int nk, int nt, const double* row_ap, const int32_t* row_npos,
                 const int32_t* row_hits, const double* col_ap, const int32_t* col_npos, const int32_t* col_counts,
                 const int32_t* col_agree, const int32_t* flag, double* summary) {
    const char* who = "scnattn_tag_finalize";
    if (!(row_ap && row_npos && col_ap && col_npos && col_agree && flag && summary) || (nk > 0 && !row_hits) ||
        (nt > 0 && !col_counts)) {
        set_error("%s: invalid argument: null pointer", who);
        return -1;
    }
    if (nt < 0 || nt > TG_MAXT) {
        set_error("%s: invalid argument: at most SCNATTN_TAG_MAX_THRESHOLDS (8) thresholds", who);
        return -1;
    }
    SCN_TRY(check_store(who, S, n, SCNATTN_TAG_MAX_IMAGES));
    if (n < 1) { set_error("%s: invalid argument: no images", who); return -1; }
    Ks k;
    SCN_TRY(make_ks(who, S, ks, nk, k));
    hipLaunchKernelGGL(tag_finalize_kernel, dim3(1), dim3(TG_NT), 0, st, S, (int)n, k, nt, row_ap, row_npos, row_hits, col_ap,
                       col_npos, col_counts, col_agree, flag, summary);
    SCN_LAUNCH_CHECK();
    return 0;
}

}  // namespace scn
