// What the on-chip MLP chains of frozen inference share between their fp32 (infer.hip) and bf16 (infer_bf16.hip) forms: the
// C/D layout of the 32x32 MFMAs does not depend on the input type, so everything behind the last product -- the max over a
// wave's rows and the pooling groups of a workgroup, the scores' stores and the category-restricted arg-max -- is one piece of
// code.  (Block b, register 4g + m of lane (j, h) = channel 32b + 8g + 4h + m of activation row j.)
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CHAIN_ROWS = 128;   // rows per workgroup: 4 waves x 32

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_max(float v)
{
    const int o = __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xf, false);
    return fmaxf(v, __builtin_bit_cast(float, o));
}

// max over the 32 lanes of each half of the wave (lanes 0..31 and 32..63 separately); valid in lanes 16..31 and 48..63
__device__ __forceinline__ float half_wave_max(float v)
{
    v = dpp_max<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = dpp_max<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v = dpp_max<0x124, 0xf>(v);   // row_ror:4
    v = dpp_max<0x128, 0xf>(v);   // row_ror:8  -> every lane holds the max of its row of 16
    v = dpp_max<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3 -> they hold the max of rows 0 + 1 / 2 + 3
    return v;
}

inline int chain_shape(int C0, int C1, int C2)
{
    static const int shapes[5][3] = {{32, 32, 64}, {64, 64, 128}, {64, 96, 128}, {128, 128, 256}, {128, 196, 256}};
    for (int i = 0; i < 5; ++i)
        if (shapes[i][0] == C0 && shapes[i][1] == C1 && shapes[i][2] == C2) return i;
    return -1;
}

inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

// ---- the pooled chain's end: output block b2 of the last layer (fp32 accumulators of a wave's 32 rows) -> s_pool[C2] of
// this wave.  Max over rows first, bias and ReLU on the maximum: x -> relu(x + b) is non-decreasing in fp32, so the two
// commute exactly.
__device__ __forceinline__ void chain_pool_block(f32x16 acc, const float *__restrict__ b2v, int b2, int li, int lh, float *s_pool_wave)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = half_wave_max(acc[r]);
    if (li == 31) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int c0 = 32 * b2 + 8 * gq + 4 * lh;
            const float4 bb = ld4(b2v + c0);
            *reinterpret_cast<float4 *>(&s_pool_wave[c0]) =
                make_float4(fmaxf(acc[4 * gq + 0] + bb.x, 0.f), fmaxf(acc[4 * gq + 1] + bb.y, 0.f),
                            fmaxf(acc[4 * gq + 2] + bb.z, 0.f), fmaxf(acc[4 * gq + 3] + bb.w, 0.f));
        }
    }
}

// the waves of a pooling group: pool_K / 32 neighbours (a live group has all of them: P = G * pool_K); after a barrier
template <int C2>
__device__ __forceinline__ void chain_pool_groups(const float (&s_pool)[4][C2], int G, int pool_K, float *out, long long ldo)
{
    const int wpg = pool_K >> 5, gpt = CHAIN_ROWS / pool_K;
    for (int id = threadIdx.x; id < gpt * C2; id += 256) {
        const int gi = id / C2, c = id - gi * C2;
        const long long grp = (long long)blockIdx.x * gpt + gi;
        if (grp >= G) break;
        float v = s_pool[gi * wpg][c];
        for (int w = 1; w < wpg; ++w) v = fmaxf(v, s_pool[gi * wpg + w][c]);
        out[grp * ldo + c] = v;
    }
}

// ---- the per-point tail's end: scores and / or part labels from the last layer's accumulators
constexpr int ROWS_L = 4, ROWS_W = 128, ROWS_NB = ROWS_W / 32, ROWS_MAX_CL = 64, ROWS_MAX_K0 = 160;

template <typename WT>
struct RowsArgsT {
    const float *X;
    long long ldx, P;
    const WT *W[ROWS_L];
    const float *b[ROWS_L];
    long long ldw[ROWS_L];
    int CL;
    float *scores;
    long long lds;
    int32_t *labels;
    const int32_t *cat_of_label, *shape_cat;     // shape_cat NULL: every channel < CL is allowed
    int N;                                       // rows per shape
};

// ReLU that keeps a NaN (np.maximum, torch.relu): a NaN input row reaches the scores, where the arg-max rule ranks it
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }

// order-preserving key of a score among the ALLOWED channels: score_key of seg_metrics.hip, bit for bit (NaN = the largest
// key, -0 = +0, always >= 0x007fffff so that 0 is free for the channels outside the window)
__device__ __forceinline__ unsigned rows_score_key(float x)
{
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if ((u << 1) == 0) return 0x80000000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (grid-uniform) the category table, once per workgroup; its barrier is the only one, before the chain starts
template <typename A>
__device__ __forceinline__ void rows_load_cats(const A &g, int *s_cat)
{
    if (g.labels && g.shape_cat) {
        if (threadIdx.x < ROWS_MAX_CL) s_cat[threadIdx.x] = threadIdx.x < g.CL ? g.cat_of_label[threadIdx.x] : 0;
        __syncthreads();
    }
}

struct RowsRank {
    bool vec;                     // grid-uniform: float4 stores of the scores are aligned
    int cat;                      // the row's category
    unsigned long long best;      // (key << 32) | (63 - channel): the larger key, then the lower channel
};

template <typename A>
__device__ __forceinline__ RowsRank rows_rank_begin(const A &g, long long rowc)
{
    RowsRank r;
    r.vec = g.scores && !(g.lds & 3) && !((uintptr_t)g.scores & 15);
    r.cat = (g.labels && g.shape_cat) ? g.shape_cat[(int)rowc / g.N] : 0;      // P <= 2^31 - 1
    r.best = 0;
    return r;
}

// output block b2 of the last layer: z = acc + bias, stored as scores and / or ranked among the allowed channels
template <typename A>
__device__ __forceinline__ void rows_emit(const A &g, const f32x16 &acc, int b2, int lh, long long row, bool live, const int *s_cat,
                                          RowsRank &rk)
{
    const int CL = g.CL;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int c0 = 32 * b2 + 8 * gq + 4 * lh;
        float z[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) z[m] = acc[4 * gq + m] + (c0 + m < CL ? g.b[3][c0 + m] : 0.f);
        if (g.scores && live) {
            float *sr = g.scores + row * g.lds + c0;
            if (rk.vec && c0 + 4 <= CL) *reinterpret_cast<float4 *>(sr) = make_float4(z[0], z[1], z[2], z[3]);
            else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (c0 + m < CL) sr[m] = z[m];
            }
        }
        if (g.labels) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {     // ascending channels within the lane: > keeps the first maximum
                const int ch = c0 + m;
                // a negative category is none (prifit_seg_metrics' shape_cat -1), whatever cat_of_label holds
                const bool allowed = ch < CL && (!g.shape_cat || (rk.cat >= 0 && s_cat[ch < ROWS_MAX_CL ? ch : 0] == rk.cat));
                const unsigned long long k =
                    allowed ? ((unsigned long long)rows_score_key(z[m]) << 32) | (unsigned)(63 - ch) : 0ull;
                rk.best = k > rk.best ? k : rk.best;
            }
        }
    }
}

// lanes j and j + 32 hold the two halves of row j's channels: one exchange, the tie goes to the lower channel
template <typename A>
__device__ __forceinline__ void rows_finish(const A &g, RowsRank &rk, int lh, long long row, bool live)
{
    if (g.labels) {
        unsigned long long best = rk.best;
        const unsigned hi = __shfl_xor((unsigned)(best >> 32), 32), lo = __shfl_xor((unsigned)best, 32);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        best = other > best ? other : best;
        if (lh == 0 && live) g.labels[row] = (best >> 32) ? 63 - (int)(best & 63u) : -1;
    }
}

// the checks of a rows launch that do not depend on the weights' type; CL out
template <typename WT>
inline int rows_check(int K0, int L, const int32_t *widths, const float *X, long long ldx, long long P, const WT *const *W,
                      const long long *ldw, const float *const *b, float *scores, long long lds, int32_t *labels,
                      const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape)
{
    if (!prifit_mlp_chain_rows_supported(K0, L, widths) || !X || !W || !ldw || !b || (!scores && !labels) || P < 1 ||
        P > 0x7fffffffLL || ldx < K0 || (ldx & 3) || mis16(X) || rows_per_shape <= 0)
        return PRIFIT_EINVAL;
    if (scores && lds < widths[ROWS_L - 1]) return PRIFIT_EINVAL;
    if (labels && (shape_cat != nullptr) != (cat_of_label != nullptr)) return PRIFIT_EINVAL;
    if (labels && shape_cat && P % rows_per_shape) return PRIFIT_EINVAL;
    return PRIFIT_OK;
}

}  // namespace
