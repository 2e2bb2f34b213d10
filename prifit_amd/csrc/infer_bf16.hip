// Frozen inference with bf16 arithmetic (prifit_amd/inference.py precision="bf16"): the on-chip chains of
// infer.hip on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same transposed products H^T = W1' X^T, Y^T = W2' H^T.
//
//   pack_bf16_multi_kernel      every chained layer's folded weight -> bf16 in the column order its MFMA reads, ONE launch
//   mlp_chain_pool_bf16_kernel  layers 2 and 3 of a set-abstraction scale and its pool
//   mlp_chain_rows_bf16_kernel  the per-point tail (fp1, conv1 + bn1, conv2) and the restricted arg-max
//
// The register-resident design carries over because the C/D layout of the 32x32 MFMAs does not depend on the input type:
// register r of lane (j, h) of a 32x32 result is channel (r & 3) + 8 (r >> 2) + 4h of activation row j.  The B operand of
// v_mfma_f32_32x32x16_bf16 wants B[k = 8h + e][col j] in element e = 0..7 of lane (j, h), so registers 8s .. 8s + 7 of a
// result, rounded to bf16 pairwise, ARE the B fragment of k-step s of the next product -- for the k order
//     element e of lane half h in k-step t  =  channel 16t + 8(e >> 2) + 4h + (e & 3)
// (t = 2b + s over the 32-channel blocks b), which the A operand follows: the pack kernel stores the weight's columns in
// that order, 16 per k-step, so a lane fetches its 8 elements with one 16-byte load at column 16t + 8h.  A first layer is
// fed from memory in the plain order (element e of half h = column 16t + 8h + e) and its weight is packed plainly.
// An activation is rounded to bf16 ONCE, when its layer ends, not per use; what follows the last product is infer_chain.h.
#include <algorithm>

#include "infer_chain.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

namespace {

// ---- weights -> bf16
constexpr int PACK16_JOBS = 16;

struct Pack16Jobs {
    const float *w[PACK16_JOBS];
    uint16_t *out[PACK16_JOBS];
    int rows[PACK16_JOBS], cols[PACK16_JOBS], ldw[PACK16_JOBS], order[PACK16_JOBS];
};

// round to nearest even, NaN -> the default quiet NaN, overflow -> inf: c10::BFloat16's conversion, bit for bit
__device__ __forceinline__ unsigned bf16_bits(float x)
{
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256) void pack_bf16_multi_kernel(Pack16Jobs jb)
{
    const int j = blockIdx.y;
    const float *__restrict__ w = jb.w[j];
    uint16_t *__restrict__ out = jb.out[j];
    const int cols = jb.cols[j], ldw = jb.ldw[j], acc_order = jb.order[j];
    const int ldk = (cols + 15) & ~15;
    const int total = jb.rows[j] * ldk;
    for (int id = blockIdx.x * 256 + threadIdx.x; id < total; id += gridDim.x * 256) {
        const int c = id / ldk, p = id - c * ldk;
        const int e = p & 7, h = (p >> 3) & 1;
        const int k = acc_order ? (p & ~15) + 8 * (e >> 2) + 4 * h + (e & 3) : p;
        out[id] = k < cols ? (uint16_t)bf16_bits(w[(size_t)c * ldw + k]) : (uint16_t)0;   // columns cols .. ldk - 1: zero
    }
}

// ---- fragments
__device__ __forceinline__ bf16x8 ldw8(const uint16_t *p) { return *reinterpret_cast<const bf16x8 *>(p); }

__device__ __forceinline__ bf16x8 zero8()
{
    return __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
}

// eight floats -> one B fragment (v_cvt_pk_bf16_f32: round to nearest even, a NaN stays a NaN)
__device__ __forceinline__ bf16x8 cvt8(float4 lo, float4 hi)
{
    const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_convertvector(v, bf16x8);
}

// registers 8s .. 8s + 7 of a finished layer's block -> the B fragment of k-step 2b + s of the next product
__device__ __forceinline__ bf16x8 cvt_acc(const f32x16 &a, int s)
{
    const f32x8 v = {a[8 * s + 0], a[8 * s + 1], a[8 * s + 2], a[8 * s + 3], a[8 * s + 4], a[8 * s + 5], a[8 * s + 6], a[8 * s + 7]};
    return __builtin_convertvector(v, bf16x8);
}

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

constexpr f32x16 ZERO16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

// ---- the pooled chain
struct Chain16Args {
    const float *X;
    long long ldx;
    long long P;             // G * pool_K rows
    int G, pool_K;
    const uint16_t *W1, *W2;
    const float *b1, *b2;
    long long ldw1, ldw2;
    float *out;
    long long ldo;
};

// as mlp_chain_pool_kernel of infer.hip; W1 [C1, ldw1] bf16 in the plain order, W2 [C2, ldw2] bf16 in the accumulator order,
// both zero from their input width to the next multiple of 16.  C0 % 16 == 0: no k-step of layer 1 reaches past a row of X.
// Channels C1 .. 16 KS1 - 1 of the intermediate are exactly 0 (zero A rows, zero bias) and meet zero columns of W2.
template <int C0, int C1, int C2>
__global__ __launch_bounds__(256) void mlp_chain_pool_bf16_kernel(const Chain16Args g)
{
    static_assert(C0 % 16 == 0 && C1 % 4 == 0 && C2 % 32 == 0, "fragment shapes");
    constexpr int KS0 = C0 / 16, NB1 = (C1 + 31) / 32, KS1 = (C1 + 15) / 16, NB2 = C2 / 32;
    __shared__ __attribute__((aligned(16))) float s_pool[4][C2];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * CHAIN_ROWS + 32 * wave;

    if (row0 < g.P) {    // wave-uniform; P % 32 == 0: a live wave has 32 rows
        // B operand of layer 1: lane (j, h) holds relu(X[row0 + j][16t + 8h + 0..7]) in k-step t
        bf16x8 xb[KS0];
        {
            const float *xr = g.X + (row0 + li) * g.ldx + 8 * lh;
#pragma unroll
            for (int t = 0; t < KS0; ++t) {
                const float4 u = ld4(xr + 16 * t), v = ld4(xr + 16 * t + 4);
                xb[t] = cvt8(make_float4(fmaxf(u.x, 0.f), fmaxf(u.y, 0.f), fmaxf(u.z, 0.f), fmaxf(u.w, 0.f)),
                             make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)));
            }
        }
        // layer 1, rounded to the B fragments of layer 2 as each block ends
        bf16x8 hb[KS1];
#pragma unroll
        for (int b = 0; b < NB1; ++b) {
            f32x16 acc = ZERO16;
            const int c = 32 * b + li;
            const bool ok = c < C1;
            const uint16_t *wr = g.W1 + (long long)(ok ? c : 0) * g.ldw1 + 8 * lh;
#pragma unroll
            for (int t = 0; t < KS0; ++t) {
                bf16x8 a = ldw8(wr + 16 * t);
                if (!ok) a = zero8();
                acc = mfma16(a, xb[t], acc);
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int c0 = 32 * b + 8 * gq + 4 * lh;       // C1 % 4 == 0: the four channels are in or out together
                const float4 bb = c0 < C1 ? ld4(g.b1 + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                acc[4 * gq + 0] = fmaxf(acc[4 * gq + 0] + bb.x, 0.f);
                acc[4 * gq + 1] = fmaxf(acc[4 * gq + 1] + bb.y, 0.f);
                acc[4 * gq + 2] = fmaxf(acc[4 * gq + 2] + bb.z, 0.f);
                acc[4 * gq + 3] = fmaxf(acc[4 * gq + 3] + bb.w, 0.f);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (2 * b + s < KS1) hb[2 * b + s] = cvt_acc(acc, s);      // (compile time)
        }
        // layer 2 + the max over this wave's 32 rows, 32 output channels at a time
#pragma unroll 1
        for (int b2 = 0; b2 < NB2; ++b2) {
            f32x16 acc = ZERO16;
            const uint16_t *wr = g.W2 + (long long)(32 * b2 + li) * g.ldw2 + 8 * lh;
#pragma unroll
            for (int t = 0; t < KS1; ++t) acc = mfma16(ldw8(wr + 16 * t), hb[t], acc);
            chain_pool_block(acc, g.b2, b2, li, lh, s_pool[wave]);
        }
    }
    __syncthreads();
    chain_pool_groups<C2>(s_pool, g.G, g.pool_K, g.out, g.ldo);
}

template <int C0, int C1, int C2>
void chain16_launch(const Chain16Args &g, hipStream_t st)
{
    const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
    hipLaunchKernelGGL((mlp_chain_pool_bf16_kernel<C0, C1, C2>), dim3(grid), dim3(256), 0, st, g);
}

// ---- the per-point tail
typedef RowsArgsT<uint16_t> Rows16Args;
constexpr int ROWS_KS = ROWS_W / 16;      // k-steps of a 128-wide layer

// relu(acc + bias) of output block b2, a NaN kept, rounded into the next layer's B fragments 2 b2 and 2 b2 + 1
__device__ __forceinline__ void rows16_close(f32x16 acc, const float *__restrict__ bias, int b2, int lh, bf16x8 (&out)[ROWS_KS])
{
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const float4 bb = ld4(bias + 32 * b2 + 8 * gq + 4 * lh);
        acc[4 * gq + 0] = relu_nan(acc[4 * gq + 0] + bb.x);
        acc[4 * gq + 1] = relu_nan(acc[4 * gq + 1] + bb.y);
        acc[4 * gq + 2] = relu_nan(acc[4 * gq + 2] + bb.z);
        acc[4 * gq + 3] = relu_nan(acc[4 * gq + 3] + bb.w);
    }
    out[2 * b2] = cvt_acc(acc, 0);
    out[2 * b2 + 1] = cvt_acc(acc, 1);
}

// one 128 -> 128 layer on the registers; W in the accumulator order
__device__ __forceinline__ void rows16_layer(const uint16_t *__restrict__ W, long long ldw, const float *__restrict__ bias,
                                             const bf16x8 (&in)[ROWS_KS], bf16x8 (&out)[ROWS_KS], int li, int lh)
{
#pragma unroll
    for (int b2 = 0; b2 < ROWS_NB; ++b2) {
        f32x16 acc = ZERO16;
        const uint16_t *wr = W + (long long)(32 * b2 + li) * ldw + 8 * lh;
#pragma unroll
        for (int t = 0; t < ROWS_KS; ++t) acc = mfma16(ldw8(wr + 16 * t), in[t], acc);
        rows16_close(acc, bias, b2, lh, out);
    }
}

// as mlp_chain_rows_kernel of infer.hip, X [P, 8 KQ] raw rows.  KQ odd: the upper lane half of the last k-step lies past the
// row's end -- it loads nothing (the next row, or memory that is not ours, could hold a NaN) and holds zeros.
template <int KQ>
__global__ __launch_bounds__(256) void mlp_chain_rows_bf16_kernel(const Rows16Args g)
{
    constexpr int KS = (KQ + 1) / 2;
    __shared__ int s_cat[ROWS_MAX_CL];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int CL = g.CL;
    rows_load_cats(g, s_cat);
    const long long row0 = (long long)blockIdx.x * CHAIN_ROWS + 32 * wave;
    if (row0 >= g.P) return;                      // wave-uniform
    const long long row = row0 + li;
    const bool live = row < g.P;                  // a row past the end computes on a copy of the last row and stores nothing
    const long long rowc = live ? row : g.P - 1;

    bf16x8 ha[ROWS_KS], hb[ROWS_KS];
    {
        bf16x8 xb[KS];
        const float *xr = g.X + rowc * g.ldx + 8 * lh;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            if (2 * t + 1 < KQ || lh == 0) xb[t] = cvt8(ld4(xr + 16 * t), ld4(xr + 16 * t + 4));
            else xb[t] = zero8();
        }
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
            f32x16 acc = ZERO16;
            const uint16_t *wr = g.W[0] + (long long)(32 * b + li) * g.ldw[0] + 8 * lh;
#pragma unroll
            for (int t = 0; t < KS; ++t) acc = mfma16(ldw8(wr + 16 * t), xb[t], acc);
            rows16_close(acc, g.b[0], b, lh, ha);
        }
    }
    rows16_layer(g.W[1], g.ldw[1], g.b[1], ha, hb, li, lh);
    rows16_layer(g.W[2], g.ldw[2], g.b[2], hb, ha, li, lh);

    // layer 4, no ReLU: channels >= CL are zero A rows (the row index clamped for the load, the value zeroed)
    RowsRank rk = rows_rank_begin(g, rowc);
#pragma unroll
    for (int b2 = 0; b2 < ROWS_MAX_CL / 32; ++b2) {
        if (32 * b2 >= CL) break;                 // grid-uniform
        f32x16 acc = ZERO16;
        const int c = 32 * b2 + li;
        const bool ok = c < CL;
        const uint16_t *wr = g.W[3] + (long long)(ok ? c : 0) * g.ldw[3] + 8 * lh;
#pragma unroll
        for (int t = 0; t < ROWS_KS; ++t) {
            bf16x8 a = ldw8(wr + 16 * t);
            if (!ok) a = zero8();
            acc = mfma16(a, ha[t], acc);
        }
        rows_emit(g, acc, b2, lh, row, live, s_cat, rk);
    }
    rows_finish(g, rk, lh, row, live);
}

template <int KQ>
void rows16_dispatch(int kq, const Rows16Args &g, hipStream_t st)
{
    if (kq == KQ) {
        const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
        hipLaunchKernelGGL((mlp_chain_rows_bf16_kernel<KQ>), dim3(grid), dim3(256), 0, st, g);
    } else if constexpr (KQ > 1) rows16_dispatch<KQ - 1>(kq, g, st);
}

inline long long up16(long long k) { return (k + 15) & ~15LL; }

}  // namespace

extern "C" {

int prifit_pack_bf16_max_jobs(void) { return PACK16_JOBS; }

int prifit_pack_bf16_multi(int njobs, const float *const *w, const int32_t *rows, const int32_t *cols, const int32_t *ldw,
                           const int32_t *order, uint16_t *const *out, void *stream)
{
    if (njobs <= 0 || njobs > PACK16_JOBS || !w || !rows || !cols || !ldw || !order || !out) return PRIFIT_EINVAL;
    Pack16Jobs jb = {};
    long long most = 0;
    for (int j = 0; j < njobs; ++j) {
        if (!w[j] || !out[j] || rows[j] <= 0 || cols[j] <= 0 || ldw[j] < cols[j] || (order[j] != 0 && order[j] != 1) || mis16(out[j]) ||
            (long long)rows[j] * up16(cols[j]) > 0x7fffffffLL)
            return PRIFIT_EINVAL;
        jb.w[j] = w[j]; jb.out[j] = out[j]; jb.rows[j] = rows[j]; jb.cols[j] = cols[j]; jb.ldw[j] = ldw[j]; jb.order[j] = order[j];
        most = std::max(most, (long long)rows[j] * up16(cols[j]));
    }
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((most + 256 * 4 - 1) / (256 * 4), 1), 256);
    hipLaunchKernelGGL(pack_bf16_multi_kernel, dim3(gx, njobs), dim3(256), 0, as_stream(stream), jb);
    return prifit_check_launch();
}

int prifit_mlp_chain_pool_bf16_supported(int C0, int C1, int C2, int pool_K)
{
    return prifit_mlp_chain_pool_supported(C0, C1, C2, pool_K);   // the same five triples (every C0 is a multiple of 16)
}

long long prifit_mlp_chain_pool_bf16_workspace(int G, int pool_K, int C0, int C1, int C2)
{
    (void)G; (void)pool_K; (void)C0; (void)C1; (void)C2;
    return 0;   // the intermediates live in registers
}

int prifit_mlp_chain_pool_bf16(const float *X, long long ldx, int G, int pool_K, int C0, int C1, int C2, const uint16_t *W1,
                               long long ldw1, const float *b1, const uint16_t *W2, long long ldw2, const float *b2, float *out,
                               long long ldo, float *workspace, void *stream)
{
    (void)workspace;
    if (!prifit_mlp_chain_pool_bf16_supported(C0, C1, C2, pool_K) || !X || !W1 || !b1 || !W2 || !b2 || !out || G <= 0 || ldx < C0 ||
        (ldx & 3) || ldw1 < up16(C0) || (ldw1 & 7) || ldw2 < up16(C1) || (ldw2 & 7) || ldo < C2 || mis16(X) || mis16(W1) || mis16(b1) ||
        mis16(W2) || mis16(b2) || (long long)G * pool_K > 0x7fffffffLL)
        return PRIFIT_EINVAL;
    Chain16Args g = {};
    g.X = X; g.ldx = ldx; g.P = (long long)G * pool_K; g.G = G; g.pool_K = pool_K;
    g.W1 = W1; g.b1 = b1; g.W2 = W2; g.b2 = b2; g.ldw1 = ldw1; g.ldw2 = ldw2; g.out = out; g.ldo = ldo;
    hipStream_t st = as_stream(stream);
    switch (chain_shape(C0, C1, C2)) {
    case 0: chain16_launch<32, 32, 64>(g, st); break;
    case 1: chain16_launch<64, 64, 128>(g, st); break;
    case 2: chain16_launch<64, 96, 128>(g, st); break;
    case 3: chain16_launch<128, 128, 256>(g, st); break;
    default: chain16_launch<128, 196, 256>(g, st); break;
    }
    return prifit_check_launch();
}

int prifit_mlp_chain_rows_bf16_supported(int K0, int L, const int32_t *widths)
{
    return prifit_mlp_chain_rows_supported(K0, L, widths);
}

long long prifit_mlp_chain_rows_bf16_workspace(long long P, int K0, int L, const int32_t *widths)
{
    (void)P; (void)K0; (void)L; (void)widths;
    return 0;   // the intermediates live in registers
}

int prifit_mlp_chain_rows_bf16(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                               const uint16_t *const *W, const long long *ldw, const float *const *b, float *scores, long long lds,
                               int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape,
                               float *workspace, void *stream)
{
    (void)workspace;
    if (rows_check(K0, L, widths, X, ldx, P, W, ldw, b, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape))
        return PRIFIT_EINVAL;
    Rows16Args g = {};
    for (int l = 0; l < ROWS_L; ++l) {
        const int kin = l ? ROWS_W : K0;
        if (!W[l] || !b[l] || ldw[l] < up16(kin) || (ldw[l] & 7) || mis16(W[l]) || mis16(b[l])) return PRIFIT_EINVAL;
        g.W[l] = W[l]; g.b[l] = b[l]; g.ldw[l] = ldw[l];
    }
    g.X = X; g.ldx = ldx; g.P = P; g.CL = widths[ROWS_L - 1]; g.scores = scores; g.lds = lds; g.labels = labels;
    g.cat_of_label = labels ? cat_of_label : nullptr; g.shape_cat = labels ? shape_cat : nullptr; g.N = rows_per_shape;
    rows16_dispatch<ROWS_MAX_K0 / 8>(K0 / 8, g, as_stream(stream));
    return prifit_check_launch();
}

}  // extern "C"
