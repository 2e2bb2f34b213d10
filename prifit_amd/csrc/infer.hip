// Frozen inference (prifit_amd/inference.py): with fixed statistics a BatchNorm is a per-channel affine that
// folds into the 1x1 convolution in front of it, and the (conv + BN + ReLU) x 3 + max stack of a set-abstraction scale
// (models/pointnet_util.py:250-257 in eval mode) becomes relu(W2' relu(W1' relu(y1) + b1') + b2') followed by the max over
// a group's samples -- which needs no intermediate tensor in memory.
//
//   fold_bn_kernel         every layer of a network in ONE launch: W' = W * s, b' = (b - mean) * s + beta, s = gamma / sqrt(var + eps)
//   mlp_chain_pool_kernel  layers 2 and 3 of a scale and its pool in one launch, the intermediates in registers
//   mlp_chain_rows_kernel  the per-point tail (fp1, conv1 + bn1, conv2) and the restricted arg-max in one launch
//
// The chain kernel computes the TRANSPOSED products on v_mfma_f32_32x32x2_f32 (exact fp32, the instruction of gemm.hip and
// gemm_stream.hip): H^T = W1' X^T and Y^T = W2' H^T, the weights as the A operand and 32 rows of the activation as the B
// operand.  The C/D layout of that instruction gives lane (j, h) the channels 8g + 4h + 0..3 (g = 0..3) of activation row j
// -- which is exactly what the same lane has to supply as the B operand of the next product, for a k order (8g + 4h + m
// instead of ascending k) that the A operand follows by reading W2' at those columns.  So a wave carries its 32 rows from
// the pre-activation it loads to the pooled maximum without LDS, without a barrier and without a shuffle; the only
// cross-lane traffic is the max over the 32 rows at the very end (DPP) and 4 C2 floats of LDS per workgroup to combine the
// waves of a pooling group.  The weights are read from L2 / L1 as MFMA fragments (W1' + W2' are 12 .. 300 KB per scale).
// What follows the last product of a chain is shared with the bf16 kernels of infer_bf16.hip: infer_chain.h.
#include <algorithm>

#include "infer_chain.h"

namespace {

constexpr int FOLD_JOBS = 32;

// the jobs travel by value, like PackJobs of pointops.hip
struct FoldJobs {
    const float *W[FOLD_JOBS], *bias[FOLD_JOBS], *gamma[FOLD_JOBS], *beta[FOLD_JOBS], *mean[FOLD_JOBS], *var[FOLD_JOBS];
    float eps[FOLD_JOBS];
    int cout[FOLD_JOBS], kin[FOLD_JOBS], ldw[FOLD_JOBS];
    long long w_off[FOLD_JOBS], b_off[FOLD_JOBS];
    float *flat;
};

__device__ __forceinline__ float fold_scale(const FoldJobs &jb, int j, int c)
{
    // correctly rounded sqrt and divide whatever the build flags: the test's bound counts one rounding each
    return __fdiv_rn(jb.gamma[j][c], __fsqrt_rn(__fadd_rn(jb.var[j][c], jb.eps[j])));
}

__global__ __launch_bounds__(256) void fold_bn_kernel(FoldJobs jb)
{
    const int j = blockIdx.y;
    const float *__restrict__ W = jb.W[j];
    const int cout = jb.cout[j], kin = jb.kin[j], ldw = jb.ldw[j];
    const bool bn = jb.gamma[j] != nullptr;
    float *__restrict__ Wo = jb.flat + jb.w_off[j];
    const int total = cout * ldw;
    for (int id = blockIdx.x * 256 + threadIdx.x; id < total; id += gridDim.x * 256) {
        const int c = id / ldw, k = id - c * ldw;
        float v = 0.f;                                     // columns kin .. ldw - 1: the padding to a 16-byte row
        if (k < kin) {
            v = W[(size_t)c * kin + k];
            if (bn) v = __fmul_rn(v, fold_scale(jb, j, c));
        }
        Wo[id] = v;
    }
    if (blockIdx.x == 0) {
        float *__restrict__ bo = jb.flat + jb.b_off[j];
        for (int c = threadIdx.x; c < cout; c += 256) {
            const float b = jb.bias[j] ? jb.bias[j][c] : 0.f;
            bo[c] = bn ? __fadd_rn(__fmul_rn(__fsub_rn(b, jb.mean[j][c]), fold_scale(jb, j, c)), jb.beta[j][c]) : b;
        }
    }
}

struct ChainArgs {
    const float *X;
    long long ldx;
    long long P;             // G * pool_K rows
    int G, pool_K;
    const float *W1, *b1, *W2, *b2;
    long long ldw1, ldw2;
    float *out;
    long long ldo;
};

// X [P, C0] (pre-activation of layer 1, ReLU on load) -> out[g, :] = max over the pool_K rows of group g of
// relu(W2 relu(W1 relu(x) + b1) + b2); W1 [C1, ldw1], W2 [C2, ldw2].  C0 % 8 == 0, C1 % 4 == 0, C2 % 32 == 0,
// pool_K in {32, 64, 128}: a wave's 32 rows lie in one group and a workgroup's 128 rows hold whole groups.
template <int C0, int C1, int C2>
__global__ __launch_bounds__(256) void mlp_chain_pool_kernel(const ChainArgs g)
{
    static_assert(C0 % 8 == 0 && C1 % 4 == 0 && C2 % 32 == 0, "fragment shapes");
    constexpr int KQ = C0 / 8, NB1 = (C1 + 31) / 32, NB2 = C2 / 32;
    __shared__ __attribute__((aligned(16))) float s_pool[4][C2];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * CHAIN_ROWS + 32 * wave;

    if (row0 < g.P) {    // wave-uniform; P % 32 == 0: a live wave has 32 rows
        // B operand of layer 1: lane (j, h) holds X[row0 + j][8q + 4h + 0..3], ReLU applied
        float4 xf[KQ];
        {
            const float *xr = g.X + (row0 + li) * g.ldx + 4 * lh;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const float4 v = ld4(xr + 8 * q);
                xf[q] = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            }
        }
        // layer 1: h[b][4g + m] = relu(.) of channel 32b + 8g + 4h + m of row j; channels >= C1 are exactly 0
        f32x16 h[NB1];
#pragma unroll
        for (int b = 0; b < NB1; ++b) {
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int c = 32 * b + li;
            const bool ok = c < C1;
            const float *wr = g.W1 + (long long)(ok ? c : 0) * g.ldw1 + 4 * lh;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                float4 a = ld4(wr + 8 * q);
                if (!ok) a = make_float4(0.f, 0.f, 0.f, 0.f);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xf[q].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xf[q].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xf[q].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xf[q].w, acc, 0, 0, 0);
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
            h[b] = acc;
        }
        // layer 2 + the max over this wave's 32 rows, 32 output channels at a time
#pragma unroll 1
        for (int b2 = 0; b2 < NB2; ++b2) {
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float *wr = g.W2 + (long long)(32 * b2 + li) * g.ldw2;
#pragma unroll
            for (int b = 0; b < NB1; ++b) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    if (32 * b + 8 * gq >= C1) continue;                  // (compile time) no such input channels
                    const int k0 = 32 * b + 8 * gq + 4 * lh;
                    float4 a;
                    if (32 * b + 8 * gq + 8 <= C1) a = ld4(wr + k0);      // (compile time) both halves inside the row
                    else {                                                // C1 % 8 == 4: the upper half is past the row's end
                        a = ld4(wr + (k0 < C1 ? k0 : 0));
                        if (k0 >= C1) a = make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, h[b][4 * gq + 0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, h[b][4 * gq + 1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, h[b][4 * gq + 2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, h[b][4 * gq + 3], acc, 0, 0, 0);
                }
            }
            chain_pool_block(acc, g.b2, b2, li, lh, s_pool[wave]);
        }
    }
    __syncthreads();
    chain_pool_groups<C2>(s_pool, g.G, g.pool_K, g.out, g.ldo);
}

template <int C0, int C1, int C2>
void chain_launch(const ChainArgs &g, hipStream_t st)
{
    const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
    hipLaunchKernelGGL((mlp_chain_pool_kernel<C0, C1, C2>), dim3(grid), dim3(256), 0, st, g);
}

// ---- the per-point tail of the part-segmentation network: four layers over raw rows, scores and / or part labels out
//
// The layout argument above does not stop at two layers: whatever the depth, the C/D registers of one transposed product
// are the B operand of the next, as long as the next weight is read at columns 32b + 8g + 4h + m.  So a wave carries its 32
// rows through fp1's two layers, conv1 + bn1 and conv2 in registers; the last product's C/D layout leaves lane (j, h) with
// the scores of channels 32b + 8g + 4h + m of row j, which it ranks itself before one exchange with lane j of the other half.
typedef RowsArgsT<float> RowsArgs;

// one 128 -> 128 layer on the registers: out = relu(W in + bias), both in the C/D layout (block b, register 4g + m of lane
// (j, h) = channel 32b + 8g + 4h + m of row j)
__device__ __forceinline__ void rows_layer(const float *__restrict__ W, long long ldw, const float *__restrict__ bias,
                                           const f32x16 (&in)[ROWS_NB], f32x16 (&out)[ROWS_NB], int li, int lh)
{
#pragma unroll
    for (int b2 = 0; b2 < ROWS_NB; ++b2) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float *wr = W + (long long)(32 * b2 + li) * ldw + 4 * lh;
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 a = ld4(wr + 32 * b + 8 * gq);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, in[b][4 * gq + 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, in[b][4 * gq + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, in[b][4 * gq + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, in[b][4 * gq + 3], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 bb = ld4(bias + 32 * b2 + 8 * gq + 4 * lh);
            acc[4 * gq + 0] = relu_nan(acc[4 * gq + 0] + bb.x);
            acc[4 * gq + 1] = relu_nan(acc[4 * gq + 1] + bb.y);
            acc[4 * gq + 2] = relu_nan(acc[4 * gq + 2] + bb.z);
            acc[4 * gq + 3] = relu_nan(acc[4 * gq + 3] + bb.w);
        }
        out[b2] = acc;
    }
}

// X [P, 8 KQ] raw rows -> z = W4 relu(W3 relu(W2 relu(W1 x + b1) + b2) + b3) + b4, widths (128, 128, 128, CL <= 64);
// scores[p][0:CL] = z and / or labels[p] = the first maximum of z among the allowed channels (-1: none allowed)
template <int KQ>
__global__ __launch_bounds__(256) void mlp_chain_rows_kernel(const RowsArgs g)
{
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

    f32x16 ha[ROWS_NB], hb[ROWS_NB];
    {
        // B operand of layer 1: lane (j, h) holds X[row0 + j][8q + 4h + 0..3]
        float4 xf[KQ];
        const float *xr = g.X + rowc * g.ldx + 4 * lh;
#pragma unroll
        for (int q = 0; q < KQ; ++q) xf[q] = ld4(xr + 8 * q);
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float *wr = g.W[0] + (long long)(32 * b + li) * g.ldw[0] + 4 * lh;
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const float4 a = ld4(wr + 8 * q);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xf[q].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xf[q].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xf[q].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xf[q].w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 bb = ld4(g.b[0] + 32 * b + 8 * gq + 4 * lh);
                acc[4 * gq + 0] = relu_nan(acc[4 * gq + 0] + bb.x);
                acc[4 * gq + 1] = relu_nan(acc[4 * gq + 1] + bb.y);
                acc[4 * gq + 2] = relu_nan(acc[4 * gq + 2] + bb.z);
                acc[4 * gq + 3] = relu_nan(acc[4 * gq + 3] + bb.w);
            }
            ha[b] = acc;
        }
    }
    rows_layer(g.W[1], g.ldw[1], g.b[1], ha, hb, li, lh);
    rows_layer(g.W[2], g.ldw[2], g.b[2], hb, ha, li, lh);

    // layer 4, no ReLU: channels >= CL are zero A rows (the row index clamped for the load, the value zeroed)
    RowsRank rk = rows_rank_begin(g, rowc);
#pragma unroll
    for (int b2 = 0; b2 < ROWS_MAX_CL / 32; ++b2) {
        if (32 * b2 >= CL) break;                 // grid-uniform
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int c = 32 * b2 + li;
        const bool ok = c < CL;
        const float *wr = g.W[3] + (long long)(ok ? c : 0) * g.ldw[3] + 4 * lh;
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float4 a = ld4(wr + 32 * b + 8 * gq);
                if (!ok) a = make_float4(0.f, 0.f, 0.f, 0.f);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, ha[b][4 * gq + 0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, ha[b][4 * gq + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, ha[b][4 * gq + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, ha[b][4 * gq + 3], acc, 0, 0, 0);
            }
        }
        rows_emit(g, acc, b2, lh, row, live, s_cat, rk);
    }
    rows_finish(g, rk, lh, row, live);
}

template <int KQ>
void rows_launch(const RowsArgs &g, hipStream_t st)
{
    const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
    hipLaunchKernelGGL((mlp_chain_rows_kernel<KQ>), dim3(grid), dim3(256), 0, st, g);
}

template <int KQ>
void rows_dispatch(int kq, const RowsArgs &g, hipStream_t st)
{
    if (kq == KQ) rows_launch<KQ>(g, st);
    else if constexpr (KQ > 1) rows_dispatch<KQ - 1>(kq, g, st);
}

}  // namespace

extern "C" {

int prifit_fold_bn_max_jobs(void) { return FOLD_JOBS; }

int prifit_fold_bn(int njobs, const float *const *W, const int32_t *cout, const int32_t *kin, const float *const *bias,
                   const float *const *gamma, const float *const *beta, const float *const *mean, const float *const *var,
                   const float *eps, const long long *w_off, const int32_t *ldw, const long long *b_off, float *flat,
                   long long flat_len, void *stream)
{
    if (njobs <= 0 || njobs > FOLD_JOBS || !W || !cout || !kin || !bias || !gamma || !beta || !mean || !var || !eps || !w_off ||
        !ldw || !b_off || !flat || mis16(flat))
        return PRIFIT_EINVAL;
    FoldJobs jb = {};
    long long most = 0;
    for (int j = 0; j < njobs; ++j) {
        if (!W[j] || cout[j] <= 0 || kin[j] <= 0 || ldw[j] < kin[j] || (ldw[j] & 3) || (w_off[j] & 3) || w_off[j] < 0 || b_off[j] < 0 ||
            (long long)cout[j] * ldw[j] > 0x7fffffffLL || w_off[j] + (long long)cout[j] * ldw[j] > flat_len ||
            b_off[j] + cout[j] > flat_len)
            return PRIFIT_EINVAL;
        if (gamma[j] && (!beta[j] || !mean[j] || !var[j])) return PRIFIT_EINVAL;
        jb.W[j] = W[j]; jb.bias[j] = bias[j]; jb.gamma[j] = gamma[j]; jb.beta[j] = beta[j]; jb.mean[j] = mean[j]; jb.var[j] = var[j];
        jb.eps[j] = eps[j]; jb.cout[j] = cout[j]; jb.kin[j] = kin[j]; jb.ldw[j] = ldw[j]; jb.w_off[j] = w_off[j]; jb.b_off[j] = b_off[j];
        most = std::max(most, (long long)cout[j] * ldw[j]);
    }
    jb.flat = flat;
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((most + 256 * 4 - 1) / (256 * 4), 1), 256);
    hipLaunchKernelGGL(fold_bn_kernel, dim3(gx, njobs), dim3(256), 0, as_stream(stream), jb);
    return prifit_check_launch();
}

int prifit_mlp_chain_pool_supported(int C0, int C1, int C2, int pool_K)
{
    return (chain_shape(C0, C1, C2) >= 0 && (pool_K == 32 || pool_K == 64 || pool_K == 128)) ? 1 : 0;
}

long long prifit_mlp_chain_pool_workspace(int G, int pool_K, int C0, int C1, int C2)
{
    (void)G; (void)pool_K; (void)C0; (void)C1; (void)C2;
    return 0;   // the intermediates live in registers
}

int prifit_mlp_chain_pool_f32(const float *X, long long ldx, int G, int pool_K, int C0, int C1, int C2, const float *W1,
                              long long ldw1, const float *b1, const float *W2, long long ldw2, const float *b2, float *out,
                              long long ldo, float *workspace, void *stream)
{
    (void)workspace;
    if (!prifit_mlp_chain_pool_supported(C0, C1, C2, pool_K) || !X || !W1 || !b1 || !W2 || !b2 || !out || G <= 0 || ldx < C0 ||
        (ldx & 3) || ldw1 < C0 || (ldw1 & 3) || ldw2 < C1 || (ldw2 & 3) || ldo < C2 || mis16(X) || mis16(W1) || mis16(b1) || mis16(W2) ||
        mis16(b2) || (long long)G * pool_K > 0x7fffffffLL)
        return PRIFIT_EINVAL;
    ChainArgs g = {};
    g.X = X; g.ldx = ldx; g.P = (long long)G * pool_K; g.G = G; g.pool_K = pool_K;
    g.W1 = W1; g.b1 = b1; g.W2 = W2; g.b2 = b2; g.ldw1 = ldw1; g.ldw2 = ldw2; g.out = out; g.ldo = ldo;
    hipStream_t st = as_stream(stream);
    switch (chain_shape(C0, C1, C2)) {
    case 0: chain_launch<32, 32, 64>(g, st); break;
    case 1: chain_launch<64, 64, 128>(g, st); break;
    case 2: chain_launch<64, 96, 128>(g, st); break;
    case 3: chain_launch<128, 128, 256>(g, st); break;
    default: chain_launch<128, 196, 256>(g, st); break;
    }
    return prifit_check_launch();
}

int prifit_mlp_chain_rows_supported(int K0, int L, const int32_t *widths)
{
    if (L != ROWS_L || !widths || K0 < 8 || K0 > ROWS_MAX_K0 || (K0 & 7)) return 0;
    for (int l = 0; l + 1 < ROWS_L; ++l)
        if (widths[l] != ROWS_W) return 0;
    return (widths[ROWS_L - 1] >= 1 && widths[ROWS_L - 1] <= ROWS_MAX_CL) ? 1 : 0;
}

long long prifit_mlp_chain_rows_workspace(long long P, int K0, int L, const int32_t *widths)
{
    (void)P; (void)K0; (void)L; (void)widths;
    return 0;   // the intermediates live in registers
}

int prifit_mlp_chain_rows_f32(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                              const float *const *W, const long long *ldw, const float *const *b, float *scores, long long lds,
                              int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape,
                              float *workspace, void *stream)
{
    (void)workspace;
    if (rows_check(K0, L, widths, X, ldx, P, W, ldw, b, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape))
        return PRIFIT_EINVAL;
    const int CL = widths[ROWS_L - 1];
    RowsArgs g = {};
    for (int l = 0; l < ROWS_L; ++l) {
        const int kin = l ? ROWS_W : K0;
        if (!W[l] || !b[l] || ldw[l] < kin || (ldw[l] & 3) || mis16(W[l]) || mis16(b[l])) return PRIFIT_EINVAL;
        g.W[l] = W[l]; g.b[l] = b[l]; g.ldw[l] = ldw[l];
    }
    g.X = X; g.ldx = ldx; g.P = P; g.CL = CL; g.scores = scores; g.lds = lds; g.labels = labels;
    g.cat_of_label = labels ? cat_of_label : nullptr; g.shape_cat = labels ? shape_cat : nullptr; g.N = rows_per_shape;
    rows_dispatch<ROWS_MAX_K0 / 8>(K0 / 8, g, as_stream(stream));
    return prifit_check_launch();
}

}  // extern "C"
