// Frozen inference (prifit_amd/inference.py): with fixed statistics a BatchNorm is a per-channel affine that
// folds into the 1x1 convolution in front of it, and the (conv + BN + ReLU) x 3 + max stack of a set-abstraction scale
// (models/pointnet_util.py:250-257 in eval mode) becomes relu(W2' relu(W1' relu(y1) + b1') + b2') followed by the max over
// a group's samples -- which needs no intermediate tensor in memory.
//
//   fold_bn_kernel         every layer of a network in ONE launch: W' = W * s, b' = (b - mean) * s + beta, s = gamma / sqrt(var + eps)
//   mlp_chain_pool_kernel  layers 2 and 3 of a scale and its pool in one launch, the intermediates in registers
//   mlp_chain_rows_kernel  the per-point tail (fp1, conv1 + bn1, conv2) and the restricted arg-max in one launch
//   mlp_chain_embed_kernel the same tail with two heads: extra_conv_emb (row-major, optionally unit-normalised) and conv2
//
// The chain kernels, their argument checks and their launch ladders are written once, in infer_chain.h, over a matrix-pipe
// policy; this file holds the fold and the fp32 entry points, which instantiate the skeleton for the fp32 policy (PipeF32 of
// infer_pipe_f32.h: v_mfma_f32_32x32x2_f32, exact fp32, the instruction of gemm.hip and gemm_stream.hip).  The bf16 twin is
// infer_bf16.hip; the training half of the row chain (loss and conv2 gradient) is probe_head.hip.
// The weights are read from L2 / L1 as MFMA fragments (W1' + W2' are 12 .. 300 KB per scale).
#include <algorithm>

#include "infer_chain.h"
#include "infer_pipe_f32.h"

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

int prifit_mlp_chain_pool_supported(int C0, int C1, int C2, int pool_K) { return chain_pool_supported(C0, C1, C2, pool_K); }

long long prifit_mlp_chain_pool_workspace(int, int, int, int, int) { return 0; }     // the intermediates live in registers

int prifit_mlp_chain_pool_f32(const float *X, long long ldx, int G, int pool_K, int C0, int C1, int C2, const float *W1,
                              long long ldw1, const float *b1, const float *W2, long long ldw2, const float *b2, float *out,
                              long long ldo, float *, void *stream)
{
    return chain_pool_run<PipeF32>(X, ldx, G, pool_K, C0, C1, C2, W1, ldw1, b1, W2, ldw2, b2, out, ldo, stream);
}

int prifit_mlp_chain_rows_supported(int K0, int L, const int32_t *widths) { return chain_rows_supported(K0, L, widths); }

long long prifit_mlp_chain_rows_workspace(long long, int, int, const int32_t *) { return 0; }     // likewise

int prifit_mlp_chain_rows_f32(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                              const float *const *W, const long long *ldw, const float *const *b, float *scores, long long lds,
                              int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape, float *,
                              void *stream)
{
    return chain_rows_run<PipeF32>(X, ldx, P, K0, L, widths, W, ldw, b, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape,
                                   stream);
}

int prifit_mlp_chain_embed_supported(int K0, int L, const int32_t *widths, int CL) { return chain_embed_supported(K0, L, widths, CL); }

long long prifit_mlp_chain_embed_workspace(long long, int, int, const int32_t *, int) { return 0; }     // likewise

int prifit_mlp_chain_embed_f32(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                               const float *const *W, const long long *ldw, const float *const *b, const float *W_cls,
                               long long ldw_cls, const float *b_cls, int CL, float *emb, long long lde, int normalize, float *scores,
                               long long lds, int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat,
                               int rows_per_shape, float *, void *stream)
{
    return chain_embed_run<PipeF32>(X, ldx, P, K0, L, widths, W, ldw, b, W_cls, ldw_cls, b_cls, CL, emb, lde, normalize, scores, lds,
                                    labels, cat_of_label, shape_cat, rows_per_shape, stream);
}

}  // extern "C"
