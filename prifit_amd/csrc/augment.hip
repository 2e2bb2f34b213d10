// Batch augmentation in ONE launch: a per-shape affine map of the first three channels, the channels-last -> channels-first
// layout change and the gather of the model's input subset (pretrain_partseg_shapenet.py:321-351: random_scale, shift,
// anisotropic scale and the two y rotations of provider.py compose into one 3x4 matrix per shape; the transpose of :342 and the
// `chamfer_points[:, :, choice]` of :351 follow).  As torch operators that is ~10 launches over a 1.4 MB batch (B 24, M 5000).
//
// Grid (x, y) = (blocks, shape).  The first `n_main` blocks of a shape take 256 points each: the 256 * C contiguous floats of the
// channels-last source are loaded coalesced (float4 where the block's first float is 16-byte aligned, scalar otherwise) into LDS,
// thread i transforms point i, the channels-first rows are written 256 contiguous floats per channel, and the channels-last
// output goes back through LDS the way it came.  LDS rows are padded to an odd stride (C | 1), so the per-point reads of
// threads i, i + 1, ... fall on different banks for every C.  The blocks behind them take 256 subset columns each: a 4 * C
// byte read at a random point per thread, coalesced row writes.  The 12 affine floats are uniform per block (blockIdx.y).
// No atomics, plain vector stores; every rounding is spelled out (__fmul_rn / __fadd_rn), so the bits do not depend on contraction.
#include "common.h"

namespace {

constexpr int AFF_BLOCK = 256;

struct AffineArgs {
    const float *src;
    const float *affine;
    const int32_t *subset;
    float *dst_cl, *dst_cf, *dst_sub;
    int M, n_subset;
    int n_main;                // blocks per shape that take points; the rest take subset columns
};

__device__ __forceinline__ void affine_xyz(const float *A, float p0, float p1, float p2, float *o)
{
#pragma unroll
    for (int j = 0; j < 3; ++j)
        o[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(p0, A[j]), __fmul_rn(p1, A[3 + j])), __fmul_rn(p2, A[6 + j])), A[9 + j]);
}

// n contiguous floats between global memory and the padded LDS tile (element e = point e / C, channel e % C)
template <int C, bool TO_LDS>
__device__ __forceinline__ void stage(float *g, float *s, int n)
{
    constexpr int CP = C | 1;
    const int t = threadIdx.x;
    if ((((uintptr_t)g) & 15) == 0) {
        const int n4 = n >> 2;
        for (int v = t; v < n4; v += AFF_BLOCK) {
            float4 x;
            float *xs = &x.x;
            if (TO_LDS) x = reinterpret_cast<const float4 *>(g)[v];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * v + k, at = (e / C) * CP + e % C;
                if (TO_LDS) s[at] = xs[k]; else xs[k] = s[at];
            }
            if (!TO_LDS) reinterpret_cast<float4 *>(g)[v] = x;
        }
        for (int e = 4 * n4 + t; e < n; e += AFF_BLOCK) {
            const int at = (e / C) * CP + e % C;
            if (TO_LDS) s[at] = g[e]; else g[e] = s[at];
        }
    } else {
        for (int e = t; e < n; e += AFF_BLOCK) {
            const int at = (e / C) * CP + e % C;
            if (TO_LDS) s[at] = g[e]; else g[e] = s[at];
        }
    }
}

template <int C>
__global__ __launch_bounds__(AFF_BLOCK) void affine_points_kernel(AffineArgs a)
{
    constexpr int CP = C | 1;
    __shared__ float tile[AFF_BLOCK * CP];
    const int b = blockIdx.y, t = threadIdx.x;
    float A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = a.affine[(size_t)b * 12 + k];

    if ((int)blockIdx.x < a.n_main) {
        const int m0 = blockIdx.x * AFF_BLOCK, cnt = min(AFF_BLOCK, a.M - m0);
        const size_t first = ((size_t)b * a.M + m0) * C;
        stage<C, true>(const_cast<float *>(a.src) + first, tile, cnt * C);
        __syncthreads();
        if (t < cnt) {
            float *p = tile + t * CP, o[3];
            affine_xyz(A, p[0], p[1], p[2], o);
            if (a.dst_cf) {
                float *row = a.dst_cf + (size_t)b * C * a.M + m0 + t;
#pragma unroll
                for (int c = 0; c < C; ++c) row[(size_t)c * a.M] = c < 3 ? o[c] : p[c];
            }
            p[0] = o[0], p[1] = o[1], p[2] = o[2];      // this thread's own row: nobody else reads it before the barrier
        }
        if (a.dst_cl) {
            __syncthreads();
            stage<C, false>(a.dst_cl + first, tile, cnt * C);
        }
        return;
    }
    const int j = ((int)blockIdx.x - a.n_main) * AFF_BLOCK + t;
    if (j >= a.n_subset) return;
    const int idx = a.subset[j];
    float p[C], o[3];
    if ((unsigned)idx < (unsigned)a.M) {
        const float *q = a.src + ((size_t)b * a.M + idx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = q[c];
        affine_xyz(A, p[0], p[1], p[2], o);
    } else {                                            // outside the caller's contract: nothing is read, the column shows it
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = __builtin_nanf("");
        o[0] = o[1] = o[2] = p[0];
    }
    float *col = a.dst_sub + (size_t)b * C * a.n_subset + j;
#pragma unroll
    for (int c = 0; c < C; ++c) col[(size_t)c * a.n_subset] = c < 3 ? o[c] : p[c];
}

int launch(int C, dim3 grid, hipStream_t st, const AffineArgs &a)
{
    switch (C) {
    case 3: hipLaunchKernelGGL(affine_points_kernel<3>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    case 4: hipLaunchKernelGGL(affine_points_kernel<4>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    case 5: hipLaunchKernelGGL(affine_points_kernel<5>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    case 6: hipLaunchKernelGGL(affine_points_kernel<6>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    case 7: hipLaunchKernelGGL(affine_points_kernel<7>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    default: hipLaunchKernelGGL(affine_points_kernel<8>, grid, dim3(AFF_BLOCK), 0, st, a); break;
    }
    return prifit_check_launch();
}

}  // namespace

extern "C" int prifit_affine_points(const float *src, int B, int M, int C, const float *affine, const int32_t *subset, int n_subset,
                                    float *dst_cl, float *dst_cf, float *dst_sub, void *stream)
{
    if (!src || !affine || B <= 0 || B > 65535 || M <= 0 || C < 3 || C > 8 || (!dst_cl && !dst_cf && !dst_sub) ||
        (dst_sub && (!subset || n_subset <= 0)) || dst_cf == src)
        return PRIFIT_EINVAL;
    const int n_main = (dst_cl || dst_cf) ? (M + AFF_BLOCK - 1) / AFF_BLOCK : 0;
    const int n_sub = dst_sub ? (n_subset + AFF_BLOCK - 1) / AFF_BLOCK : 0;
    AffineArgs a{src, affine, subset, dst_cl, dst_cf, dst_sub, M, dst_sub ? n_subset : 0, n_main};
    if (dst_cl == src && n_sub) {
        // in place: the subset columns read the source, so they go first on the stream, in a launch of their own
        AffineArgs s = a;
        s.n_main = 0;
        const int rc = launch(C, dim3(n_sub, B), as_stream(stream), s);
        if (rc != PRIFIT_OK) return rc;
        return launch(C, dim3(n_main, B), as_stream(stream), a);
    }
    return launch(C, dim3(n_main + n_sub, B), as_stream(stream), a);
}
