// The per-POINT half of the reference's provider.py in ONE launch: clipped Gaussian jitter (:265-276) and random point dropout
// (:320-327), on top of the per-shape affine map of csrc/augment.hip -- now with the normals of a [B, M, 6] batch rotated along
// (:150-194, :216-236).  The random numbers come from a counter-based generator (Philox4x32-10, key = the seed, counter = (point,
// shape, stream, 0)): no state, no atomics, the same bits for every launch geometry.
//
// Grid (x, y) = (workgroups of a shape, shape).  A workgroup takes tiles of 256 points, tile = blockIdx.x, + gridDim.x, ...: the
// 256 * C contiguous floats of the channels-last source go coalesced (float4 where the tile's first float is 16-byte aligned)
// into LDS rows padded to an odd stride, thread i computes point i of the tile, the channels-first rows are written 256
// contiguous floats per channel and the channels-last output goes back through LDS the way it came.  12-24 bytes in and as many
// out per point against ~100 integer multiplies and a handful of transcendental calls: bound by memory and, at the sizes of a
// training batch (1.4 MB), by the launch itself.
//
// Dropout overwrites a dropped point with the OUTPUT of point 0 of its shape.  No workgroup waits for the one that owns point 0:
// each recomputes that output from point 0's source before its first tile.  In place that source is overwritten by whoever owns
// tile 0, so there ONE workgroup takes the whole shape (gridDim.x = 1): it has read point 0 before it writes anything.
// Every rounding is spelled out (__fmul_rn / __fadd_rn) and the file is built with -ffp-contract=off.
#include "common.h"

namespace {

constexpr int PTB_BLOCK = 256;
constexpr unsigned PTB_STREAM_JITTER = 0, PTB_STREAM_DROPOUT = 1;

struct PerturbArgs {
    const float *src;
    const float *affine;       // NULL: channels 0..2 are bit copies
    const float *drop_ratio;   // NULL: no dropout
    float *dst_cl, *dst_cf;
    int M, n_tiles;
    int rotate_normals;
    float sigma, clip;         // sigma == 0: no jitter
    unsigned seed_lo, seed_hi;
};

struct U4 {
    unsigned w[4];
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ U4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return U4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float unit24(unsigned w) { return __fmul_rn((float)(w >> 8), 0x1p-24f); }          // [0, 1), exact
__device__ __forceinline__ float unit24_open(unsigned w) { return __fmul_rn((float)((w >> 8) + 1), 0x1p-24f); }  // (0, 1], exact

__device__ __forceinline__ float clipped(float sigma, float clip, float z)
{
    return fminf(fmaxf(__fmul_rn(sigma, z), -clip), clip);
}

// the three jitter offsets of point p of shape b
__device__ __forceinline__ void jitter3(const PerturbArgs &a, unsigned p, unsigned b, float *j)
{
    const U4 x = philox4x32_10(p, b, PTB_STREAM_JITTER, 0u, a.seed_lo, a.seed_hi);
    const float two_pi = 6.2831855f;                                // fp32(2 pi) = 0x40C90FDB
    const float r01 = sqrtf(__fmul_rn(-2.0f, logf(unit24_open(x.w[0])))), th01 = __fmul_rn(two_pi, unit24(x.w[1]));
    const float r2 = sqrtf(__fmul_rn(-2.0f, logf(unit24_open(x.w[2])))), th2 = __fmul_rn(two_pi, unit24(x.w[3]));
    j[0] = clipped(a.sigma, a.clip, __fmul_rn(r01, cosf(th01)));
    j[1] = clipped(a.sigma, a.clip, __fmul_rn(r01, sinf(th01)));
    j[2] = clipped(a.sigma, a.clip, __fmul_rn(r2, cosf(th2)));
}

__device__ __forceinline__ bool dropped(const PerturbArgs &a, unsigned p, unsigned b, float ratio)
{
    return unit24(philox4x32_10(p, b, PTB_STREAM_DROPOUT, 0u, a.seed_lo, a.seed_hi).w[0]) <= ratio;
}

// point p of shape b before dropout: q[C] in (the source channels), q[C] out
template <int C>
__device__ __forceinline__ void transform(const PerturbArgs &a, const float *A, unsigned p, unsigned b, float *q)
{
    if (a.affine) {
        const float p0 = q[0], p1 = q[1], p2 = q[2];
#pragma unroll
        for (int j = 0; j < 3; ++j)
            q[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(p0, A[j]), __fmul_rn(p1, A[3 + j])), __fmul_rn(p2, A[6 + j])), A[9 + j]);
        if (C == 6 && a.rotate_normals) {
            const float n0 = q[3], n1 = q[4], n2 = q[5];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                q[3 + j] = __fadd_rn(__fadd_rn(__fmul_rn(n0, A[j]), __fmul_rn(n1, A[3 + j])), __fmul_rn(n2, A[6 + j]));
        }
    }
    if (a.sigma > 0.0f) {
        float j[3];
        jitter3(a, p, b, j);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = __fadd_rn(q[k], j[k]);
    }
}

// n contiguous floats between global memory and the padded LDS tile (element e = point e / C, channel e % C)
template <int C, bool TO_LDS>
__device__ __forceinline__ void stage(float *g, float *s, int n)
{
    constexpr int CP = C | 1;
    const int t = threadIdx.x;
    const int n4 = (((uintptr_t)g) & 15) == 0 ? n >> 2 : 0;
    for (int v = t; v < n4; v += PTB_BLOCK) {
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
    for (int e = 4 * n4 + t; e < n; e += PTB_BLOCK) {
        const int at = (e / C) * CP + e % C;
        if (TO_LDS) s[at] = g[e]; else g[e] = s[at];
    }
}

template <int C>
__global__ __launch_bounds__(PTB_BLOCK) void perturb_points_kernel(PerturbArgs a)
{
    constexpr int CP = C | 1;
    __shared__ float tile[PTB_BLOCK * CP];
    const int b = blockIdx.y, t = threadIdx.x;
    float A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = a.affine ? a.affine[(size_t)b * 12 + k] : 0.0f;

    // what a dropped point becomes: the output of point 0, formed here from its SOURCE (before this workgroup writes anything)
    float first[C], ratio = 0.0f;
    if (a.drop_ratio) {
        ratio = a.drop_ratio[b];
        const float *q = a.src + (size_t)b * a.M * C;
#pragma unroll
        for (int c = 0; c < C; ++c) first[c] = q[c];
        transform<C>(a, A, 0u, (unsigned)b, first);
    }

    for (int tl = blockIdx.x; tl < a.n_tiles; tl += gridDim.x) {
        const int m0 = tl * PTB_BLOCK, cnt = min(PTB_BLOCK, a.M - m0);
        const size_t at = ((size_t)b * a.M + m0) * C;
        stage<C, true>(const_cast<float *>(a.src) + at, tile, cnt * C);
        __syncthreads();
        if (t < cnt) {
            float *row = tile + t * CP, q[C];
#pragma unroll
            for (int c = 0; c < C; ++c) q[c] = row[c];
            const unsigned p = (unsigned)(m0 + t);
            if (a.drop_ratio && dropped(a, p, (unsigned)b, ratio)) {
#pragma unroll
                for (int c = 0; c < C; ++c) q[c] = first[c];
            } else {
                transform<C>(a, A, p, (unsigned)b, q);
            }
            if (a.dst_cf) {
                float *col = a.dst_cf + (size_t)b * C * a.M + m0 + t;
#pragma unroll
                for (int c = 0; c < C; ++c) col[(size_t)c * a.M] = q[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) row[c] = q[c];      // this thread's own row: nobody else reads it before the barrier
        }
        __syncthreads();
        if (a.dst_cl) {
            stage<C, false>(a.dst_cl + at, tile, cnt * C);
            __syncthreads();                                // the next tile's loads overwrite the LDS rows
        }
    }
}

}  // namespace

extern "C" int prifit_perturb_points(const float *src, int B, int M, int C, const float *affine, int rotate_normals, float sigma,
                                     float clip, const float *drop_ratio, uint32_t seed_lo, uint32_t seed_hi, float *dst_cl,
                                     float *dst_cf, void *stream)
{
    if (!src || B <= 0 || B > 65535 || M <= 0 || (C != 3 && C != 6) || (!dst_cl && !dst_cf) || dst_cf == src ||
        (dst_cf && dst_cf == dst_cl) || (rotate_normals && (C != 6 || !affine)) || !(sigma >= 0.0f) || (sigma > 0.0f && !(clip > 0.0f)))
        return PRIFIT_EINVAL;
    const int n_tiles = (M + PTB_BLOCK - 1) / PTB_BLOCK;
    PerturbArgs a{src, affine, drop_ratio, dst_cl, dst_cf, M, n_tiles, rotate_normals, sigma, clip, seed_lo, seed_hi};
    // in place with dropout: one workgroup per shape, so point 0's source is read before anyone overwrites it
    const dim3 grid(drop_ratio && dst_cl == src ? 1 : n_tiles, B);
    if (C == 3)
        hipLaunchKernelGGL(perturb_points_kernel<3>, grid, dim3(PTB_BLOCK), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(perturb_points_kernel<6>, grid, dim3(PTB_BLOCK), 0, as_stream(stream), a);
    return prifit_check_launch();
}
