// Point-set Chamfer distance between two batched, ragged clouds: exact nearest neighbour (forward) and its gradient to both
// clouds (backward).  Replaces the pairwise matrix + min of src/utils.py:271-358 (chamfer_distance,
// chamfer_distance_one_side, chamfer_distance_single_shape) and the host KD-tree of :361-381 / :413-416.
//
// Arithmetic is fp32 in one fixed order, compiled with -ffp-contract=off (no fma), so a numpy restatement reproduces
// every output bit for bit (tests/chamfer_common.py):
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz),  dx = a.x - b.x ...          (direct differences)
//   idx(i)   = the lowest j attaining the minimum
//   ga(i)    = (2 g(i)) * (a(i) - b(idx(i)))                           per component
//   gb(j)    = ((0 - ga(i0)) - ga(i1)) - ...  over the i with idx(i) == j in ascending order
// No floating-point atomics anywhere: the same bits from run to run.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int CH_THREADS = 256;   // one query (forward) / one target (backward) per thread
constexpr int CH_TILE = 256;      // targets staged in LDS per step: 3 KB, never the whole cloud
constexpr int CH_MAX_SPLIT = 32;  // ranges the targets of one shape are cut into (gridDim.y)
constexpr int CH_BWD_TILE = 1024; // queries (index + gradient row) staged in LDS per step of the backward: 16 KB

// Ranges the target cloud is cut into.  One workgroup searches 256 queries against one range; the search is a serial loop
// per thread, so the launch wants ~4 workgroups per CU (256 CUs) to fill the chip: B = 24, NA = 10000 has 960 query blocks
// -> 2 ranges; B = 1 has 40 -> 16 ranges of 313 targets at NB = 5000 (640 workgroups).  A range is never shorter than one
// LDS tile.  Pure function of the sizes: the workspace query and both kernels use the same value.
int chamfer_split(int B, int NA, int NB)
{
    const long long blocks = (long long)B * ((NA + CH_THREADS - 1) / CH_THREADS);
    int split = 1;
    while (split < CH_MAX_SPLIT && blocks * split < 1024 && NB / (2 * split) >= CH_TILE) split *= 2;
    return split;
}

__device__ __forceinline__ int live_count(const int32_t *cnt, int s, int full)
{
    return cnt ? min(max(cnt[s], 0), full) : full;
}

// One range of targets for 256 queries.  Every lane reads the same LDS address per step (a broadcast: no bank conflict).
// split == 1: writes d2 / idx; otherwise the (distance, index) candidate of the range goes to ws [B][split][NA].
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_fwd_kernel(
    const float *__restrict__ a, const float *__restrict__ b, const int32_t *__restrict__ na_p,
    const int32_t *__restrict__ nb_p, int NA, int NB, int split, float *__restrict__ d2, int32_t *__restrict__ idx,
    float2 *__restrict__ ws)
{
    // one array per coordinate: four targets come out of LDS as three 16-byte broadcast reads
    __shared__ __attribute__((aligned(16))) float s_x[CH_TILE], s_y[CH_TILE], s_z[CH_TILE];
    const int s = blockIdx.z, z = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    const int na = live_count(na_p, s, NA), nb = live_count(nb_p, s, NB);
    const bool row = i < NA;
    const bool live = i < na && nb > 0;
    if (split == 1 && (blockIdx.x * CH_THREADS >= na || nb == 0)) {   // block-uniform: nothing to search
        if (row) { d2[(size_t)s * NA + i] = 0.f; idx[(size_t)s * NA + i] = -1; }
        return;
    }
    const int chunk = (nb + split - 1) / split;
    const int m_lo = z * chunk, m_hi = min(nb, m_lo + chunk);
    if (split > 1 && (blockIdx.x * CH_THREADS >= na || m_lo >= m_hi)) return;   // block-uniform; the pick kernel skips it too

    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) {
        const float *p = a + ((size_t)s * NA + i) * 3;
        px = p[0]; py = p[1]; pz = p[2];
    }
    const float *T = b + (size_t)s * NB * 3;
    float best = INFINITY;
    int bi = m_lo;
    for (int base = m_lo; base < m_hi; base += CH_TILE) {
        const int tn = min(CH_TILE, m_hi - base);
        __syncthreads();
        {
            // slots past the range repeat its last target: a repeat comes later and never wins the strict comparison
            const int ii = base + min((int)threadIdx.x, tn - 1);
            s_x[threadIdx.x] = T[(size_t)ii * 3]; s_y[threadIdx.x] = T[(size_t)ii * 3 + 1]; s_z[threadIdx.x] = T[(size_t)ii * 3 + 2];
        }
        __syncthreads();
        const int tn4 = (tn + 3) & ~3;
        for (int j = 0; j < tn4; j += 4) {
            const float4 tx4 = *reinterpret_cast<const float4 *>(s_x + j), ty4 = *reinterpret_cast<const float4 *>(s_y + j),
                         tz4 = *reinterpret_cast<const float4 *>(s_z + j);
            const float tx[4] = {tx4.x, tx4.y, tx4.z, tx4.w}, ty[4] = {ty4.x, ty4.y, ty4.z, ty4.w},
                        tz[4] = {tz4.x, tz4.y, tz4.z, tz4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float dx = px - tx[u], dy = py - ty[u], dz = pz - tz[u];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < best) { best = d; bi = base + j + u; }
            }
        }
    }
    if (split == 1) {
        if (row) {
            d2[(size_t)s * NA + i] = live ? best : 0.f;
            idx[(size_t)s * NA + i] = live ? bi : -1;
        }
    } else if (live) {
        ws[((size_t)s * split + z) * NA + i] = make_float2(best, __int_as_float(bi));
    }
}

// first minimum over the ranges in ascending order: the neighbour the unsplit loop finds
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_pick_kernel(
    const float2 *__restrict__ ws, const int32_t *__restrict__ na_p, const int32_t *__restrict__ nb_p, int NA, int NB,
    int split, float *__restrict__ d2, int32_t *__restrict__ idx)
{
    const int s = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= NA) return;
    const int na = live_count(na_p, s, NA), nb = live_count(nb_p, s, NB);
    float best = 0.f;
    int bi = -1;
    if (i < na && nb > 0) {
        const int chunk = (nb + split - 1) / split;
        best = INFINITY;
        bi = 0;
        for (int z = 0; z < split; ++z) {
            if (z * chunk >= nb) break;
            const float2 e = ws[((size_t)s * split + z) * NA + i];
            if (e.x < best) { best = e.x; bi = __float_as_int(e.y); }
        }
    }
    d2[(size_t)s * NA + i] = best;
    idx[(size_t)s * NA + i] = bi;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_bwd_a_kernel(
    const float *__restrict__ a, const float *__restrict__ b, const int32_t *__restrict__ na_p, int NA, int NB,
    const int32_t *__restrict__ idx, const float *__restrict__ g, float *__restrict__ ga)
{
    const int s = blockIdx.y;
    const int i = blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= NA) return;
    const int na = live_count(na_p, s, NA);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const size_t r = (size_t)s * NA + i;
    if (i < na) {
        const int j = idx[r];
        if (j >= 0 && j < NB) {
            const float *p = a + r * 3, *q = b + ((size_t)s * NB + j) * 3;
            const float t = 2.f * g[r];
            gx = t * (p[0] - q[0]); gy = t * (p[1] - q[1]); gz = t * (p[2] - q[2]);
        }
    }
    ga[r * 3] = gx; ga[r * 3 + 1] = gy; ga[r * 3 + 2] = gz;
}

// One thread per target row; the shape's (idx, ga) rows pass through LDS in order.  A wave looks at 64 indices per step
// (one per lane), a ballot finds the ones that point into its own 64 targets, and those are taken in ascending order: the
// owning lane subtracts the ga row (an LDS broadcast read).  NA / 64 steps per wave plus one step per referencing query.
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_bwd_b_kernel(
    const int32_t *__restrict__ na_p, int NA, int NB, const int32_t *__restrict__ idx, const float *__restrict__ ga,
    float *__restrict__ gb, int accumulate)
{
    __shared__ int32_t s_idx[CH_BWD_TILE];
    __shared__ float s_g[CH_BWD_TILE * 3];
    const int s = blockIdx.y;
    const int j = blockIdx.x * CH_THREADS + threadIdx.x;
    const int j0w = j - lane_id();   // first target of this wave
    const int na = live_count(na_p, s, NA);
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int base = 0; base < na; base += CH_BWD_TILE) {
        const int tn = min(CH_BWD_TILE, na - base);
        __syncthreads();
        for (int k = threadIdx.x; k < tn; k += CH_THREADS) s_idx[k] = idx[(size_t)s * NA + base + k];
        for (int k = threadIdx.x; k < tn * 3; k += CH_THREADS) s_g[k] = ga[((size_t)s * NA + base) * 3 + k];
        __syncthreads();
        for (int c = 0; c < tn; c += 64) {
            const int k = c + lane_id();
            const int id = k < tn ? s_idx[k] : -1;
            unsigned long long m = __ballot((unsigned)(id - j0w) < 64u && id >= 0);
            while (m) {
                const int k1 = c + __ffsll((long long)m) - 1;
                m &= m - 1;
                if (s_idx[k1] == j) {
                    ax = ax - s_g[k1 * 3]; ay = ay - s_g[k1 * 3 + 1]; az = az - s_g[k1 * 3 + 2];
                }
            }
        }
    }
    if (j < NB) {
        float *o = gb + ((size_t)s * NB + j) * 3;
        if (accumulate) { ax = o[0] + ax; ay = o[1] + ay; az = o[2] + az; }
        o[0] = ax; o[1] = ay; o[2] = az;
    }
}

bool chamfer_sizes_ok(int B, int NA, int NB)
{
    return B > 0 && B <= 65535 && NA >= 0 && NB >= 0 && (long long)B * NA * 3 <= INT_MAX && (long long)B * NB * 3 <= INT_MAX;
}

}  // namespace

extern "C" {

long long prifit_chamfer_nn_workspace_floats(int B, int NA, int NB)
{
    if (!chamfer_sizes_ok(B, NA, NB)) return 0;
    const int split = chamfer_split(B, NA, NB);
    return split > 1 ? 2LL * split * B * NA : 0;
}

int prifit_chamfer_nn_fwd(const float *a, const float *b, const int32_t *na, const int32_t *nb, int B, int NA, int NB,
                          float *d2, int32_t *idx, float *workspace, void *stream)
{
    if (!a || !b || !d2 || !idx || !chamfer_sizes_ok(B, NA, NB)) return PRIFIT_EINVAL;
    if (NA == 0) return PRIFIT_OK;
    const int split = chamfer_split(B, NA, NB);
    if (split > 1 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7))) return PRIFIT_EINVAL;
    hipStream_t st = as_stream(stream);
    const int qb = (NA + CH_THREADS - 1) / CH_THREADS;
    float2 *ws = reinterpret_cast<float2 *>(workspace);
    hipLaunchKernelGGL(chamfer_nn_fwd_kernel, dim3(qb, split, B), dim3(CH_THREADS), 0, st, a, b, na, nb, NA, NB, split, d2,
                       idx, ws);
    if (split > 1)
        hipLaunchKernelGGL(chamfer_nn_pick_kernel, dim3(qb, B), dim3(CH_THREADS), 0, st, ws, na, nb, NA, NB, split, d2, idx);
    return prifit_check_launch();
}

int prifit_chamfer_nn_bwd(const float *a, const float *b, const int32_t *na, const int32_t *nb, int B, int NA, int NB,
                          const int32_t *idx, const float *g, float *ga, float *gb, int accumulate_b, void *stream)
{
    (void)nb;   // rows of gb at or past nb[s] are referenced by no index: they get zero like any unreferenced row
    if (!a || !b || !idx || !g || !ga || !gb || !chamfer_sizes_ok(B, NA, NB)) return PRIFIT_EINVAL;
    hipStream_t st = as_stream(stream);
    if (NA > 0)
        hipLaunchKernelGGL(chamfer_nn_bwd_a_kernel, dim3((NA + CH_THREADS - 1) / CH_THREADS, B), dim3(CH_THREADS), 0, st, a, b,
                           na, NA, NB, idx, g, ga);
    if (NB > 0)
        hipLaunchKernelGGL(chamfer_nn_bwd_b_kernel, dim3((NB + CH_THREADS - 1) / CH_THREADS, B), dim3(CH_THREADS), 0, st, na, NA,
                           NB, idx, ga, gb, accumulate_b ? 1 : 0);
    return prifit_check_launch();
}

}  // extern "C"
