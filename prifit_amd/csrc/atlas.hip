// Chart-batched AtlasNet decoder (models/reconstruction.py:8-70 of the reference): every chart's four 1x1 convolutions, three
// BatchNorms and the tanh, forward and backward, in a number of launches that depends on neither the chart count nor B.
//
// Per chart c and row (b, p) of the B * P positions:
//   y1 = W1[:, :2] . grid_p + (W1[:, 2:] . z_b + b1)      the [B,130,P] input is never formed; the z part is H [C,B,130]
//   x1 = relu(bn1(y1));  y2 = W2 x1 + b2;  x2 = relu(bn2(y2));  y3 = W3 x2 + b3;  x3 = relu(bn3(y3));  out = tanh(W4 x3 + b4)
// bn1 statistics come from the two parts of y1 (the cross term sums to zero): mean = mean_p + mean_b, var = var_p + var_b.
// x1 is recomputed where it is consumed; y2 and y3 are the only activations stored.
//
// Tiling: a workgroup owns 32 consecutive grid points of ONE shape (tile t -> b = t / TPB, p0 = 32 (t % TPB)), so the z part
// is one vector per tile.  The 130->65, 65->32 products and their backward products run on v_mfma_f32_16x16x4_f32 from
// zero-padded LDS tiles (130, 65, 121 are multiples of nothing: pad columns hold zeros or their lane index is clamped onto a
// zero / discarded column).  BatchNorm sums leave the product kernels as per-tile partials (sum and centred sum of squares)
// and are merged in tile order in fp64 by the consumer: no floating-point atomics, the same bits from run to run.
// Weight gradients accumulate in MFMA registers over the tiles of a row group (at most 16 groups per chart) and the group
// partials are summed in group order by the finish kernel.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int AT_Z = 128;                       // latent width
constexpr int AT_D1 = 130, AT_D2 = 65, AT_D3 = 32;
constexpr int AT_TM = 32;                       // rows per tile
constexpr int AT_THREADS = 256;                 // 4 waves
constexpr int AT_S1 = 132;                      // LDS row stride of a 130-wide tile (k padded to a multiple of 4)
constexpr int AT_S2 = 68;                       // ... of a 65-wide tile
constexpr int AT_NPTR = 24;                     // pointers per chart in the parameter table
constexpr int AT_LD = 132;                      // stride of the per-layer channel vectors in the workspace
constexpr int AT_MAXG = 16;                     // row groups per chart in the backward
constexpr int AT_BT = 8;                        // shapes per workgroup in the latent product
constexpr int AT_NPARAM = 28210;                // parameters of one chart = floats of one chart's gradient block

// slots of the parameter table
enum { P_W1, P_B1, P_W2, P_B2, P_W3, P_B3, P_W4, P_B4, P_G1, P_BE1, P_RM1, P_RV1, P_G2, P_BE2, P_RM2, P_RV2, P_G3, P_BE3,
       P_RM3, P_RV3, P_NBT1, P_NBT2, P_NBT3 };
// offsets inside a chart's gradient block: the order of the module's parameters
constexpr int G_W1 = 0, G_B1 = 16900, G_W2 = 17030, G_B2 = 25480, G_W3 = 25545, G_B3 = 27625, G_W4 = 27657, G_B4 = 27753,
              G_G1 = 27756, G_BE1 = 27886, G_G2 = 28016, G_BE2 = 28081, G_G3 = 28146, G_BE3 = 28178;
static_assert(G_BE3 + AT_D3 == AT_NPARAM, "gradient block layout");
// the finish kernel writes a weight and the bias behind it as one run
static_assert(G_W2 + AT_D2 * AT_D1 == G_B2 && G_W3 + AT_D3 * AT_D2 == G_B3 && G_W4 + 3 * AT_D3 == G_B4, "bias follows its weight");

constexpr int PW2_N = AT_D2 * AT_D1 + AT_D2, PW3_N = AT_D3 * AT_D2 + AT_D3, PW4_N = 3 * AT_D3 + 3;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Dims {
    int C, B, P, TPB, T, R, NG;
};

// forward workspace (kept for the backward) and backward scratch: offsets in floats
struct FwdWs {
    size_t H, AB, SV, Y2, Y3, PS2, PS3, total;
};
struct BwdWs {
    size_t G3, G2, Q3, Q2, Q1, PW4, PW3, PW2, DH, total;
};

Dims make_dims(int C, int B, int P)
{
    Dims d;
    d.C = C; d.B = B; d.P = P;
    d.TPB = (P + AT_TM - 1) / AT_TM;
    d.T = B * d.TPB;
    d.R = B * P;
    d.NG = d.T < AT_MAXG ? d.T : AT_MAXG;
    return d;
}

FwdWs fwd_ws(const Dims &d)
{
    FwdWs w;
    size_t o = 0;
    w.H = o;   o += (size_t)d.C * d.B * AT_D1;
    w.AB = o;  o += (size_t)d.C * 6 * AT_LD;
    w.SV = o;  o += (size_t)d.C * 6 * AT_LD;
    w.Y2 = o;  o += (size_t)d.C * d.R * AT_D2;
    w.Y3 = o;  o += (size_t)d.C * d.R * AT_D3;
    w.PS2 = o; o += (size_t)d.C * d.T * 2 * AT_D2;
    w.PS3 = o; o += (size_t)d.C * d.T * 2 * AT_D3;
    w.total = o;
    return w;
}

BwdWs bwd_ws(const Dims &d)
{
    BwdWs w;
    size_t o = 0;
    w.G3 = o;  o += (size_t)d.C * d.R * AT_D3;
    w.G2 = o;  o += (size_t)d.C * d.R * AT_D2;
    w.Q3 = o;  o += (size_t)d.C * d.T * 2 * AT_D3;
    w.Q2 = o;  o += (size_t)d.C * d.T * 2 * AT_D2;
    w.Q1 = o;  o += (size_t)d.C * d.T * 4 * AT_D1;
    w.PW4 = o; o += (size_t)d.C * d.NG * PW4_N;
    w.PW3 = o; o += (size_t)d.C * d.NG * PW3_N;
    w.PW2 = o; o += (size_t)d.C * d.NG * PW2_N;
    w.DH = o;  o += (size_t)d.C * d.B * AT_D1;
    w.total = o;
    return w;
}

bool dims_ok(int C, int B, int P)
{
    if (C <= 0 || C > 65534 || B <= 0 || P <= 0) return false;
    const long long R = (long long)B * P;
    return R * C * AT_D1 <= INT_MAX && (long long)B * ((P + AT_TM - 1) / AT_TM) <= INT_MAX / 1024;
}

__device__ __forceinline__ const float *tabf(const void *const *tab, int c, int slot)
{
    return static_cast<const float *>(tab[(size_t)c * AT_NPTR + slot]);
}
__device__ __forceinline__ float *tabw(const void *const *tab, int c, int slot)
{
    return static_cast<float *>(const_cast<void *>(tab[(size_t)c * AT_NPTR + slot]));
}

__device__ __forceinline__ int tile_rows(int t, int TPB, int P) { return min(AT_TM, P - (t % TPB) * AT_TM); }

// y1 of one (row, channel): the same expression in the forward and in the backward, so that the relu mask is the same.  The
// fused multiply-adds are written out: what the compiler contracts may differ from one kernel to the next.
__device__ __forceinline__ float x1_pre(float w0, float w1, float u, float v, float h) { return fmaf(w1, v, w0 * u) + h; }
// bn + relu as a (y - mean) + beta, a = gamma / sqrt(var + eps): the difference first, so that a column whose variance is ~0
// (a large a) does not lose its value in the cancellation of a y against a mean
__device__ __forceinline__ float bn_relu(float a, float mu, float beta, float y) { return fmaxf(fmaf(a, y - mu, beta), 0.f); }

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// mean and 1 / sqrt(var + eps) of one channel from the per-tile (sum, centred sum of squares) partials, merged in tile order
__device__ void merge_stats(const float *ps, int width, int ch, int T, int TPB, int P, int R, double &mean, double &var)
{
    double S = 0.0;
    for (int t = 0; t < T; ++t) S += (double)ps[((size_t)t * 2) * width + ch];
    mean = S / R;
    double M = 0.0;
    for (int t = 0; t < T; ++t) {
        const int n = tile_rows(t, TPB, P);
        const double d = (double)ps[((size_t)t * 2) * width + ch] / n - mean;
        M += (double)ps[((size_t)t * 2 + 1) * width + ch] + n * d * d;
    }
    var = M / R;
}

// scale / shift of a BatchNorm channel into (a, s); tile 0 of the chart also keeps them for the backward and, in training
// mode, moves the running statistics (biased variance normalises, unbiased variance is tracked)
__device__ void bn_channel(const void *const *tab, int c, int layer, int ch, bool training, bool owner, double mean, double var,
                           int R, float eps, float momentum, float *AB, float *SV, float &a, float &mu, float &beta)
{
    const int gs = P_G1 + 4 * layer;
    float *rm = tabw(tab, c, gs + 2), *rv = tabw(tab, c, gs + 3);
    float inv;
    if (training) {
        mu = (float)mean;
        inv = 1.f / sqrtf((float)var + eps);
        if (owner) {
            rm[ch] = (1.f - momentum) * rm[ch] + momentum * mu;
            rv[ch] = (1.f - momentum) * rv[ch] + momentum * (float)(var * ((double)R / (double)(R - 1)));
        }
    } else {
        mu = rm[ch];
        inv = 1.f / sqrtf(rv[ch] + eps);
    }
    a = tabf(tab, c, gs)[ch] * inv;
    beta = tabf(tab, c, gs + 1)[ch];
    if (owner) {
        float *ab = AB + ((size_t)c * 6 + layer * 2) * AT_LD, *sv = SV + ((size_t)c * 6 + layer * 2) * AT_LD;
        ab[ch] = a; ab[AT_LD + ch] = beta;
        sv[ch] = mu; sv[AT_LD + ch] = inv;
    }
}

// ------------------------------------------------------------------------------------------------------------- forward

// H[c][b][:] = W1[:, 2:] z_b + b1 for 8 shapes per workgroup
__global__ __launch_bounds__(AT_THREADS) void atlas_latent_kernel(const void *const *tab, const float *__restrict__ z, int B,
                                                                  float *__restrict__ H)
{
    __shared__ float zs[AT_BT][AT_Z];
    const int c = blockIdx.y, b0 = blockIdx.x * AT_BT, nb = min(AT_BT, B - b0);
    for (int i = threadIdx.x; i < AT_BT * AT_Z; i += AT_THREADS) {
        const int bb = i / AT_Z;
        zs[bb][i % AT_Z] = bb < nb ? z[(size_t)(b0 + bb) * AT_Z + i % AT_Z] : 0.f;
    }
    __syncthreads();
    const int ch = threadIdx.x;
    if (ch >= AT_D1) return;
    const float *W = tabf(tab, c, P_W1) + ch * AT_D1 + 2;
    float acc[AT_BT];
#pragma unroll
    for (int j = 0; j < AT_BT; ++j) acc[j] = 0.f;
    for (int k = 0; k < AT_Z; ++k) {
        const float w = W[k];
#pragma unroll
        for (int j = 0; j < AT_BT; ++j) acc[j] = fmaf(w, zs[j][k], acc[j]);
    }
    const float bias = tabf(tab, c, P_B1)[ch];
    for (int j = 0; j < nb; ++j) H[((size_t)c * B + b0 + j) * AT_D1 + ch] = acc[j] + bias;
}

// bn1 of every chart: one thread per channel, statistics of the grid part over p and of the latent part over b
__global__ __launch_bounds__(192) void atlas_bn1_kernel(const void *const *tab, const float *__restrict__ grid, Dims d,
                                                         int training, float eps, float momentum, const float *__restrict__ H,
                                                         float *__restrict__ AB, float *__restrict__ SV)
{
    const int c = blockIdx.x, ch = threadIdx.x;
    if (ch == 0 && training) {
        for (int l = 0; l < 3; ++l) *static_cast<long long *>(const_cast<void *>(tab[(size_t)c * AT_NPTR + P_NBT1 + l])) += 1;
    }
    if (ch >= AT_D1) return;
    double mean = 0.0, var = 0.0;
    if (training) {
        const float *W = tabf(tab, c, P_W1) + ch * AT_D1;
        const float w0 = W[0], w1 = W[1];
        double sp = 0.0, sb = 0.0;
        for (int p = 0; p < d.P; ++p) sp += (double)(w0 * grid[p] + w1 * grid[d.P + p]);
        for (int b = 0; b < d.B; ++b) sb += (double)H[((size_t)c * d.B + b) * AT_D1 + ch];
        const double mp = sp / d.P, mb = sb / d.B;
        double vp = 0.0, vb = 0.0;
        for (int p = 0; p < d.P; ++p) {
            const double e = (double)(w0 * grid[p] + w1 * grid[d.P + p]) - mp;
            vp += e * e;
        }
        for (int b = 0; b < d.B; ++b) {
            const double e = (double)H[((size_t)c * d.B + b) * AT_D1 + ch] - mb;
            vb += e * e;
        }
        mean = mp + mb;
        var = vp / d.P + vb / d.B;
    }
    float a, mu, beta;
    bn_channel(tab, c, 0, ch, training != 0, true, mean, var, d.R, eps, momentum, AB, SV, a, mu, beta);
}

// y2 tile = x1 tile [32 x 130] . W2^T [130 x 65] + b2, its column sums; x1 formed on load
__global__ __launch_bounds__(AT_THREADS) void atlas_l2_fwd_kernel(const void *const *tab, const float *__restrict__ grid, Dims d,
                                                                  int training, const float *__restrict__ H,
                                                                  const float *__restrict__ AB, const float *__restrict__ SV,
                                                                  float *__restrict__ Y2, float *__restrict__ PS2)
{
    __shared__ float Xs[AT_TM * AT_S1];          // x1, later the y2 tile [32][80]
    __shared__ float Ws[80 * AT_S1];             // W2, rows 65 .. 79 and columns 130, 131 zero
    __shared__ float w0s[AT_D1], w1s[AT_D1], as[AT_D1], ss[AT_D1], ms[AT_D1], hs[AT_D1];
    const int c = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
    const float *W1 = tabf(tab, c, P_W1), *W2 = tabf(tab, c, P_W2);
    if (tid < AT_D1) {
        w0s[tid] = W1[tid * AT_D1]; w1s[tid] = W1[tid * AT_D1 + 1];
        as[tid] = AB[(size_t)c * 6 * AT_LD + tid]; ss[tid] = AB[((size_t)c * 6 + 1) * AT_LD + tid];
        ms[tid] = SV[(size_t)c * 6 * AT_LD + tid];
        hs[tid] = H[((size_t)c * d.B + b) * AT_D1 + tid];
    }
    for (int i = tid; i < 80 * AT_S1; i += AT_THREADS) {
        const int r = i / AT_S1, k = i % AT_S1;
        Ws[i] = (r < AT_D2 && k < AT_D1) ? W2[r * AT_D1 + k] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < AT_TM * AT_S1; i += AT_THREADS) {
        const int r = i / AT_S1, k = i % AT_S1;
        float x = 0.f;
        if (r < nv && k < AT_D1) x = bn_relu(as[k], ms[k], ss[k], x1_pre(w0s[k], w1s[k], grid[p0 + r], grid[d.P + p0 + r], hs[k]));
        Xs[i] = x;
    }
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    f32x4 acc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int blk = wave + 4 * q;
        if (blk < 10) {
            const int mb = blk / 5, nb = blk % 5;
            const float *A = Xs + (mb * 16 + li) * AT_S1 + lk, *Bm = Ws + (nb * 16 + li) * AT_S1 + lk;
            for (int ks = 0; ks < AT_S1 / 4; ++ks) acc[q] = mfma4(A[ks * 4], Bm[ks * 4], acc[q]);
        }
    }
    __syncthreads();
    float *Ys = Xs;
    const float *b2 = tabf(tab, c, P_B2);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int blk = wave + 4 * q;
        if (blk < 10) {
            const int mb = blk / 5, nb = blk % 5, col = nb * 16 + li;
            const float bias = col < AT_D2 ? b2[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ys[(mb * 16 + lk * 4 + r) * 80 + col] = acc[q][r] + bias;
        }
    }
    __syncthreads();
    float *Yg = Y2 + ((size_t)c * d.R + (size_t)b * d.P + p0) * AT_D2;
    for (int i = tid; i < nv * AT_D2; i += AT_THREADS) Yg[i] = Ys[(i / AT_D2) * 80 + i % AT_D2];
    if (training && tid < AT_D2) {
        float s = 0.f;
        for (int r = 0; r < nv; ++r) s += Ys[r * 80 + tid];
        const float m = s / nv;
        float q = 0.f;
        for (int r = 0; r < nv; ++r) { const float e = Ys[r * 80 + tid] - m; q += e * e; }
        float *ps = PS2 + ((size_t)c * d.T + t) * 2 * AT_D2;
        ps[tid] = s; ps[AT_D2 + tid] = q;
    }
}

// bn2 (merged here from the partials) + relu on load, y3 tile = x2 [32 x 65] . W3^T [65 x 32] + b3, its column sums
__global__ __launch_bounds__(AT_THREADS) void atlas_l3_fwd_kernel(const void *const *tab, Dims d, int training, float eps,
                                                                  float momentum, const float *__restrict__ Y2,
                                                                  const float *__restrict__ PS2, float *__restrict__ AB,
                                                                  float *__restrict__ SV, float *__restrict__ Y3,
                                                                  float *__restrict__ PS3)
{
    __shared__ float Xs[AT_TM * AT_S2], Ws[AT_D3 * AT_S2], Ys[AT_TM * 33], as[AT_S2], ms[AT_S2], ss[AT_S2];
    const int c = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
    if (tid < AT_D2) {
        double mean = 0.0, var = 0.0;
        if (training) merge_stats(PS2 + (size_t)c * d.T * 2 * AT_D2, AT_D2, tid, d.T, d.TPB, d.P, d.R, mean, var);
        bn_channel(tab, c, 1, tid, training != 0, t == 0, mean, var, d.R, eps, momentum, AB, SV, as[tid], ms[tid], ss[tid]);
    }
    const float *W3 = tabf(tab, c, P_W3);
    for (int i = tid; i < AT_D3 * AT_S2; i += AT_THREADS) {
        const int r = i / AT_S2, k = i % AT_S2;
        Ws[i] = k < AT_D2 ? W3[r * AT_D2 + k] : 0.f;
    }
    __syncthreads();
    const float *Yin = Y2 + ((size_t)c * d.R + (size_t)b * d.P + p0) * AT_D2;
    for (int i = tid; i < AT_TM * AT_S2; i += AT_THREADS) {
        const int r = i / AT_S2, k = i % AT_S2;
        Xs[i] = (r < nv && k < AT_D2) ? bn_relu(as[k], ms[k], ss[k], Yin[r * AT_D2 + k]) : 0.f;
    }
    __syncthreads();
    const int wave = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    const int mb = wave >> 1, nb = wave & 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    {
        const float *A = Xs + (mb * 16 + li) * AT_S2 + lk, *Bm = Ws + (nb * 16 + li) * AT_S2 + lk;
        for (int ks = 0; ks < AT_S2 / 4; ++ks) acc = mfma4(A[ks * 4], Bm[ks * 4], acc);
    }
    const float bias = tabf(tab, c, P_B3)[nb * 16 + li];
#pragma unroll
    for (int r = 0; r < 4; ++r) Ys[(mb * 16 + lk * 4 + r) * 33 + nb * 16 + li] = acc[r] + bias;
    __syncthreads();
    float *Yg = Y3 + ((size_t)c * d.R + (size_t)b * d.P + p0) * AT_D3;
    for (int i = tid; i < nv * AT_D3; i += AT_THREADS) Yg[i] = Ys[(i / AT_D3) * 33 + i % AT_D3];
    if (training && tid < AT_D3) {
        float s = 0.f;
        for (int r = 0; r < nv; ++r) s += Ys[r * 33 + tid];
        const float m = s / nv;
        float q = 0.f;
        for (int r = 0; r < nv; ++r) { const float e = Ys[r * 33 + tid] - m; q += e * e; }
        float *ps = PS3 + ((size_t)c * d.T + t) * 2 * AT_D3;
        ps[tid] = s; ps[AT_D3 + tid] = q;
    }
}

// bn3 + relu on load, out[b][c P + p][:] = tanh(W4 x3 + b4)
__global__ __launch_bounds__(128) void atlas_l4_fwd_kernel(const void *const *tab, Dims d, int training, float eps, float momentum,
                                                           const float *__restrict__ Y3, const float *__restrict__ PS3,
                                                           float *__restrict__ AB, float *__restrict__ SV, float *__restrict__ out)
{
    __shared__ float Xs[AT_TM * 33], W4s[3 * AT_D3], as[AT_D3], ms[AT_D3], ss[AT_D3];
    const int c = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
    if (tid < AT_D3) {
        double mean = 0.0, var = 0.0;
        if (training) merge_stats(PS3 + (size_t)c * d.T * 2 * AT_D3, AT_D3, tid, d.T, d.TPB, d.P, d.R, mean, var);
        bn_channel(tab, c, 2, tid, training != 0, t == 0, mean, var, d.R, eps, momentum, AB, SV, as[tid], ms[tid], ss[tid]);
    }
    if (tid < 3 * AT_D3) W4s[tid] = tabf(tab, c, P_W4)[tid];
    __syncthreads();
    const float *Yin = Y3 + ((size_t)c * d.R + (size_t)b * d.P + p0) * AT_D3;
    for (int i = tid; i < nv * AT_D3; i += 128) Xs[(i / AT_D3) * 33 + i % AT_D3] = bn_relu(as[i % AT_D3], ms[i % AT_D3], ss[i % AT_D3], Yin[i]);
    __syncthreads();
    if (tid < 3 * AT_TM) {
        const int r = tid / 3, j = tid % 3;
        if (r < nv) {
            float acc = tabf(tab, c, P_B4)[j];
            for (int k = 0; k < AT_D3; ++k) acc = fmaf(Xs[r * 33 + k], W4s[j * AT_D3 + k], acc);
            out[(((size_t)b * d.C + c) * d.P + p0 + r) * 3 + j] = tanhf(acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ backward

// through tanh and conv4: G3 = (d4 W4) masked by x3 > 0, its BatchNorm sums per tile, dW4 / db4 per row group
__global__ __launch_bounds__(AT_THREADS) void atlas_l4_bwd_kernel(const void *const *tab, Dims d, const float *__restrict__ gout,
                                                                  const float *__restrict__ out, const float *__restrict__ Y3,
                                                                  const float *__restrict__ AB, const float *__restrict__ SV,
                                                                  float *__restrict__ G3, float *__restrict__ Q3,
                                                                  float *__restrict__ PW4)
{
    __shared__ float d4s[AT_TM * 3], Xs[AT_TM * 33], Hs[AT_TM * 33], Gs[AT_TM * 33], W4s[3 * AT_D3];
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float *ab = AB + ((size_t)c * 6 + 4) * AT_LD, *sv = SV + ((size_t)c * 6 + 4) * AT_LD;
    if (tid < 3 * AT_D3) W4s[tid] = tabf(tab, c, P_W4)[tid];
    float accw = 0.f;
    for (int t = g; t < d.T; t += d.NG) {
        const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
        __syncthreads();
        if (tid < 3 * AT_TM) {
            const int r = tid / 3;
            float v = 0.f;
            if (r < nv) {
                const size_t o = (((size_t)b * d.C + c) * d.P + p0) * 3 + tid;
                const float y = out[o];
                v = gout[o] * (1.f - y * y);
            }
            d4s[tid] = v;
        }
        const size_t row0 = (size_t)c * d.R + (size_t)b * d.P + p0;
        for (int i = tid; i < AT_TM * AT_D3; i += AT_THREADS) {
            const int r = i / AT_D3, k = i % AT_D3;
            float x = 0.f, h = 0.f;
            if (r < nv) {
                const float y = Y3[row0 * AT_D3 + i];
                x = bn_relu(ab[k], sv[k], ab[AT_LD + k], y);
                h = (y - sv[k]) * sv[AT_LD + k];
            }
            Xs[r * 33 + k] = x; Hs[r * 33 + k] = h;
        }
        __syncthreads();
        for (int i = tid; i < AT_TM * AT_D3; i += AT_THREADS) {
            const int r = i / AT_D3, k = i % AT_D3;
            float gx = d4s[r * 3] * W4s[k];
            gx = fmaf(d4s[r * 3 + 1], W4s[AT_D3 + k], gx);
            gx = fmaf(d4s[r * 3 + 2], W4s[2 * AT_D3 + k], gx);
            gx = Xs[r * 33 + k] > 0.f ? gx : 0.f;
            Gs[r * 33 + k] = gx;
            if (r < nv) G3[row0 * AT_D3 + i] = gx;
        }
        if (tid >= 128 && tid < 128 + 3 * AT_D3) {
            const int j = (tid - 128) / AT_D3, k = (tid - 128) % AT_D3;
            for (int r = 0; r < nv; ++r) accw = fmaf(d4s[r * 3 + j], Xs[r * 33 + k], accw);
        } else if (tid >= 128 + 3 * AT_D3 && tid < 128 + 3 * AT_D3 + 3) {
            for (int r = 0; r < nv; ++r) accw += d4s[r * 3 + tid - 128 - 3 * AT_D3];
        }
        __syncthreads();
        if (tid < AT_D3) {
            float s0 = 0.f, s1 = 0.f;
            for (int r = 0; r < nv; ++r) { s0 += Gs[r * 33 + tid]; s1 = fmaf(Gs[r * 33 + tid], Hs[r * 33 + tid], s1); }
            float *q = Q3 + ((size_t)c * d.T + t) * 2 * AT_D3;
            q[tid] = s0; q[AT_D3 + tid] = s1;
        }
    }
    if (tid >= 128 && tid < 128 + PW4_N) PW4[((size_t)c * d.NG + g) * PW4_N + tid - 128] = accw;
}

// the two sums of a BatchNorm backward over all tiles of a chart, in tile order
__device__ void merge_bwd(const float *q, int width, int ch, int T, double &s0, double &s1)
{
    s0 = 0.0; s1 = 0.0;
    for (int t = 0; t < T; ++t) {
        s0 += (double)q[((size_t)t * 2) * width + ch];
        s1 += (double)q[((size_t)t * 2 + 1) * width + ch];
    }
}

// through bn3 and conv3: dY3 from G3, dW3 / db3 per row group, G2 = (dY3 W3) masked by x2 > 0 and its sums per tile
__global__ __launch_bounds__(AT_THREADS) void atlas_l3_bwd_kernel(const void *const *tab, Dims d, int training,
                                                                  const float *__restrict__ Y2, const float *__restrict__ Y3,
                                                                  const float *__restrict__ AB, const float *__restrict__ SV,
                                                                  const float *__restrict__ G3, const float *__restrict__ Q3,
                                                                  float *__restrict__ G2, float *__restrict__ Q2,
                                                                  float *__restrict__ PW3, float *__restrict__ gparams)
{
    __shared__ float dYs[AT_TM * 36], Xs[AT_TM * AT_S2], Ws[AT_D3 * AT_S2], Gs[AT_TM * AT_S2];
    __shared__ float m1s[AT_D3], m2s[AT_D3];
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float *ab3 = AB + ((size_t)c * 6 + 4) * AT_LD, *sv3 = SV + ((size_t)c * 6 + 4) * AT_LD;
    const float *ab2 = AB + ((size_t)c * 6 + 2) * AT_LD, *sv2 = SV + ((size_t)c * 6 + 2) * AT_LD;
    if (tid < AT_D3) {
        double s0, s1;
        merge_bwd(Q3 + (size_t)c * d.T * 2 * AT_D3, AT_D3, tid, d.T, s0, s1);
        m1s[tid] = (float)(s0 / d.R); m2s[tid] = (float)(s1 / d.R);
        if (g == 0) {
            gparams[(size_t)c * AT_NPARAM + G_G3 + tid] = (float)s1;
            gparams[(size_t)c * AT_NPARAM + G_BE3 + tid] = (float)s0;
        }
    }
    const float *W3 = tabf(tab, c, P_W3);
    for (int i = tid; i < AT_D3 * AT_S2; i += AT_THREADS) {
        const int r = i / AT_S2, k = i % AT_S2;
        Ws[i] = k < AT_D2 ? W3[r * AT_D2 + k] : 0.f;
    }
    const int wave = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    f32x4 accw[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) accw[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float accb = 0.f;
    for (int t = g; t < d.T; t += d.NG) {
        const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
        const size_t row0 = (size_t)c * d.R + (size_t)b * d.P + p0;
        __syncthreads();
        for (int i = tid; i < AT_TM * AT_D3; i += AT_THREADS) {
            const int r = i / AT_D3, n = i % AT_D3;
            float v = 0.f;
            if (r < nv) {
                const float gg = G3[row0 * AT_D3 + i];
                if (training) {
                    const float h = (Y3[row0 * AT_D3 + i] - sv3[n]) * sv3[AT_LD + n];
                    v = ab3[n] * ((gg - m1s[n]) - h * m2s[n]);
                } else {
                    v = ab3[n] * gg;
                }
            }
            dYs[r * 36 + n] = v;
        }
        for (int i = tid; i < AT_TM * AT_S2; i += AT_THREADS) {
            const int r = i / AT_S2, k = i % AT_S2;
            Xs[i] = (r < nv && k < AT_D2) ? bn_relu(ab2[k], sv2[k], ab2[AT_LD + k], Y2[(row0 + r) * AT_D2 + k]) : 0.f;
        }
        __syncthreads();
        // dW3 [32 x 65] += dY3^T [32 x rows] . x2 [rows x 65]
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int blk = wave + 4 * q;
            if (blk < 10) {
                const int mb = blk / 5, nb = blk % 5;
                const float *A = dYs + lk * 36 + mb * 16 + li, *Bm = Xs + lk * AT_S2 + min(nb * 16 + li, AT_S2 - 1);
                for (int ks = 0; ks < AT_TM / 4; ++ks) accw[q] = mfma4(A[ks * 4 * 36], Bm[ks * 4 * AT_S2], accw[q]);
            }
        }
        if (tid >= 128 && tid < 128 + AT_D3)
            for (int r = 0; r < nv; ++r) accb += dYs[r * 36 + tid - 128];
        // dX2 [rows x 65] = dY3 [rows x 32] . W3 [32 x 65]
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int blk = wave + 4 * q;
            if (blk < 10) {
                const int mb = blk / 5, nb = blk % 5, col = nb * 16 + li;
                const float *A = dYs + (mb * 16 + li) * 36 + lk, *Bm = Ws + lk * AT_S2 + min(col, AT_S2 - 1);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int ks = 0; ks < AT_D3 / 4; ++ks) acc = mfma4(A[ks * 4], Bm[ks * 4 * AT_S2], acc);
                if (col < AT_D2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = mb * 16 + lk * 4 + r;
                        Gs[row * AT_S2 + col] = Xs[row * AT_S2 + col] > 0.f ? acc[r] : 0.f;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nv * AT_D2; i += AT_THREADS) G2[row0 * AT_D2 + i] = Gs[(i / AT_D2) * AT_S2 + i % AT_D2];
        if (tid < AT_D2) {
            float s0 = 0.f, s1 = 0.f;
            const float mu = sv2[tid], inv = sv2[AT_LD + tid];
            for (int r = 0; r < nv; ++r) {
                const float gg = Gs[r * AT_S2 + tid];
                s0 += gg;
                s1 = fmaf(gg, (Y2[(row0 + r) * AT_D2 + tid] - mu) * inv, s1);
            }
            float *q = Q2 + ((size_t)c * d.T + t) * 2 * AT_D2;
            q[tid] = s0; q[AT_D2 + tid] = s1;
        }
    }
    float *pw = PW3 + ((size_t)c * d.NG + g) * PW3_N;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int blk = wave + 4 * q;
        if (blk < 10) {
            const int mb = blk / 5, nb = blk % 5, col = nb * 16 + li;
            if (col < AT_D2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) pw[(mb * 16 + lk * 4 + r) * AT_D2 + col] = accw[q][r];
            }
        }
    }
    if (tid >= 128 && tid < 128 + AT_D3) pw[AT_D3 * AT_D2 + tid - 128] = accb;
}

// through bn2 and conv2: dY2 from G2, dW2 / db2 per row group, and of G1 = (dY2 W2) masked by x1 > 0 only the four sums per
// tile that the first layer's backward needs (G1 itself is never stored)
__global__ __launch_bounds__(AT_THREADS) void atlas_l2_bwd_kernel(const void *const *tab, const float *__restrict__ grid, Dims d,
                                                                  int training, const float *__restrict__ H,
                                                                  const float *__restrict__ Y2, const float *__restrict__ AB,
                                                                  const float *__restrict__ SV, const float *__restrict__ G2,
                                                                  const float *__restrict__ Q2, float *__restrict__ Q1,
                                                                  float *__restrict__ PW2, float *__restrict__ gparams)
{
    // 65 400 of the 65 536 bytes of static LDS a workgroup may declare: another shared array here does not build; it has
    // to come out of the tiles (a smaller AT_TM) first
    __shared__ float Ws[AT_S2 * AT_S1];          // W2 [65 x 130], rows 65 .. 67 and columns 130, 131 zero
    __shared__ float Xs[AT_TM * AT_S1];          // x1
    __shared__ float dYs[AT_TM * AT_S2];         // dY2, columns 65 .. 67 zero
    __shared__ float w0s[AT_D1], w1s[AT_D1], as[AT_D1], ss[AT_D1], ms[AT_D1], hs[AT_D1];
    __shared__ float m1s[AT_D2], m2s[AT_D2], us[AT_TM], vs[AT_TM];
    const int c = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    const float *ab2 = AB + ((size_t)c * 6 + 2) * AT_LD, *sv2 = SV + ((size_t)c * 6 + 2) * AT_LD;
    const float *sv1 = SV + (size_t)c * 6 * AT_LD;
    const float *W1 = tabf(tab, c, P_W1), *W2 = tabf(tab, c, P_W2);
    if (tid < AT_D2) {
        double s0, s1;
        merge_bwd(Q2 + (size_t)c * d.T * 2 * AT_D2, AT_D2, tid, d.T, s0, s1);
        m1s[tid] = (float)(s0 / d.R); m2s[tid] = (float)(s1 / d.R);
        if (g == 0) {
            gparams[(size_t)c * AT_NPARAM + G_G2 + tid] = (float)s1;
            gparams[(size_t)c * AT_NPARAM + G_BE2 + tid] = (float)s0;
        }
    }
    if (tid < AT_D1) {
        w0s[tid] = W1[tid * AT_D1]; w1s[tid] = W1[tid * AT_D1 + 1];
        as[tid] = AB[(size_t)c * 6 * AT_LD + tid]; ss[tid] = AB[((size_t)c * 6 + 1) * AT_LD + tid];
        ms[tid] = sv1[tid];
    }
    for (int i = tid; i < AT_S2 * AT_S1; i += AT_THREADS) {
        const int r = i / AT_S1, k = i % AT_S1;
        Ws[i] = (r < AT_D2 && k < AT_D1) ? W2[r * AT_D1 + k] : 0.f;
    }
    const int wave = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    f32x4 accw[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) accw[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float accb = 0.f;
    for (int t = g; t < d.T; t += d.NG) {
        const int b = t / d.TPB, p0 = (t % d.TPB) * AT_TM, nv = min(AT_TM, d.P - p0);
        const size_t row0 = (size_t)c * d.R + (size_t)b * d.P + p0;
        __syncthreads();
        if (tid < AT_D1) hs[tid] = H[((size_t)c * d.B + b) * AT_D1 + tid];
        if (tid >= 192 && tid < 192 + AT_TM) {
            const int r = tid - 192;
            us[r] = r < nv ? grid[p0 + r] : 0.f;
            vs[r] = r < nv ? grid[d.P + p0 + r] : 0.f;
        }
        for (int i = tid; i < AT_TM * AT_S2; i += AT_THREADS) {
            const int r = i / AT_S2, n = i % AT_S2;
            float v = 0.f;
            if (r < nv && n < AT_D2) {
                const float gg = G2[(row0 + r) * AT_D2 + n];
                if (training) {
                    const float h = (Y2[(row0 + r) * AT_D2 + n] - sv2[n]) * sv2[AT_LD + n];
                    v = ab2[n] * ((gg - m1s[n]) - h * m2s[n]);
                } else {
                    v = ab2[n] * gg;
                }
            }
            dYs[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < AT_TM * AT_S1; i += AT_THREADS) {
            const int r = i / AT_S1, k = i % AT_S1;
            float x = 0.f;
            if (r < nv && k < AT_D1) x = bn_relu(as[k], ms[k], ss[k], x1_pre(w0s[k], w1s[k], us[r], vs[r], hs[k]));
            Xs[i] = x;
        }
        __syncthreads();
        // dW2 [65 x 130] += dY2^T [65 x rows] . x1 [rows x 130]: 5 x 9 blocks of 16 x 16, clamped lanes land on zero columns
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const int blk = wave + 4 * q;
            if (blk < 45) {
                const int mb = blk / 9, nb = blk % 9;
                const float *A = dYs + lk * AT_S2 + min(mb * 16 + li, AT_S2 - 1), *Bm = Xs + lk * AT_S1 + min(nb * 16 + li, AT_S1 - 1);
                for (int ks = 0; ks < AT_TM / 4; ++ks) accw[q] = mfma4(A[ks * 4 * AT_S2], Bm[ks * 4 * AT_S1], accw[q]);
            }
        }
        if (tid >= 128 && tid < 128 + AT_D2)
            for (int r = 0; r < nv; ++r) accb += dYs[r * AT_S2 + tid - 128];
        // dX1 [rows x 130] = dY2 [rows x 65] . W2 [65 x 130]; a wave owns whole columns, so the sums over the tile's rows stay
        // inside it: registers, then the lanes 16 and 32 apart
        for (int nb = wave; nb < 9; nb += 4) {
            const int col = nb * 16 + li, colc = min(col, AT_S1 - 1);
            float s0 = 0.f, su = 0.f, sv = 0.f, sx = 0.f;
            const float mu = col < AT_D1 ? ms[col] : 0.f, inv = col < AT_D1 ? sv1[AT_LD + col] : 0.f;
            const float w0 = col < AT_D1 ? w0s[col] : 0.f, w1 = col < AT_D1 ? w1s[col] : 0.f, hh = col < AT_D1 ? hs[col] : 0.f;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const float *A = dYs + (mb * 16 + li) * AT_S2 + lk, *Bm = Ws + lk * AT_S1 + colc;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int ks = 0; ks < AT_S2 / 4; ++ks) acc = mfma4(A[ks * 4], Bm[ks * 4 * AT_S1], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mb * 16 + lk * 4 + r;
                    const float gg = Xs[row * AT_S1 + colc] > 0.f ? acc[r] : 0.f;
                    const float u = us[row], v = vs[row];
                    s0 += gg;
                    su = fmaf(gg, u, su);
                    sv = fmaf(gg, v, sv);
                    sx = fmaf(gg, (x1_pre(w0, w1, u, v, hh) - mu) * inv, sx);
                }
            }
            s0 += __shfl_xor(s0, 16, 64); su += __shfl_xor(su, 16, 64); sv += __shfl_xor(sv, 16, 64); sx += __shfl_xor(sx, 16, 64);
            s0 += __shfl_xor(s0, 32, 64); su += __shfl_xor(su, 32, 64); sv += __shfl_xor(sv, 32, 64); sx += __shfl_xor(sx, 32, 64);
            if (lk == 0 && col < AT_D1) {
                float *q = Q1 + ((size_t)c * d.T + t) * 4 * AT_D1;
                q[col] = s0; q[AT_D1 + col] = su; q[2 * AT_D1 + col] = sv; q[3 * AT_D1 + col] = sx;
            }
        }
    }
    float *pw = PW2 + ((size_t)c * d.NG + g) * PW2_N;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int blk = wave + 4 * q;
        if (blk < 45) {
            const int mb = blk / 9, nb = blk % 9, col = nb * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = mb * 16 + lk * 4 + r;
                if (n < AT_D2 && col < AT_D1) pw[n * AT_D1 + col] = accw[q][r];
            }
        }
    }
    if (tid >= 128 && tid < 128 + AT_D2) pw[AT_D2 * AT_D1 + tid - 128] = accb;
}

// through bn1: per channel the gradient of the latent part dH [B], of the two grid columns of W1, of b1, gamma1 and beta1
__global__ __launch_bounds__(192) void atlas_l1_bwd_kernel(const void *const *tab, const float *__restrict__ grid, Dims d,
                                                            int training, const float *__restrict__ H,
                                                            const float *__restrict__ AB, const float *__restrict__ SV,
                                                            const float *__restrict__ Q1, float *__restrict__ DH,
                                                            float *__restrict__ gparams)
{
    const int c = blockIdx.x, ch = threadIdx.x;
    if (ch >= AT_D1) return;
    const float *q = Q1 + (size_t)c * d.T * 4 * AT_D1;
    double S0 = 0.0, Su = 0.0, Sv = 0.0, Sx = 0.0;
    for (int t = 0; t < d.T; ++t) {
        S0 += (double)q[((size_t)t * 4) * AT_D1 + ch];
        Su += (double)q[((size_t)t * 4 + 1) * AT_D1 + ch];
        Sv += (double)q[((size_t)t * 4 + 2) * AT_D1 + ch];
        Sx += (double)q[((size_t)t * 4 + 3) * AT_D1 + ch];
    }
    const double a = AB[(size_t)c * 6 * AT_LD + ch];
    const double inv = SV[((size_t)c * 6 + 1) * AT_LD + ch];
    float *gp = gparams + (size_t)c * AT_NPARAM;
    gp[G_G1 + ch] = (float)Sx;
    gp[G_BE1 + ch] = (float)S0;
    const float *W = tabf(tab, c, P_W1) + ch * AT_D1;
    const double w0 = W[0], w1 = W[1];
    double sg = 0.0, sgu = 0.0, sgv = 0.0, sumu = 0.0, sumv = 0.0, sumh = 0.0;
    if (training) {
        for (int p = 0; p < d.P; ++p) {
            const double u = grid[p], v = grid[d.P + p], gg = (double)((float)w0 * grid[p] + (float)w1 * grid[d.P + p]);
            sg += gg; sgu += gg * u; sgv += gg * v; sumu += u; sumv += v;
        }
        for (int b = 0; b < d.B; ++b) sumh += (double)H[((size_t)c * d.B + b) * AT_D1 + ch];
    }
    // the batch mean before its rounding to fp32: the sums of x1hat over p and over (b, p) below are differences of y1 and
    // this mean that cancel (to zero for B = 1), which the rounded mean would turn into noise of P ulps
    const double mu = sg / d.P + sumh / d.B;
    const double m1 = S0 / d.R, m2 = Sx / d.R;
    double db = 0.0;
    for (int b = 0; b < d.B; ++b) {
        double s0b = 0.0;
        for (int tt = 0; tt < d.TPB; ++tt) s0b += (double)q[((size_t)(b * d.TPB + tt) * 4) * AT_D1 + ch];
        double dh;
        if (training) {
            const double hb = H[((size_t)c * d.B + b) * AT_D1 + ch];
            dh = a * (s0b - d.P * m1 - m2 * inv * (sg + d.P * (hb - mu)));
        } else {
            dh = a * s0b;
        }
        db += dh;
        DH[((size_t)c * d.B + b) * AT_D1 + ch] = (float)dh;
    }
    double dw0, dw1;
    if (training) {
        const double rest = sumh - d.B * mu;   // sum over b of (H_b - mean)
        dw0 = a * (Su - m1 * d.B * sumu - m2 * inv * (d.B * sgu + rest * sumu));
        dw1 = a * (Sv - m1 * d.B * sumv - m2 * inv * (d.B * sgv + rest * sumv));
        db = 0.0;                              // a bias in front of a batch-statistics BatchNorm has zero gradient
    } else {
        dw0 = a * Su;
        dw1 = a * Sv;
    }
    gp[G_W1 + ch * AT_D1] = (float)dw0;
    gp[G_W1 + ch * AT_D1 + 1] = (float)dw1;
    gp[G_B1 + ch] = (float)db;
}

// y < C: the latent columns of dW1 and the sums of the row-group partials of chart y; y == C: dz over all charts
__global__ __launch_bounds__(AT_THREADS) void atlas_finish_kernel(const void *const *tab, const float *__restrict__ z, Dims d,
                                                                  int training, const float *__restrict__ DH,
                                                                  const float *__restrict__ PW2, const float *__restrict__ PW3,
                                                                  const float *__restrict__ PW4, float *__restrict__ gz,
                                                                  float *__restrict__ gparams)
{
    const int c = blockIdx.y;
    const int step = gridDim.x * AT_THREADS;
    if (c == d.C) {
        for (int i = blockIdx.x * AT_THREADS + threadIdx.x; i < d.B * AT_Z; i += step) {
            const int b = i / AT_Z, k = i % AT_Z;
            float acc = 0.f;
            for (int cc = 0; cc < d.C; ++cc) {
                const float *W = tabf(tab, cc, P_W1) + 2 + k, *dh = DH + ((size_t)cc * d.B + b) * AT_D1;
                for (int ch = 0; ch < AT_D1; ++ch) acc = fmaf(dh[ch], W[ch * AT_D1], acc);
            }
            gz[i] = acc;
        }
        return;
    }
    float *gp = gparams + (size_t)c * AT_NPARAM;
    constexpr int N1 = AT_D1 * AT_Z;
    for (int i = blockIdx.x * AT_THREADS + threadIdx.x; i < N1 + PW2_N + PW3_N + PW4_N; i += step) {
        if (i < N1) {
            const int ch = i / AT_Z, k = i % AT_Z;
            float acc = 0.f;
            for (int b = 0; b < d.B; ++b) acc = fmaf(DH[((size_t)c * d.B + b) * AT_D1 + ch], z[(size_t)b * AT_Z + k], acc);
            gp[G_W1 + ch * AT_D1 + 2 + k] = acc;
            continue;
        }
        int j = i - N1, n, dst;
        const float *src;
        bool bias;
        if (j < PW2_N) { src = PW2 + (size_t)c * d.NG * PW2_N; n = PW2_N; dst = G_W2; bias = j >= AT_D2 * AT_D1; }
        else if ((j -= PW2_N) < PW3_N) { src = PW3 + (size_t)c * d.NG * PW3_N; n = PW3_N; dst = G_W3; bias = j >= AT_D3 * AT_D2; }
        else { j -= PW3_N; src = PW4 + (size_t)c * d.NG * PW4_N; n = PW4_N; dst = G_W4; bias = false; }
        float acc = 0.f;
        for (int gI = 0; gI < d.NG; ++gI) acc += src[(size_t)gI * n + j];
        // a bias in front of a batch-statistics BatchNorm has zero gradient
        gp[dst + j] = (bias && training) ? 0.f : acc;
    }
}

bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

long long prifit_atlas_workspace_floats(int num_charts, int B, int P, int backward)
{
    if (!dims_ok(num_charts, B, P)) return 0;
    const Dims d = make_dims(num_charts, B, P);
    return (long long)(backward ? bwd_ws(d).total : fwd_ws(d).total);
}

int prifit_atlas_fwd(const void *const *params, const float *z, const float *grid, int num_charts, int B, int P, int training,
                     float eps, float momentum, float *out, float *workspace, void *stream)
{
    if (!params || !z || !grid || !out || !workspace || !dims_ok(num_charts, B, P) || !aligned(params, 8) ||
        !aligned(workspace, 4) || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f))
        return PRIFIT_EINVAL;
    if (training && (long long)B * P < 2) return PRIFIT_EINVAL;   // no variance from one value per channel
    const Dims d = make_dims(num_charts, B, P);
    const FwdWs w = fwd_ws(d);
    float *ws = workspace;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(atlas_latent_kernel, dim3((B + AT_BT - 1) / AT_BT, d.C), dim3(AT_THREADS), 0, st, params, z, B, ws + w.H);
    hipLaunchKernelGGL(atlas_bn1_kernel, dim3(d.C), dim3(192), 0, st, params, grid, d, training, eps, momentum, ws + w.H,
                       ws + w.AB, ws + w.SV);
    hipLaunchKernelGGL(atlas_l2_fwd_kernel, dim3(d.T, d.C), dim3(AT_THREADS), 0, st, params, grid, d, training, ws + w.H,
                       ws + w.AB, ws + w.SV, ws + w.Y2, ws + w.PS2);
    hipLaunchKernelGGL(atlas_l3_fwd_kernel, dim3(d.T, d.C), dim3(AT_THREADS), 0, st, params, d, training, eps, momentum,
                       ws + w.Y2, ws + w.PS2, ws + w.AB, ws + w.SV, ws + w.Y3, ws + w.PS3);
    hipLaunchKernelGGL(atlas_l4_fwd_kernel, dim3(d.T, d.C), dim3(128), 0, st, params, d, training, eps, momentum, ws + w.Y3,
                       ws + w.PS3, ws + w.AB, ws + w.SV, out);
    return prifit_check_launch();
}

int prifit_atlas_bwd(const void *const *params, const float *z, const float *grid, int num_charts, int B, int P, int training,
                     const float *gout, const float *out, const float *fwd_workspace, float *workspace, float *gz,
                     float *gparams, void *stream)
{
    if (!params || !z || !grid || !gout || !out || !fwd_workspace || !workspace || !gz || !gparams ||
        !dims_ok(num_charts, B, P) || !aligned(params, 8))
        return PRIFIT_EINVAL;
    if (training && (long long)B * P < 2) return PRIFIT_EINVAL;
    const Dims d = make_dims(num_charts, B, P);
    const FwdWs f = fwd_ws(d);
    const BwdWs w = bwd_ws(d);
    const float *fw = fwd_workspace;
    float *ws = workspace;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(atlas_l4_bwd_kernel, dim3(d.NG, d.C), dim3(AT_THREADS), 0, st, params, d, gout, out, fw + f.Y3, fw + f.AB,
                       fw + f.SV, ws + w.G3, ws + w.Q3, ws + w.PW4);
    hipLaunchKernelGGL(atlas_l3_bwd_kernel, dim3(d.NG, d.C), dim3(AT_THREADS), 0, st, params, d, training, fw + f.Y2, fw + f.Y3,
                       fw + f.AB, fw + f.SV, ws + w.G3, ws + w.Q3, ws + w.G2, ws + w.Q2, ws + w.PW3, gparams);
    hipLaunchKernelGGL(atlas_l2_bwd_kernel, dim3(d.NG, d.C), dim3(AT_THREADS), 0, st, params, grid, d, training, fw + f.H,
                       fw + f.Y2, fw + f.AB, fw + f.SV, ws + w.G2, ws + w.Q2, ws + w.Q1, ws + w.PW2, gparams);
    hipLaunchKernelGGL(atlas_l1_bwd_kernel, dim3(d.C), dim3(192), 0, st, params, grid, d, training, fw + f.H, fw + f.AB,
                       fw + f.SV, ws + w.Q1, ws + w.DH, gparams);
    hipLaunchKernelGGL(atlas_finish_kernel, dim3(24, d.C + 1), dim3(AT_THREADS), 0, st, params, z, d, training, ws + w.DH,
                       ws + w.PW2, ws + w.PW3, ws + w.PW4, gz, gparams);
    return prifit_check_launch();
}

}  // extern "C"
