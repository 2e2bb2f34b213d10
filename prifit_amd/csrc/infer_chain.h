// The on-chip MLP chains of frozen inference, written once for every matrix pipe.  A chain computes the
// TRANSPOSED products H^T = W1' X^T, Y^T = W2' H^T, ... on a 32x32 MFMA: the weights are the A operand, 32 activation rows
// the B operand.  The C/D layout of the 32x32 MFMAs does not depend on the input type -- block b, register 4g + m of lane
// (j, h) = channel 32b + 8g + 4h + m of activation row j -- so a finished block IS the B operand of the next product, and a
// wave carries its 32 rows through all layers in registers: no LDS tile, no barrier, no shuffle between the layers.
//
// What depends on the input type is a small policy struct, `Pipe` (PipeF32 in infer.hip, PipeBf16 in infer_bf16.hip):
//   W, Frag, KSTEP   the weight element, a lane's operand fragment, the input columns per k-step of a wave.  A lane half
//                    reads KSTEP / 2 consecutive elements at column KSTEP t + (KSTEP / 2) h: one 16-byte load
//   PADDED           weight rows are zero from their input width to a whole k-step (else the skeleton masks a tail fragment)
//   zero()           an all-zero fragment
//   load_w(p, t)     the weight fragment of k-step t; p = the lane's row, advanced to its half
//   from_mem<RELU, K>(xr, t, h)   the B fragment of k-step t of a K-column row in memory; xr advanced to the lane's half
//   from_acc(acc, s) the B fragment s (0 .. 32 / KSTEP - 1) of a finished 32-channel block
//   mma(a, b, acc)   the MFMA(s) of one k-step
//   block_end()      a scheduling hook behind a finished block's fragments (bf16: a fence, see PipeBf16)
//   pitch_ok(ld, kin)   (host) the pitch rule of a weight row
// Everything else is here: the product of one output block, bias + ReLU, the three kernels (pooled chain, row chain, embedding
// chain), what follows the last product (the max over a wave's rows and the pooling groups of a workgroup; the scores' stores
// and the category-restricted arg-max; the embedding's stores and its normalisation), the argument checks and the launch
// ladders.  Each of the two translation units instantiates the kernels for its own pipe.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int CHAIN_ROWS = 128;   // rows per workgroup: 4 waves x 32
constexpr f32x16 ZERO16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

// the ReLU between layers.  KEEP_NAN (np.maximum, torch.relu): a NaN input row reaches the scores, where the arg-max rule
// ranks it; else fmaxf, which drops it -- the pooled chain's, whose max over rows drops a NaN anyway
template <bool KEEP_NAN>
__device__ __forceinline__ float chain_relu(float v) { return KEEP_NAN ? (v < 0.f ? 0.f : v) : fmaxf(v, 0.f); }

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

inline bool mis16(const void *p) { return ((uintptr_t)p & 15) != 0; }

// ---- the pieces of a layer
template <typename Pipe>
constexpr int chain_ksteps(int K) { return (K + Pipe::KSTEP - 1) / Pipe::KSTEP; }

// output block b of one transposed product: rows 32b + 0..31 of Wm [., ldw] times the K input channels held in `in`.
// MASKED: rows >= C are zero A rows (the row index clamped for the load, the value zeroed).
template <typename Pipe, int K, bool MASKED>
__device__ __forceinline__ f32x16 chain_block(const typename Pipe::W *Wm, long long ldw, int b, int C,
                                              const typename Pipe::Frag (&in)[chain_ksteps<Pipe>(K)], int li, int lh)
{
    constexpr int KSTEP = Pipe::KSTEP, H = KSTEP / 2;
    static_assert(Pipe::PADDED || K % KSTEP == 0 || K % KSTEP == H, "a lane half is in or out of the row as a whole");
    f32x16 acc = ZERO16;
    const int c = 32 * b + li;
    const bool ok = !MASKED || c < C;
    const typename Pipe::W *wr = Wm + (long long)(ok ? c : 0) * ldw + H * lh;
#pragma unroll
    for (int t = 0; t < chain_ksteps<Pipe>(K); ++t) {
        typename Pipe::Frag a;
        if (Pipe::PADDED || KSTEP * t + KSTEP <= K) a = Pipe::load_w(wr, t);      // (compile time) both halves inside the row
        else {                                                                    // the upper half is past the row's end
            a = Pipe::load_w(wr - H * lh, lh ? 0 : t);      // any address inside the row
            if (lh) a = Pipe::zero();
        }
        if (!ok) a = Pipe::zero();
        acc = Pipe::mma(a, in[t], acc);
    }
    return acc;
}

// bias + ReLU of the finished block b of a C-channel layer (C % 4 == 0: a lane's four channels are in or out together;
// channels >= C get a zero bias and stay exactly 0), handed on as the B fragments of the next product
template <typename Pipe, bool KEEP_NAN, int C>
__device__ __forceinline__ void chain_close(f32x16 acc, const float *bias, int b, int lh, typename Pipe::Frag (&out)[chain_ksteps<Pipe>(C)])
{
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int c0 = 32 * b + 8 * gq + 4 * lh;
        const float4 bb = (32 * b + 8 * gq + 8 <= C || c0 < C) ? ld4(bias + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[4 * gq + 0] = chain_relu<KEEP_NAN>(acc[4 * gq + 0] + bb.x);
        acc[4 * gq + 1] = chain_relu<KEEP_NAN>(acc[4 * gq + 1] + bb.y);
        acc[4 * gq + 2] = chain_relu<KEEP_NAN>(acc[4 * gq + 2] + bb.z);
        acc[4 * gq + 3] = chain_relu<KEEP_NAN>(acc[4 * gq + 3] + bb.w);
    }
    constexpr int FPB = 32 / Pipe::KSTEP;
#pragma unroll
    for (int s = 0; s < FPB; ++s)
        if (FPB * b + s < chain_ksteps<Pipe>(C)) out[FPB * b + s] = Pipe::from_acc(acc, s);      // (compile time)
    Pipe::block_end();
}

// ---- the pooled chain: layers 2 and 3 of a set-abstraction scale and its pool
template <typename WT>
struct ChainArgsT {
    const float *X;
    long long ldx;
    long long P;             // G * pool_K rows
    int G, pool_K;
    const WT *W1;
    const float *b1;
    const WT *W2;
    const float *b2;
    long long ldw1, ldw2;
    float *out;
    long long ldo;
};

// output block b2 of the last layer (fp32 accumulators of a wave's 32 rows) -> s_pool[C2] of this wave.  Max over rows first,
// bias and ReLU on the maximum: x -> relu(x + b) is non-decreasing in fp32, so the two commute exactly.
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

// X [P, C0] (pre-activation of layer 1, ReLU on load) -> out[g, :] = max over the pool_K rows of group g of
// relu(W2 relu(W1 relu(x) + b1) + b2); W1 [C1, ldw1], W2 [C2, ldw2] in the pipe's weight layout.  C0 a multiple of the
// k-step, C1 % 4 == 0, C2 % 32 == 0, pool_K in {32, 64, 128}: a wave's 32 rows lie in one group and a workgroup's 128 rows
// hold whole groups.  Channels >= C1 of the intermediate are exactly 0 (zero A rows, zero bias) and meet zero columns of W2:
// the pack kernel's padding, or the masked tail fragment of an unpadded pipe (fp32 at C1 = 196), decided at compile time.
template <typename Pipe, int C0, int C1, int C2>
__global__ __launch_bounds__(256) void mlp_chain_pool_kernel(const ChainArgsT<typename Pipe::W> g)
{
    static_assert(C0 % Pipe::KSTEP == 0 && C1 % 4 == 0 && C2 % 32 == 0, "fragment shapes");
    constexpr int H = Pipe::KSTEP / 2, NB1 = (C1 + 31) / 32, NB2 = C2 / 32;
    __shared__ __attribute__((aligned(16))) float s_pool[4][C2];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * CHAIN_ROWS + 32 * wave;

    if (row0 < g.P) {    // wave-uniform; P % 32 == 0: a live wave has 32 rows
        // B operand of layer 1: lane (j, h) holds relu(X[row0 + j][KSTEP t + H h + 0 .. H - 1]) in k-step t
        typename Pipe::Frag xf[chain_ksteps<Pipe>(C0)];
        const float *xr = g.X + (row0 + li) * g.ldx + H * lh;
#pragma unroll
        for (int t = 0; t < chain_ksteps<Pipe>(C0); ++t) xf[t] = Pipe::template from_mem<true, C0>(xr, t, lh);
        // layer 1, handed on as the B fragments of layer 2 as each block ends
        typename Pipe::Frag hf[chain_ksteps<Pipe>(C1)];
#pragma unroll
        for (int b = 0; b < NB1; ++b)
            chain_close<Pipe, false, C1>(chain_block<Pipe, C0, true>(g.W1, g.ldw1, b, C1, xf, li, lh), g.b1, b, lh, hf);
        // layer 2 + the max over this wave's 32 rows, 32 output channels at a time
#pragma unroll 1
        for (int b2 = 0; b2 < NB2; ++b2)
            chain_pool_block(chain_block<Pipe, C1, false>(g.W2, g.ldw2, b2, C2, hf, li, lh), g.b2, b2, li, lh, s_pool[wave]);
    }
    __syncthreads();
    chain_pool_groups<C2>(s_pool, g.G, g.pool_K, g.out, g.ldo);
}

inline int chain_shape(int C0, int C1, int C2)
{
    static const int shapes[5][3] = {{32, 32, 64}, {64, 64, 128}, {64, 96, 128}, {128, 128, 256}, {128, 196, 256}};
    for (int i = 0; i < 5; ++i)
        if (shapes[i][0] == C0 && shapes[i][1] == C1 && shapes[i][2] == C2) return i;
    return -1;
}

inline int chain_pool_supported(int C0, int C1, int C2, int pool_K)
{
    return (chain_shape(C0, C1, C2) >= 0 && (pool_K == 32 || pool_K == 64 || pool_K == 128)) ? 1 : 0;
}

template <typename Pipe, int C0, int C1, int C2>
void chain_pool_launch(const ChainArgsT<typename Pipe::W> &g, hipStream_t st)
{
    const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
    hipLaunchKernelGGL((mlp_chain_pool_kernel<Pipe, C0, C1, C2>), dim3(grid), dim3(256), 0, st, g);
}

template <typename Pipe>
int chain_pool_run(const float *X, long long ldx, int G, int pool_K, int C0, int C1, int C2, const typename Pipe::W *W1,
                   long long ldw1, const float *b1, const typename Pipe::W *W2, long long ldw2, const float *b2, float *out,
                   long long ldo, void *stream)
{
    if (!chain_pool_supported(C0, C1, C2, pool_K) || !X || !W1 || !b1 || !W2 || !b2 || !out || G <= 0 || ldx < C0 || (ldx & 3) ||
        !Pipe::pitch_ok(ldw1, C0) || !Pipe::pitch_ok(ldw2, C1) || ldo < C2 || mis16(X) || mis16(W1) || mis16(b1) || mis16(W2) ||
        mis16(b2) || (long long)G * pool_K > 0x7fffffffLL)
        return PRIFIT_EINVAL;
    ChainArgsT<typename Pipe::W> g = {};
    g.X = X; g.ldx = ldx; g.P = (long long)G * pool_K; g.G = G; g.pool_K = pool_K;
    g.W1 = W1; g.b1 = b1; g.W2 = W2; g.b2 = b2; g.ldw1 = ldw1; g.ldw2 = ldw2; g.out = out; g.ldo = ldo;
    hipStream_t st = as_stream(stream);
    switch (chain_shape(C0, C1, C2)) {
    case 0: chain_pool_launch<Pipe, 32, 32, 64>(g, st); break;
    case 1: chain_pool_launch<Pipe, 64, 64, 128>(g, st); break;
    case 2: chain_pool_launch<Pipe, 64, 96, 128>(g, st); break;
    case 3: chain_pool_launch<Pipe, 128, 128, 256>(g, st); break;
    default: chain_pool_launch<Pipe, 128, 196, 256>(g, st); break;
    }
    return prifit_check_launch();
}

// ---- the per-point tail of the part-segmentation network: four layers over raw rows, scores and / or part labels out
//
// The layout argument does not stop at two layers: a wave carries its 32 rows through fp1's two layers, conv1 + bn1 and
// conv2 with two register generations of activations that swap roles; the last product's C/D layout leaves lane (j, h) with
// the scores of channels 32b + 8g + 4h + m of row j, which it ranks itself before one exchange with lane j of the other half.
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

// one 128 -> 128 layer on the registers: out = relu(W in + bias), a NaN kept
template <typename Pipe>
__device__ __forceinline__ void chain_rows_layer(const typename Pipe::W *__restrict__ W, long long ldw, const float *__restrict__ bias,
                                                 const typename Pipe::Frag (&in)[chain_ksteps<Pipe>(ROWS_W)],
                                                 typename Pipe::Frag (&out)[chain_ksteps<Pipe>(ROWS_W)], int li, int lh)
{
#pragma unroll
    for (int b = 0; b < ROWS_NB; ++b)
        chain_close<Pipe, true, ROWS_W>(chain_block<Pipe, ROWS_W, false>(W, ldw, b, ROWS_W, in, li, lh), bias, b, lh, out);
}

// X [P, 8 KQ] raw rows -> z = W4 relu(W3 relu(W2 relu(W1 x + b1) + b2) + b3) + b4, widths (128, 128, 128, CL <= 64);
// scores[p][0:CL] = z and / or labels[p] = the first maximum of z among the allowed channels (-1: none allowed)
template <typename Pipe, int KQ>
__global__ __launch_bounds__(256) void mlp_chain_rows_kernel(const RowsArgsT<typename Pipe::W> g)
{
    constexpr int K0 = 8 * KQ, H = Pipe::KSTEP / 2;
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

    typename Pipe::Frag ha[chain_ksteps<Pipe>(ROWS_W)], hb[chain_ksteps<Pipe>(ROWS_W)];
    {
        // B operand of layer 1: lane (j, h) holds X[row0 + j][KSTEP t + H h + 0 .. H - 1] in k-step t
        typename Pipe::Frag xf[chain_ksteps<Pipe>(K0)];
        const float *xr = g.X + rowc * g.ldx + H * lh;
#pragma unroll
        for (int t = 0; t < chain_ksteps<Pipe>(K0); ++t) xf[t] = Pipe::template from_mem<false, K0>(xr, t, lh);
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b)
            chain_close<Pipe, true, ROWS_W>(chain_block<Pipe, K0, false>(g.W[0], g.ldw[0], b, ROWS_W, xf, li, lh), g.b[0], b, lh, ha);
    }
    chain_rows_layer<Pipe>(g.W[1], g.ldw[1], g.b[1], ha, hb, li, lh);
    chain_rows_layer<Pipe>(g.W[2], g.ldw[2], g.b[2], hb, ha, li, lh);

    // layer 4, no ReLU: channels >= CL are zero A rows
    RowsRank rk = rows_rank_begin(g, rowc);
#pragma unroll
    for (int b2 = 0; b2 < ROWS_MAX_CL / 32; ++b2) {
        if (32 * b2 >= CL) break;                 // grid-uniform
        rows_emit(g, chain_block<Pipe, ROWS_W, true>(g.W[3], g.ldw[3], b2, CL, ha, li, lh), b2, lh, row, live, s_cat, rk);
    }
    rows_finish(g, rk, lh, row, live);
}

inline int chain_rows_supported(int K0, int L, const int32_t *widths)
{
    if (L != ROWS_L || !widths || K0 < 8 || K0 > ROWS_MAX_K0 || (K0 & 7)) return 0;
    for (int l = 0; l + 1 < ROWS_L; ++l)
        if (widths[l] != ROWS_W) return 0;
    return (widths[ROWS_L - 1] >= 1 && widths[ROWS_L - 1] <= ROWS_MAX_CL) ? 1 : 0;
}

template <typename Pipe, int KQ>
void chain_rows_dispatch(int kq, const RowsArgsT<typename Pipe::W> &g, hipStream_t st)
{
    if (kq == KQ) {
        const unsigned grid = (unsigned)((g.P + CHAIN_ROWS - 1) / CHAIN_ROWS);
        hipLaunchKernelGGL((mlp_chain_rows_kernel<Pipe, KQ>), dim3(grid), dim3(256), 0, st, g);
    } else if constexpr (KQ > 1) chain_rows_dispatch<Pipe, KQ - 1>(kq, g, st);
}

// the argument checks of the row chain, shared by its consumers (the labels' chain, the embedding chain): everything about
// the rows, the four layers' host arrays and the scores / labels outputs -> g, PRIFIT_EINVAL for what they refuse.  The
// shape query is the caller's; CL is the width of the product that feeds scores / labels (its layer may be none of W's).
template <typename Pipe>
int chain_rows_args(RowsArgsT<typename Pipe::W> &g, const float *X, long long ldx, long long P, int K0, const typename Pipe::W *const *W,
                    const long long *ldw, const float *const *b, int CL, float *scores, long long lds, int32_t *labels,
                    const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape)
{
    if (!X || !W || !ldw || !b || P < 1 || P > 0x7fffffffLL || ldx < K0 || (ldx & 3) || mis16(X) || rows_per_shape <= 0)
        return PRIFIT_EINVAL;
    if (scores && lds < CL) return PRIFIT_EINVAL;
    if (labels && (shape_cat != nullptr) != (cat_of_label != nullptr)) return PRIFIT_EINVAL;
    if (labels && shape_cat && P % rows_per_shape) return PRIFIT_EINVAL;
    for (int l = 0; l < ROWS_L; ++l) {
        if (!W[l] || !b[l] || !Pipe::pitch_ok(ldw[l], l ? ROWS_W : K0) || mis16(W[l]) || mis16(b[l])) return PRIFIT_EINVAL;
        g.W[l] = W[l]; g.b[l] = b[l]; g.ldw[l] = ldw[l];
    }
    g.X = X; g.ldx = ldx; g.P = P; g.CL = CL; g.scores = scores; g.lds = lds; g.labels = labels;
    g.cat_of_label = labels ? cat_of_label : nullptr; g.shape_cat = labels ? shape_cat : nullptr; g.N = rows_per_shape;
    return PRIFIT_OK;
}

template <typename Pipe>
int chain_rows_run(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths, const typename Pipe::W *const *W,
                   const long long *ldw, const float *const *b, float *scores, long long lds, int32_t *labels,
                   const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape, void *stream)
{
    if (!chain_rows_supported(K0, L, widths) || (!scores && !labels)) return PRIFIT_EINVAL;
    RowsArgsT<typename Pipe::W> g = {};
    if (chain_rows_args<Pipe>(g, X, ldx, P, K0, W, ldw, b, widths[ROWS_L - 1], scores, lds, labels, cat_of_label, shape_cat,
                              rows_per_shape))
        return PRIFIT_EINVAL;
    chain_rows_dispatch<Pipe, ROWS_MAX_K0 / 8>(K0 / 8, g, as_stream(stream));
    return prifit_check_launch();
}

// ---- the per-point embedding: layers 1 .. 3 of the row chain, then TWO heads on a_3 (the network's `feat`) while it is in
// registers -- head A, the row chain's last layer and emit code (scores and / or labels; optional), and head B,
// e = W_e a_3 + b_e, 128 channels, no ReLU (extra_conv_emb), stored row-major: lane (j, h) writes its four channels
// 32b + 8g + 4h + 0 .. 3 of row j as one 16-byte store, so a row is written as 16-byte pieces, two adjacent ones per store
// instruction (the scores' pattern).
//
// NORM (F.normalize(e, p = 2, dim = channel)): the four head-B blocks stay in accumulators (hb is dead by then).  The order of
// the sum of squares is fixed: lane (j, h) adds the squares of its 64 values to 0 in the order block 0 .. 3, register 0 .. 15
// (channel 32b + 8(r >> 2) + 4h + (r & 3)), one rounded multiply and one rounded add each, no fma; then ONE exchange with
// lane (j, 1 - h), s = own + other -- fp32 addition commutes, so both lanes hold the same bits.  Then sqrt and divide, each
// correctly rounded: e / max(sqrt(s), 1e-12).  A NaN in s makes the divisor NaN (torch's clamp_min keeps it), so the whole
// row is NaN; no other row sees it.
template <typename WT>
struct EmbedArgsT {
    RowsArgsT<WT> r;         // X, layers 1 .. 3 in W/b/ldw[0 .. 2]; head A in W/b/ldw[3], CL (0: no head A), scores, labels ...
    const WT *We;
    const float *be;
    long long ldwe;
    float *emb;
    long long lde;
};

// head B's bias on the finished block b
__device__ __forceinline__ void embed_bias(f32x16 &acc, const float *__restrict__ be, int b, int lh)
{
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const float4 bb = ld4(be + 32 * b + 8 * gq + 4 * lh);
        acc[4 * gq + 0] += bb.x; acc[4 * gq + 1] += bb.y; acc[4 * gq + 2] += bb.z; acc[4 * gq + 3] += bb.w;
    }
}

// s + a a in two roundings whatever -ffp-contract says: the sum of squares has a stated order AND stated roundings
__device__ __forceinline__ float embed_sq_add(float s, float a)
{
#pragma clang fp contract(off)
    const float q = a * a;
    return s + q;
}

__device__ __forceinline__ void embed_store(const f32x16 &acc, float *er, int b, int lh)
{
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
        *reinterpret_cast<float4 *>(er + 32 * b + 8 * gq + 4 * lh) =
            make_float4(acc[4 * gq + 0], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]);
}

template <typename Pipe, int KQ, bool NORM>
__global__ __launch_bounds__(256) void mlp_chain_embed_kernel(const EmbedArgsT<typename Pipe::W> e)
{
    constexpr int K0 = 8 * KQ, H = Pipe::KSTEP / 2;
    const RowsArgsT<typename Pipe::W> &g = e.r;
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

    typename Pipe::Frag ha[chain_ksteps<Pipe>(ROWS_W)], hb[chain_ksteps<Pipe>(ROWS_W)];
    {
        typename Pipe::Frag xf[chain_ksteps<Pipe>(K0)];
        const float *xr = g.X + rowc * g.ldx + H * lh;
#pragma unroll
        for (int t = 0; t < chain_ksteps<Pipe>(K0); ++t) xf[t] = Pipe::template from_mem<false, K0>(xr, t, lh);
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b)
            chain_close<Pipe, true, ROWS_W>(chain_block<Pipe, K0, false>(g.W[0], g.ldw[0], b, ROWS_W, xf, li, lh), g.b[0], b, lh, ha);
    }
    chain_rows_layer<Pipe>(g.W[1], g.ldw[1], g.b[1], ha, hb, li, lh);
    chain_rows_layer<Pipe>(g.W[2], g.ldw[2], g.b[2], hb, ha, li, lh);

    // head A: the row chain's layer 4 and emit code (grid-uniform: present or not)
    if (CL > 0) {
        RowsRank rk = rows_rank_begin(g, rowc);
#pragma unroll
        for (int b2 = 0; b2 < ROWS_MAX_CL / 32; ++b2) {
            if (32 * b2 >= CL) break;
            rows_emit(g, chain_block<Pipe, ROWS_W, true>(g.W[3], g.ldw[3], b2, CL, ha, li, lh), b2, lh, row, live, s_cat, rk);
        }
        rows_finish(g, rk, lh, row, live);
    }

    // head B
    float *er = e.emb + row * e.lde;
    if constexpr (!NORM) {
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {       // a block is stored as it finishes: nothing is kept
            f32x16 acc = chain_block<Pipe, ROWS_W, false>(e.We, e.ldwe, b, ROWS_W, ha, li, lh);
            embed_bias(acc, e.be, b, lh);
            if (live) embed_store(acc, er, b, lh);
            Pipe::block_end();
        }
    } else {
        f32x16 acc[ROWS_NB];
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
            acc[b] = chain_block<Pipe, ROWS_W, false>(e.We, e.ldwe, b, ROWS_W, ha, li, lh);
            embed_bias(acc[b], e.be, b, lh);
        }
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) s = embed_sq_add(s, acc[b][r]);
        s += __shfl_xor(s, 32);                   // every lane of the wave is here: rows past the end compute too
        // sqrtf and / are correctly rounded in a HIP build (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt;
        // __fsqrt_rn is NOT: without OCML_BASIC_ROUNDED_OPERATIONS it is the hardware's approximate square root)
        const float q = __builtin_sqrtf(s);
        const float d = q < 1e-12f ? 1e-12f : q;  // fmaxf(q, 1e-12f) for a number; a NaN stays (fmaxf would drop it)
#pragma unroll
        for (int b = 0; b < ROWS_NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = acc[b][r] / d;
            if (live) embed_store(acc[b], er, b, lh);
        }
    }
}

// widths (128, 128, 128, 128): layers 1 .. 3 and W_e; CL == 0: no head A
inline int chain_embed_supported(int K0, int L, const int32_t *widths, int CL)
{
    if (L != ROWS_L || !widths || widths[ROWS_L - 1] != ROWS_W || CL < 0) return 0;
    const int32_t as_rows[ROWS_L] = {widths[0], widths[1], widths[2], CL ? CL : 1};
    return chain_rows_supported(K0, L, as_rows);
}

template <typename Pipe, int KQ>
void chain_embed_dispatch(int kq, bool norm, const EmbedArgsT<typename Pipe::W> &e, hipStream_t st)
{
    if (kq == KQ) {
        const dim3 grid((unsigned)((e.r.P + CHAIN_ROWS - 1) / CHAIN_ROWS));
        if (norm) hipLaunchKernelGGL((mlp_chain_embed_kernel<Pipe, KQ, true>), grid, dim3(256), 0, st, e);
        else hipLaunchKernelGGL((mlp_chain_embed_kernel<Pipe, KQ, false>), grid, dim3(256), 0, st, e);
    } else if constexpr (KQ > 1) chain_embed_dispatch<Pipe, KQ - 1>(kq, norm, e, st);
}

template <typename Pipe>
int chain_embed_run(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths, const typename Pipe::W *const *W,
                    const long long *ldw, const float *const *b, const typename Pipe::W *W_cls, long long ldw_cls, const float *b_cls,
                    int CL, float *emb, long long lde, int normalize, float *scores, long long lds, int32_t *labels,
                    const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape, void *stream)
{
    if (!chain_embed_supported(K0, L, widths, CL) || !emb || mis16(emb) || lde < ROWS_W || (lde & 3)) return PRIFIT_EINVAL;
    if ((CL > 0) != (scores || labels)) return PRIFIT_EINVAL;      // head A: asked for and described, or neither
    if (CL > 0 && (!W_cls || !b_cls || !Pipe::pitch_ok(ldw_cls, ROWS_W) || mis16(W_cls) || mis16(b_cls))) return PRIFIT_EINVAL;
    EmbedArgsT<typename Pipe::W> e = {};
    if (chain_rows_args<Pipe>(e.r, X, ldx, P, K0, W, ldw, b, CL, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape))
        return PRIFIT_EINVAL;
    e.We = e.r.W[3]; e.be = e.r.b[3]; e.ldwe = e.r.ldw[3]; e.emb = emb; e.lde = lde;
    e.r.W[3] = W_cls; e.r.b[3] = b_cls; e.r.ldw[3] = ldw_cls;
    chain_embed_dispatch<Pipe, ROWS_MAX_K0 / 8>(K0 / 8, normalize != 0, e, as_stream(stream));
    return prifit_check_launch();
}

}  // namespace
