// Classifier-layer pre-training on the frozen network (FrozenPartSeg.probe_step): the per-point tail of
// infer_chain.h -- fp1's two layers, conv1 + bn1, conv2 on the registers of a wave -- ending not in scores but in the
// segmentation loss, the gradient of conv2 and the accuracy count (train_partseg_shapenet.py:56-99 with the network in eval
// mode: only conv2 learns, so nothing in front of it needs a backward).
//
//   probe_head_kernel    a FIXED grid of at most PROBE_GRID workgroups; workgroup g walks the 128-row tiles g, g + grid, ...
//                        Per tile a wave runs the chain on its 32 rows, forms z = W4 a3 + b4, the double log-softmax loss of
//                        models/pointnet2_part_seg_msg.py:129,143, the arg-max and dz = softmax(log_softmax(z)) - onehot, and
//                        stages a3 [128 x 128] and dz [128 x 64] in LDS (the contraction of dW = dz^T a3 runs over ROWS, which
//                        the chain holds across lanes: one transposition).  After one barrier wave w owns columns 32 w .. + 31
//                        of dW: two 32 x 32 accumulator blocks that stay in registers over all tiles of the workgroup
//                        (v_mfma_f32_32x32x2_f32 over the 128 rows), lane c of wave w sums dz[:, c] of the wave's own rows (db).
//                        At the end the workgroup writes ONE partial: dW 64 x 128, db 64, (loss, kept, correct).
//   probe_final_kernel   sums the partials in a fixed order (fp64), divides by the kept rows, writes dW, db, loss.
// No floating-point atomics, no [P, 128] or [P, C_L] tensor, the same bits on every run.
#include "infer_chain.h"
#include "infer_pipe_f32.h"

namespace {

constexpr int PROBE_GRID = 256;                              // workgroups at most: a constant, not the device's CU count
constexpr int PROBE_A3P = ROWS_W + 4, PROBE_DZP = ROWS_MAX_CL + 4;   // LDS pitches = 4 mod 32: the float4 stores of 8 rows tile the banks
constexpr int PROBE_DB = ROWS_MAX_CL * ROWS_W, PROBE_SC = PROBE_DB + ROWS_MAX_CL;
constexpr int PROBE_PART = PROBE_SC + 4;                     // floats of a partial: dW | db | loss (high part), kept, correct, loss (low part)
constexpr long long PROBE_IGNORE = -100;                     // F.cross_entropy's default ignore_index

struct ProbeArgs {
    const float *X;
    long long ldx, P;
    const float *W[ROWS_L];
    const float *b[ROWS_L];
    long long ldw[ROWS_L];
    int CL;
    const long long *target;
    float *part;
};

// element i (0 .. 31) of a lane's scores: block i / 16, register i % 16 -> the channel (infer_chain.h's C/D layout)
__device__ __forceinline__ int probe_channel(int i, int lh) { return 32 * (i >> 4) + 8 * ((i & 15) >> 2) + 4 * lh + (i & 3); }

template <int KQ>
__global__ __launch_bounds__(256) void probe_head_kernel(const ProbeArgs g)
{
    typedef PipeF32 Pipe;
    constexpr int K0 = 8 * KQ, H = Pipe::KSTEP / 2;
    __shared__ __attribute__((aligned(16))) float s_a3[CHAIN_ROWS * PROBE_A3P];      // 66 KB
    __shared__ __attribute__((aligned(16))) float s_dz[CHAIN_ROWS * PROBE_DZP];      // 34 KB
    __shared__ float s_db[4][ROWS_MAX_CL];
    __shared__ double s_loss[4];
    __shared__ int s_cnt[4][2];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int CL = g.CL;
    const bool two = CL > 32;                       // grid-uniform: channels 32 .. 63 exist
    const long long tiles = (g.P + CHAIN_ROWS - 1) / CHAIN_ROWS;

    f32x16 dw0 = ZERO16, dw1 = ZERO16;              // dW[32 blk + 8 (r / 4) + 4 lh + r % 4][32 wave + li], summed over this workgroup's tiles
    float db_acc = 0.f;                             // db[lane], this wave's rows
    double loss_acc = 0.0;
    int kept_acc = 0, corr_acc = 0;

    float *const a3w = s_a3 + (32 * wave + li) * PROBE_A3P + 4 * lh;
    float *const dzw = s_dz + (32 * wave + li) * PROBE_DZP + 4 * lh;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row0 = tile * CHAIN_ROWS + 32 * wave;
        if (row0 < g.P) {                           // wave-uniform
            const long long row = row0 + li;
            const bool live = row < g.P;            // a row past the end computes on a copy of the last row and contributes zeros
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

            // a3: fragment t of lane (j, h) = channels 8 t + 4 h + 0 .. 3 of row j
#pragma unroll
            for (int t = 0; t < chain_ksteps<Pipe>(ROWS_W); ++t)
                *reinterpret_cast<float4 *>(a3w + 8 * t) =
                    make_float4(live ? ha[t].x : 0.f, live ? ha[t].y : 0.f, live ? ha[t].z : 0.f, live ? ha[t].w : 0.f);

            // layer 4, no ReLU: channels >= CL are zero A rows; z as prifit_mlp_chain_rows_f32 forms it, bit for bit
            const f32x16 acc0 = chain_block<Pipe, ROWS_W, true>(g.W[3], g.ldw[3], 0, CL, ha, li, lh);
            f32x16 acc1 = ZERO16;
            if (two) acc1 = chain_block<Pipe, ROWS_W, true>(g.W[3], g.ldw[3], 1, CL, ha, li, lh);
            float z[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int ch = probe_channel(i, lh);
                z[i] = (i < 16 ? acc0[i & 15] : acc1[i & 15]) + (ch < CL ? g.b[3][ch] : 0.f);
            }

            const long long t = g.target[rowc];
            const bool ignored = t == PROBE_IGNORE || !live, valid = t >= 0 && t < CL;

            // the row's maximum, its first arg-max (rows_emit's key: a NaN beats every number, the lower channel wins a tie)
            // and the labelled score; lanes j and j + 32 hold the two halves of row j's channels
            float m = -INFINITY, zt = 0.f;
            unsigned long long best = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int ch = probe_channel(i, lh);
                if (ch < CL) {
                    m = fmaxf(m, z[i]);
                    const unsigned long long k = ((unsigned long long)rows_score_key(z[i]) << 32) | (unsigned)(63 - ch);
                    best = k > best ? k : best;
                    if (ch == t) zt = z[i];
                }
            }
            m = fmaxf(m, __shfl_xor(m, 32));
            zt += __shfl_xor(zt, 32);               // one of the two is 0
            {
                const unsigned hi = __shfl_xor((unsigned)(best >> 32), 32), lo = __shfl_xor((unsigned)best, 32);
                const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                best = other > best ? other : best;
            }
            const int pred = 63 - (int)(best & 63u);

            // y = log_softmax(z): the exponentials in fp32, their sum and the logarithm in fp64
            double S = 0.0;
#pragma unroll
            for (int i = 0; i < 32; ++i)
                if (probe_channel(i, lh) < CL) S += (double)expf(z[i] - m);
            S += __shfl_xor(S, 32);
            const double lse1 = (double)m + log(S);
            // the second softmax, on y rounded to fp32 as the network returns it: logsumexp(y) - y[t] and softmax(y)
            double S2 = 0.0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                z[i] = probe_channel(i, lh) < CL ? expf((float)((double)z[i] - lse1)) : 0.f;
                S2 += (double)z[i];
            }
            S2 += __shfl_xor(S2, 32);
            const double row_loss = valid ? log(S2) - ((double)zt - lse1) : (double)__builtin_nanf("");
            if (lh == 0 && !ignored) {
                loss_acc += row_loss;
                kept_acc += 1;
                corr_acc += (valid && pred == (int)t) ? 1 : 0;
            }
            // dz = softmax(y) - onehot (divided by the kept rows at the very end): zeros for a dropped row, NaN for a bad label
            const float s2 = (float)S2;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int ch = probe_channel(i, lh);
                float d = z[i] / s2 - (ch == t ? 1.f : 0.f);
                if (!valid) d = __builtin_nanf("");
                z[i] = (ignored || ch >= CL) ? 0.f : d;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < 4 || two) *reinterpret_cast<float4 *>(dzw + 8 * q) = make_float4(z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]);
        } else {                                    // a wave without rows in a ragged last tile: zero operands
#pragma unroll
            for (int t = 0; t < chain_ksteps<Pipe>(ROWS_W); ++t) *reinterpret_cast<float4 *>(a3w + 8 * t) = zero4;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < 4 || two) *reinterpret_cast<float4 *>(dzw + 8 * q) = zero4;
        }
        __syncthreads();

        // dW[c][32 wave + n] += sum over the tile's rows r of dz[r][c] a3[r][32 wave + n]: A = dz^T, lane (c, h) reads row 2 s + h
        {
            const float *ap = s_dz + lh * PROBE_DZP + li;
            const float *bp = s_a3 + lh * PROBE_A3P + 32 * wave + li;
#pragma unroll 8
            for (int s = 0; s < CHAIN_ROWS / 2; ++s) {
                const float bv = bp[2 * s * PROBE_A3P];
                dw0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * PROBE_DZP], bv, dw0, 0, 0, 0);
                if (two) dw1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * PROBE_DZP + 32], bv, dw1, 0, 0, 0);
            }
            // db[lane] over this wave's 32 rows, in row order
            const float *dp = s_dz + 32 * wave * PROBE_DZP + lane;
            if (lane < 32 || two) {
#pragma unroll 8
                for (int r = 0; r < 32; ++r) db_acc += dp[r * PROBE_DZP];
            }
        }
        __syncthreads();                            // the next tile overwrites the operands
    }

    // this workgroup's partial
    float *part = g.part + (long long)blockIdx.x * PROBE_PART;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = 8 * (r >> 2) + 4 * lh + (r & 3);
        part[c * ROWS_W + 32 * wave + li] = dw0[r];
        if (two) part[(32 + c) * ROWS_W + 32 * wave + li] = dw1[r];
    }
    s_db[wave][lane] = db_acc;
    loss_acc = wave_sum_f64(loss_acc);
    kept_acc = wave_sum_i32_dpp(kept_acc);
    corr_acc = wave_sum_i32_dpp(corr_acc);
    if (lane == 0) { s_loss[wave] = loss_acc; s_cnt[wave][0] = kept_acc; s_cnt[wave][1] = corr_acc; }
    __syncthreads();
    if (threadIdx.x < ROWS_MAX_CL)
        part[PROBE_DB + threadIdx.x] = (s_db[0][threadIdx.x] + s_db[1][threadIdx.x]) + (s_db[2][threadIdx.x] + s_db[3][threadIdx.x]);
    if (threadIdx.x == 0) {
        const double l = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        const float hi = (float)l;
        part[PROBE_SC + 0] = hi;
        part[PROBE_SC + 1] = (float)((s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]));
        part[PROBE_SC + 2] = (float)((s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]));
        part[PROBE_SC + 3] = (hi - hi == 0.f) ? (float)(l - (double)hi) : 0.f;      // (a finite high part)
    }
}

// the sum of v over the 256 threads of the workgroup, in a fixed tree order, in every thread
__device__ __forceinline__ double probe_block_sum(double v, double *s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// element id of (dW [CL x 128] | db [64]) = the sum over the G partials, in their order, over the kept rows; block 0 also
// writes loss [4] = (mean loss, kept rows, correct rows, 0).  No kept row: 0 / 0 = NaN for the loss as torch, the sums as they are (zeros)
__global__ __launch_bounds__(256) void probe_final_kernel(const float *__restrict__ part, int G, int CL, float *__restrict__ dW,
                                                          long long lddw, float *__restrict__ db, float *__restrict__ loss)
{
    __shared__ double s_red[256];
    const int tid = threadIdx.x;
    const float *sc = part + (long long)tid * PROBE_PART + PROBE_SC;
    const double kept = probe_block_sum(tid < G ? (double)sc[1] : 0.0, s_red);
    if (blockIdx.x == 0) {
        const double l = probe_block_sum(tid < G ? (double)sc[0] + (double)sc[3] : 0.0, s_red);
        const double correct = probe_block_sum(tid < G ? (double)sc[2] : 0.0, s_red);
        if (tid == 0) { loss[0] = (float)(l / kept); loss[1] = (float)kept; loss[2] = (float)correct; loss[3] = 0.f; }
    }
    const int id = blockIdx.x * 256 + tid;
    if (id >= PROBE_SC) return;
    const int c = id < PROBE_DB ? id / ROWS_W : id - PROBE_DB;
    if (c >= CL) return;
    double a = 0.0;
    for (int w = 0; w < G; ++w) a += (double)part[(long long)w * PROBE_PART + id];
    const float v = (float)(kept > 0.0 ? a / kept : a);
    if (id < PROBE_DB) dW[(long long)c * lddw + (id - c * ROWS_W)] = v;
    else db[c] = v;
}

inline long long probe_grid(long long P)
{
    const long long tiles = P < 1 ? 1 : (P + CHAIN_ROWS - 1) / CHAIN_ROWS;
    return tiles < PROBE_GRID ? tiles : PROBE_GRID;
}

template <int KQ>
void probe_dispatch(int kq, const ProbeArgs &g, unsigned grid, hipStream_t st)
{
    if (kq == KQ) hipLaunchKernelGGL((probe_head_kernel<KQ>), dim3(grid), dim3(256), 0, st, g);
    else if constexpr (KQ > 1) probe_dispatch<KQ - 1>(kq, g, grid, st);
}

}  // namespace

extern "C" {

int prifit_probe_head_supported(int K0, int L, const int32_t *widths) { return chain_rows_supported(K0, L, widths); }

long long prifit_probe_head_workspace(long long P, int K0, int L, const int32_t *widths)
{
    return chain_rows_supported(K0, L, widths) ? probe_grid(P) * PROBE_PART : 0;
}

int prifit_probe_head_f32(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths, const float *const *W,
                          const long long *ldw, const float *const *b, const long long *target, float *dW, long long lddw, float *db,
                          float *loss, float *workspace, void *stream)
{
    if (!chain_rows_supported(K0, L, widths) || !X || !W || !ldw || !b || !target || !dW || !db || !loss || !workspace || P < 1 ||
        P > 0x7fffffffLL || ldx < K0 || (ldx & 3) || mis16(X) || lddw < ROWS_W || mis16(dW))
        return PRIFIT_EINVAL;
    ProbeArgs g = {};
    for (int l = 0; l < ROWS_L; ++l) {
        if (!W[l] || !b[l] || !PipeF32::pitch_ok(ldw[l], l ? ROWS_W : K0) || mis16(W[l]) || mis16(b[l])) return PRIFIT_EINVAL;
        g.W[l] = W[l]; g.b[l] = b[l]; g.ldw[l] = ldw[l];
    }
    g.X = X; g.ldx = ldx; g.P = P; g.CL = widths[ROWS_L - 1]; g.target = target; g.part = workspace;
    const unsigned grid = (unsigned)probe_grid(P);
    hipStream_t st = as_stream(stream);
    probe_dispatch<ROWS_MAX_K0 / 8>(K0 / 8, g, grid, st);
    hipLaunchKernelGGL(probe_final_kernel, dim3((PROBE_SC + 255) / 256), dim3(256), 0, st, workspace, (int)grid, g.CL, dW, lddw, db, loss);
    return prifit_check_launch();
}

}  // extern "C"
