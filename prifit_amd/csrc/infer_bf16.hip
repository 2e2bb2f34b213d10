// Frozen inference with bf16 arithmetic (prifit_amd/inference.py precision="bf16"): the on-chip chains of
// infer_chain.h on v_mfma_f32_32x32x16_bf16, fp32 accumulation, the same transposed products H^T = W1' X^T, Y^T = W2' H^T.
//
//   pack_bf16_multi_kernel  every chained layer's folded weight -> bf16 in the column order its MFMA reads, ONE launch
//   PipeBf16                the matrix-pipe policy the two chain kernels of infer_chain.h are instantiated for here
//
// The register-resident design carries over because the C/D layout of the 32x32 MFMAs does not depend on the input type:
// register r of lane (j, h) of a 32x32 result is channel (r & 3) + 8 (r >> 2) + 4h of activation row j.  The B operand of
// v_mfma_f32_32x32x16_bf16 wants B[k = 8h + e][col j] in element e = 0..7 of lane (j, h), so registers 8s .. 8s + 7 of a
// result, rounded to bf16 pairwise, ARE the B fragment of k-step s of the next product -- for the k order
//     element e of lane half h in k-step t  =  channel 16t + 8(e >> 2) + 4h + (e & 3)
// (t = 2b + s over the 32-channel blocks b), which the A operand follows: the pack kernel stores the weight's columns in
// that order, 16 per k-step, so a lane fetches its 8 elements with one 16-byte load at column 16t + 8h.  A first layer is
// fed from memory in the plain order (element e of half h = column 16t + 8h + e) and its weight is packed plainly.
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

inline long long up16(long long k) { return (k + 15) & ~15LL; }

// The bf16 matrix pipe of the chains (infer_chain.h): one v_mfma_f32_32x32x16_bf16 per k-step of 16 columns, a lane half
// holds 8 of them.  Weight rows are zero from their input width to the next multiple of 16 (the pack kernel above).
struct PipeBf16 {
    typedef uint16_t W;
    typedef bf16x8 Frag;
    static constexpr int KSTEP = 16;
    static constexpr bool PADDED = true;
    static __device__ __forceinline__ Frag zero() { return __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u)); }
    static __device__ __forceinline__ Frag load_w(const W *p, int t) { return *reinterpret_cast<const bf16x8 *>(p + 16 * t); }
    // eight floats -> one B fragment (v_cvt_pk_bf16_f32: round to nearest even, a NaN stays a NaN).  An upper lane half that
    // lies past the row's end loads nothing (the next row, or memory that is not ours, could hold a NaN) and holds zeros.
    template <bool RELU, int K>
    static __device__ __forceinline__ Frag from_mem(const float *xr, int t, int lh)
    {
        static_assert(K % 8 == 0, "a lane half is in or out of the row as a whole");
        if (16 * t + 16 <= K || lh == 0) {
            float4 lo = ld4(xr + 16 * t), hi = ld4(xr + 16 * t + 4);
            if (RELU) lo = relu4(lo), hi = relu4(hi);
            const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            return __builtin_convertvector(v, bf16x8);
        }
        return zero();
    }
    // an activation is rounded to bf16 ONCE, when its layer ends, not per use
    static __device__ __forceinline__ Frag from_acc(const f32x16 &a, int s)
    {
        const f32x8 v = {a[8 * s + 0], a[8 * s + 1], a[8 * s + 2], a[8 * s + 3], a[8 * s + 4], a[8 * s + 5], a[8 * s + 6], a[8 * s + 7]};
        return __builtin_convertvector(v, bf16x8);
    }
    static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 acc)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    // a finished block is dead once it is rounded to fragments: the fence keeps the scheduler from running the blocks of a
    // layer side by side, one more live accumulator each (64 AGPRs and an occupancy step at (128, 128, 256))
    static __device__ __forceinline__ void block_end() { __builtin_amdgcn_sched_barrier(0); }
    static bool pitch_ok(long long ld, int kin) { return ld >= up16(kin) && !(ld & 7); }
};

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

// the same five triples (every C0 is a multiple of 16) and the same tails as fp32
int prifit_mlp_chain_pool_bf16_supported(int C0, int C1, int C2, int pool_K) { return chain_pool_supported(C0, C1, C2, pool_K); }

long long prifit_mlp_chain_pool_bf16_workspace(int, int, int, int, int) { return 0; }     // the intermediates live in registers

int prifit_mlp_chain_pool_bf16(const float *X, long long ldx, int G, int pool_K, int C0, int C1, int C2, const uint16_t *W1,
                               long long ldw1, const float *b1, const uint16_t *W2, long long ldw2, const float *b2, float *out,
                               long long ldo, float *, void *stream)
{
    return chain_pool_run<PipeBf16>(X, ldx, G, pool_K, C0, C1, C2, W1, ldw1, b1, W2, ldw2, b2, out, ldo, stream);
}

int prifit_mlp_chain_rows_bf16_supported(int K0, int L, const int32_t *widths) { return chain_rows_supported(K0, L, widths); }

long long prifit_mlp_chain_rows_bf16_workspace(long long, int, int, const int32_t *) { return 0; }     // likewise

int prifit_mlp_chain_rows_bf16(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                               const uint16_t *const *W, const long long *ldw, const float *const *b, float *scores, long long lds,
                               int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat, int rows_per_shape, float *,
                               void *stream)
{
    return chain_rows_run<PipeBf16>(X, ldx, P, K0, L, widths, W, ldw, b, scores, lds, labels, cat_of_label, shape_cat, rows_per_shape,
                                    stream);
}

int prifit_mlp_chain_embed_bf16_supported(int K0, int L, const int32_t *widths, int CL)
{
    return chain_embed_supported(K0, L, widths, CL);
}

long long prifit_mlp_chain_embed_bf16_workspace(long long, int, int, const int32_t *, int) { return 0; }     // likewise

int prifit_mlp_chain_embed_bf16(const float *X, long long ldx, long long P, int K0, int L, const int32_t *widths,
                                const uint16_t *const *W, const long long *ldw, const float *const *b, const uint16_t *W_cls,
                                long long ldw_cls, const float *b_cls, int CL, float *emb, long long lde, int normalize, float *scores,
                                long long lds, int32_t *labels, const int32_t *cat_of_label, const int32_t *shape_cat,
                                int rows_per_shape, float *, void *stream)
{
    return chain_embed_run<PipeBf16>(X, ldx, P, K0, L, widths, W, ldw, b, W_cls, ldw_cls, b_cls, CL, emb, lde, normalize, scores, lds,
                                     labels, cat_of_label, shape_cat, rows_per_shape, stream);
}

}  // extern "C"
