// Part-segmentation metrics in ONE launch (testing.py:139-204): the category-restricted arg-max of every point's part scores and
// the integer counts the evaluation's numbers are made of -- per shape and part the intersection and union of prediction and
// target, over the batch the hits and the per-part seen / correct counts.  As torch operators that is two [B, N, P] int64
// one-hot tensors, their & and |, a masked argmax, two bincounts and five read-backs per batch.
//
// Layout: a wave takes one row at a time with its lanes across the row's P <= 64 columns (a row is P contiguous floats: lane
// per row would be a 4 P byte stride between lanes), all SEG_WAVE_ROWS rows of the wave requested up front.  Per row:
//   key  = the score as an order-preserving uint32 (NaN = the largest key, -0 = +0, a column outside the shape's category = 0,
//          below the key of -inf);
//   pred = the first lane holding the wave's maximum key (a DPP max, then a ballot): np.argmax's first maximum, its NaN rule,
//          and the first allowed part for a row of -inf;
//   lane l counts in registers [pred == l == target], [pred == l], [target == l]: lane = part, no atomics in the row loop.
// The targets of a wave's rows are loaded once, one per lane, and handed round with readlane; pred is collected one row per lane
// and stored the same way.  A workgroup = SEG_WAVES waves = SEG_ROWS consecutive rows of ONE shape; its waves merge their lane
// counters in LDS and the first P threads flush them once: 32-bit integer atomics into inter / uni [B, P], 64-bit ones into the
// running totals.  Integer sums: the same bits in every run and in every order.
#include "common.h"

namespace {

constexpr int SEG_WAVES = 8;
constexpr int SEG_BLOCK = SEG_WAVES * PRIFIT_WAVE;
constexpr int SEG_WAVE_ROWS = 32;                       // rows per wave: their targets fit one per lane
constexpr int SEG_ROWS = SEG_WAVES * SEG_WAVE_ROWS;     // rows per workgroup

struct SegArgs {
    const float *scores;
    long long ld;
    const long long *target;
    const int32_t *cat_of_label;
    long long *pred;
    int32_t *shape_cat, *inter, *uni;
    unsigned long long *totals;
    int N, P, restricted, chunks;
};

// order-preserving key of a score among the ALLOWED columns: always >= 0x007fffff (-inf), so 0 is free for the others
__device__ __forceinline__ unsigned score_key(float x)
{
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;      // NaN beats every number (numpy's order)
    if ((u << 1) == 0) return 0x80000000u;                        // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_metrics_kernel(SegArgs a)
{
    __shared__ int hist[3][PRIFIT_WAVE];
    __shared__ int bad_rows;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    const int P = a.P, N = a.N;
    if (t < 3 * PRIFIT_WAVE) (&hist[0][0])[t] = 0;
    if (t == 0) bad_rows = 0;

    const long long row0 = (long long)b * N;
    const int n0 = chunk * SEG_ROWS + wave * SEG_WAVE_ROWS;       // this wave's rows: n0 .. n0 + rows - 1 of shape b
    const int rows = min(SEG_WAVE_ROWS, N - n0);                  // <= 0: a wave past the ragged tail
    // every score of the wave's rows is requested before anything waits: the label -> category -> mask chain below is two
    // dependent loads, and the rows behind it would otherwise start one memory latency after the other
    float x[SEG_WAVE_ROWS];
    if (rows > 0) {
        const float *base = a.scores + (row0 + n0) * a.ld + lane;
#pragma unroll
        for (int j = 0; j < SEG_WAVE_ROWS; ++j) x[j] = (lane < P && j < rows) ? base[(long long)j * a.ld] : 0.0f;
    }
    int tl = -1;                                                  // lane j: the label of row n0 + j, -1 = outside [0, P)
    if (lane < rows) {
        const long long v = a.target[row0 + n0 + lane];
        tl = (v >= 0 && v < P) ? (int)v : -1;
    }
    const long long first = a.target[row0];
    const int cat = (first >= 0 && first < P) ? a.cat_of_label[first] : -1;
    if (chunk == 0 && t == 0) a.shape_cat[b] = cat;
    const bool shape_ok = !a.restricted || cat >= 0;
    const bool allowed = lane < P && (!a.restricted || a.cat_of_label[lane] == cat);

    int c_inter = 0, c_pred = 0, c_tgt = 0, bad = 0, pred_lane = -1;
    if (rows > 0) {
#pragma unroll
        for (int j = 0; j < SEG_WAVE_ROWS; ++j) {                 // j and rows are wave-uniform
            const unsigned key = allowed ? score_key(x[j]) : 0u;
            const unsigned top = wave_max_u32_dpp(key);           // every lane takes part, whatever j is
            const unsigned long long at = __ballot(key == top);
            if (j >= rows) continue;
            const int p = shape_ok ? (int)__builtin_ctzll(at) : -1;
            const int tgt = __builtin_amdgcn_readlane(tl, j);
            if (lane == j) pred_lane = p;
            if (tgt < 0 || !shape_ok) {                           // the reference would stop here (KeyError): counted, nothing else
                ++bad;
                continue;
            }
            c_inter += (lane == p) & (lane == tgt);
            c_pred += lane == p;
            c_tgt += lane == tgt;
        }
    }
    if (a.pred && lane < rows) a.pred[row0 + n0 + lane] = pred_lane;

    __syncthreads();                                              // the zeroed histograms
    if (c_inter) atomicAdd(&hist[0][lane], c_inter);
    if (c_pred) atomicAdd(&hist[1][lane], c_pred);
    if (c_tgt) atomicAdd(&hist[2][lane], c_tgt);
    if (lane == 0 && bad) atomicAdd(&bad_rows, bad);
    __syncthreads();
    if (t >= PRIFIT_WAVE) return;
    const int i = hist[0][lane], u = hist[1][lane] + hist[2][lane] - i, seen = hist[2][lane];
    if (lane < P) {                                               // (counts of lanes >= P are 0: pred and target are < P)
        if (i) atomicAdd(&a.inter[(long long)b * P + lane], i);
        if (u) atomicAdd(&a.uni[(long long)b * P + lane], u);
        if (seen) atomicAdd(&a.totals[2 + lane], (unsigned long long)seen);
        if (i) atomicAdd(&a.totals[2 + P + lane], (unsigned long long)i);
    }
    const int hits = wave_sum_i32_dpp(i);
    if (lane == 0) {
        if (hits) atomicAdd(&a.totals[0], (unsigned long long)hits);
        if (bad_rows) atomicAdd(&a.totals[1], (unsigned long long)bad_rows);
    }
}

}  // namespace

extern "C" int prifit_seg_metrics(const float *scores, long long ld, const long long *target, int B, int N, int P,
                                  const int32_t *cat_of_label, int restricted, long long *pred, int32_t *shape_cat, int32_t *inter,
                                  int32_t *uni, long long *totals, void *stream)
{
    if (!scores || !target || !cat_of_label || !shape_cat || !inter || !uni || !totals || B <= 0 || N <= 0 || P < 1 ||
        P > PRIFIT_WAVE || ld < P)
        return PRIFIT_EINVAL;
    const long long chunks = ((long long)N + SEG_ROWS - 1) / SEG_ROWS;
    if (chunks * B > 0x7fffffffLL) return PRIFIT_EINVAL;
    SegArgs a{scores, ld, target, cat_of_label, pred, shape_cat, inter, uni, reinterpret_cast<unsigned long long *>(totals),
              N, P, restricted != 0, (int)chunks};
    hipLaunchKernelGGL(seg_metrics_kernel, dim3((unsigned)(chunks * B)), dim3(SEG_BLOCK), 0, as_stream(stream), a);
    return prifit_check_launch();
}
