// The fp32 policy of the chain skeleton (infer_chain.h), shared by infer.hip and probe_head.hip.
#pragma once
#include "infer_chain.h"

namespace {

// The fp32 matrix pipe of the chains (infer_chain.h): v_mfma_f32_32x32x2_f32, two k per instruction, so a k-step of 8 columns
// is four of them on the float4 a lane half loads.  Register 4g + m of lane half h of a finished block is channel
// 8g + 4h + m -- the column the lane reads anyway: the "accumulator order" and the plain column order coincide, and a
// weight is read as the fold wrote it (rows padded to 4 floats, NOT to a whole k-step: C1 = 196 ends in half a step).
struct PipeF32 {
    typedef float W;
    typedef float4 Frag;
    static constexpr int KSTEP = 8;
    static constexpr bool PADDED = false;
    static __device__ __forceinline__ Frag zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ Frag load_w(const W *p, int t) { return ld4(p + 8 * t); }
    template <bool RELU, int K>      // K % 8 == 0: no fragment reaches past the row's end
    static __device__ __forceinline__ Frag from_mem(const float *xr, int t, int)
    {
        static_assert(K % 8 == 0, "whole k-steps");
        const float4 v = ld4(xr + 8 * t);
        return RELU ? relu4(v) : v;
    }
    static __device__ __forceinline__ Frag from_acc(const f32x16 &acc, int s)
    {
        return make_float4(acc[4 * s + 0], acc[4 * s + 1], acc[4 * s + 2], acc[4 * s + 3]);
    }
    static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 acc)
    {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ void block_end() {}      // the blocks of a layer stay in accumulators: nothing to fence
    static bool pitch_ok(long long ld, int kin) { return ld >= kin && !(ld & 3); }
};

}  // namespace
