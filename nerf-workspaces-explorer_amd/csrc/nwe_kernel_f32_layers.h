// The layer arithmetic of the fp32 kernels (nwe_kernel_f32.hip, nwe_kernel_f32_occ.hip): one 256-thread workgroup, 16 rays.
#pragma once
#include "nwe_device.h"
#include "nwe_host.h"

namespace nwe {

constexpr int kRP = 16;  // rays per workgroup

__device__ __forceinline__ void dense16(const float* __restrict__ blob, const LayerF32& L, const float* in1, int K1,
                                        const float* in2, int K2, float* out, bool relu) {
    const int n = threadIdx.x;
    if (n < L.N) {
        const float* wt = blob + L.wt_off;
        float acc[kRP];
        const float bias = blob[L.b_off + n];
#pragma unroll
        for (int p = 0; p < kRP; ++p) acc[p] = bias;
        for (int k = 0; k < K1; ++k) {
            const float w = wt[(int64_t)k * L.N + n];
            const float4* h = reinterpret_cast<const float4*>(in1 + k * kRP);
#pragma unroll
            for (int q = 0; q < kRP / 4; ++q) {
                const float4 v = h[q];
                acc[4 * q + 0] = __fmaf_rn(w, v.x, acc[4 * q + 0]);
                acc[4 * q + 1] = __fmaf_rn(w, v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = __fmaf_rn(w, v.z, acc[4 * q + 2]);
                acc[4 * q + 3] = __fmaf_rn(w, v.w, acc[4 * q + 3]);
            }
        }
        for (int k = 0; k < K2; ++k) {
            const float w = wt[(int64_t)(K1 + k) * L.N + n];
            const float4* h = reinterpret_cast<const float4*>(in2 + k * kRP);
#pragma unroll
            for (int q = 0; q < kRP / 4; ++q) {
                const float4 v = h[q];
                acc[4 * q + 0] = __fmaf_rn(w, v.x, acc[4 * q + 0]);
                acc[4 * q + 1] = __fmaf_rn(w, v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = __fmaf_rn(w, v.z, acc[4 * q + 2]);
                acc[4 * q + 3] = __fmaf_rn(w, v.w, acc[4 * q + 3]);
            }
        }
        float4* o = reinterpret_cast<float4*>(out + n * kRP);
#pragma unroll
        for (int q = 0; q < kRP / 4; ++q) {
            float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if (relu) {   // a NaN stays NaN as in torch's relu (fmaxf would make it 0), like act() of the MFMA kernels
                v.x = __builtin_elementwise_maximum(v.x, 0.f); v.y = __builtin_elementwise_maximum(v.y, 0.f);
                v.z = __builtin_elementwise_maximum(v.z, 0.f); v.w = __builtin_elementwise_maximum(v.w, 0.f);
            }
            o[q] = v;
        }
    }
    __syncthreads();
}

// gamma(v) rows [f][16]: nerf/models/embedding.py:24-48.  f = 0..2 identity, then per band sin(3), cos(3).
__device__ __forceinline__ void encode16(float* dst, const float* src3 /*[3][16]*/, int n_feat, float inv_div) {
    const int p = threadIdx.x & (kRP - 1);
    for (int f = threadIdx.x / kRP; f < n_feat; f += 256 / kRP) {
        float val;
        if (f < 3) {
            val = __fdiv_rn(src3[f * kRP + p], inv_div);
        } else {
            const int q = f - 3, band = q / 6, within = q % 6, c = within % 3;
            const float v = __fdiv_rn(src3[c * kRP + p], inv_div);                   // embedding.py:48
            const float arg = __fmul_rn(v, (float)(1 << band));                       // exact (power of two)
            val = within >= 3 ? cosf(arg) : sinf(arg);
        }
        dst[f * kRP + p] = val;
    }
}

}  // namespace nwe
