// The ordered MFMA chains of the layer-by-layer MLP (mlp_gemm.h), device code only: one 16 x 16 output tile as a chain of
// 16 x 16 x 4 f32 MFMA steps over an A tile in LDS and a weight matrix in memory.  Shared by the GEMM launches of mlp_gemm.h and
// the fused EVOPF evaluation (evopf_eval.hip), which runs the same chains on activations that never leave LDS: the same
// operands in the same order, so the same bits.
#pragma once
#include "mlp_tile.h"

namespace rpo_mlp_dev {

#ifndef RPO_GEMM_SKIP
#define RPO_GEMM_SKIP 0            // debug builds only (tools/probe/build_stream_variants.sh KIND=gemm): timing with a phase left
#endif                             // out -- 1 no A loads, 2 no weight loads, 4 no MFMA chain, 8 no stores, 16 no epilogue operands

// One operand pair of a 16 x 16 output tile.  The k range runs in chunks of CH blocks of 16: the weight operands of chunk c + 1
// are requested before the MFMAs of chunk c are issued (register ping-pong), in a ROLLED loop.  Two things this replaces, both
// measured at 24 us for the hidden layer (K = 512): loads inside the k loop (32 dependent L2 round trips), and the fully
// unrolled form (3 700 instructions executed once per workgroup: bound by instruction fetch, every line a cold miss).
// Addresses are clamped instead of guarded (no branches); the A tile in LDS is zero beyond K, so operands beyond K multiply zeros.
// VEC: W is [N][K] with 16-byte aligned rows and K % 16 == 0.
template <bool W_NK, bool VEC, int CH>
__device__ __forceinline__ void gemm_load_chunk(float (&b)[CH][4], const float* __restrict__ W, int ldw, int K, int nc, int c, int lg) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int kb = (c * CH + u) * 16 + lg * 4;
        if (RPO_GEMM_SKIP & 2) {
            b[u][0] = b[u][1] = b[u][2] = b[u][3] = 0.001f * (float)(kb + nc);
        } else if (VEC) {
            const int kc = kb + 3 < K ? kb : 0;
            const float4 v = *reinterpret_cast<const float4*>(&W[(size_t)nc * ldw + kc]);
            b[u][0] = v.x; b[u][1] = v.y; b[u][2] = v.z; b[u][3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = kb + q, kc = k < K ? k : K - 1;
                b[u][q] = W_NK ? W[(size_t)nc * ldw + kc] : W[(size_t)kc * ldw + nc];
            }
        }
    }
}

template <int CH>
__device__ __forceinline__ f32x4 gemm_mfma_chunk(const float (&b)[CH][4], const float* a_s, int ldk, int c, int li, int lg, f32x4 acc) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const float4 a4 = *reinterpret_cast<const float4*>(&a_s[li * ldk + (c * CH + u) * 16 + lg * 4]);
        if (RPO_GEMM_SKIP & 4) { acc[0] += a4.x * b[u][0]; acc[1] += a4.y * b[u][1]; acc[2] += a4.z * b[u][2]; acc[3] += a4.w * b[u][3]; continue; }
        acc = mfma4(a4.x, b[u][0], acc);
        acc = mfma4(a4.y, b[u][1], acc);
        acc = mfma4(a4.z, b[u][2], acc);
        acc = mfma4(a4.w, b[u][3], acc);
    }
    return acc;
}

// chunks [c0, c1) of the k range (the whole range: 0, ceil(K / (16 CH)))
template <bool W_NK, bool VEC, int CH>
__device__ __forceinline__ f32x4 gemm_chain_range(const float* a_s, int ldk, const float* __restrict__ W, int ldw, int K, int N, int n,
                                                  int li, int lg, f32x4 acc, int c0, int c1) {
    const int nc = n < N ? n : N - 1;
    float b0[CH][4], b1[CH][4];
    if (c0 < c1) gemm_load_chunk<W_NK, VEC, CH>(b0, W, ldw, K, nc, c0, lg);
    for (int c = c0; c < c1; c += 2) {                            // (columns n >= N compute garbage that is never stored)
        if (c + 1 < c1) gemm_load_chunk<W_NK, VEC, CH>(b1, W, ldw, K, nc, c + 1, lg);
        acc = gemm_mfma_chunk<CH>(b0, a_s, ldk, c, li, lg, acc);
        if (c + 1 < c1) {
            if (c + 2 < c1) gemm_load_chunk<W_NK, VEC, CH>(b0, W, ldw, K, nc, c + 2, lg);
            acc = gemm_mfma_chunk<CH>(b1, a_s, ldk, c + 1, li, lg, acc);
        }
    }
    return acc;
}

template <bool W_NK, bool VEC, int CH>
__device__ __forceinline__ f32x4 gemm_chain(const float* a_s, int ldk, const float* __restrict__ W, int ldw, int K, int N, int n, int li,
                                            int lg, f32x4 acc) {
    return gemm_chain_range<W_NK, VEC, CH>(a_s, ldk, W, ldw, K, N, n, li, lg, acc, 0, (K + 16 * CH - 1) / (16 * CH));
}

}  // namespace rpo_mlp_dev
