// The streaming forward of mlp_stream.h with a SECOND ARITHMETIC for its hidden layer (opt-in, rpo_tuning(RPO_TUNE_FWD_BF16X3, 1);
// VERDICT r06 "next round" 1: one bounded experiment past the f32 MFMA ceiling): every f32 operand of h1 = relu(x0) W0^T is split
// EXACTLY into three bf16 planes, a = a_hi + a_mid + a_lo, and the six plane products with plane indices i + j <= 2 run on
// v_mfma_f32_16x16x32_bf16 (f32 accumulation).  f32-accurate, NOT bit-equal to the exact form: tests/test_forward_bf16x3_gpu.py
// holds it to the float64 bound of tests/mlp_f64.py and to <= 2 x the exact kernel's measured error.
//
// Split: TRUNCATION everywhere (hi = the top 16 bits; a - hi is exact in f32 and has <= 16 significant bits; mid = its top 16
// bits; the rest has <= 8 significant bits and IS the lo plane): exact for every finite normal a, no plane can round up to
// infinity (3e38 stays finite), a bf16 pair is ONE v_perm_b32 of two f32 registers; Inf / NaN give non-finite planes (Inf - Inf).
// bf16 has f32's exponent range but ends at 2^-133: the low bits of an operand below about 2^-109 have no plane to go to (measured:
// a weight of 1e-38 kept its hi plane only -- the instruction does NOT flush bf16 denormals -- an error of 2^-7 of its product).
// Weights are small and activations are not, so the window is moved to where the operands live: W0 is staged as 2^16 W0 (EVERY
// f32 below 2^112, denormals included, then splits exactly) and relu(x0) enters as 2^-16 relu(x0) (exact from about 2^-94 up;
// smaller activations lose low bits, below 2^-117 everything); the products are unchanged, nothing is scaled back.
//
// Accumulators: TWO sets -- hi.hi alone, the five corrections (mid.mid, hi.lo, lo.hi, hi.mid, mid.hi: small ones first within
// a k-block) together, added once in the epilogue.  The emulation behind this kernel puts ONE set at 1.8 - 2.0 x the exact
// chain's error if the instruction rounds every internal add, against a criterion of 2; two sets at 0.4 - 0.6 x.  In the
// two-pass form below a pass holds 8 column tiles, so the second set costs the 32 registers the first one gave back.
// NW = 12 waves (3 per SIMD, <= 168 registers: no scratch) whatever RPO_TUNE_FWD_STREAM_WAVES says: at 16 waves (128 registers)
// the compiler spills 38 registers; a scheduling barrier per chunk, mlp_stream.h's remedy, made it spill at 12 as well.
//
// LDS: three planes of 256 x 128 bf16 are 192 KB, the CU has 160.  TWO PASSES over the workgroup's tiles, one half of the
// hidden columns each (pass 0: columns 0..127 = the head shares w8 = 0..3; pass 1: 128..255), all three planes of that half
// resident: 3 x 128 rows x 288 bytes = 108 KB + the tables of mlp_stream.h = 120 KB.  (hi + mid of all 256 rows would fit, but
// the lo plane of W0 from L2 is 64 KB per 16-row tile.)  Pass 1 recomputes the first layer (24 of 216 MFMAs) and reads the
// inputs again; the head partial b1 + shares 0..3 of pass 0 waits in out[row] and is picked up by the lane that wrote it, so
// the head is the exact form's chain with other h1 bits.  Row stride 144 bf16 = 288 bytes: 288 / 16 = 2 mod 16, the rule of
// mlp_stream.h's 136 floats -- the ds_read_b128 of lane (li, lg) at plane[16 jt + li][32 kb + 8 lg ..+7] is conflict-free.
//
// Layout (guide: lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15], j = 0..7; C col = l & 15,
// row = 4 (l >> 4) + reg): the first layer is mlp_stream.h's, unchanged (x0 bit-equal): its C tile `it` leaves lane (li, lg)
// with x0[row li][16 it + 4 lg + i], so tiles 2 kb and 2 kb + 1 ARE the B fragment of k-block kb if k-slot (lg, j) means
// e = 32 kb + 16 (j >> 2) + 4 lg + (j & 3); the W0 planes are staged in that permuted k order and the A fragment of lane
// (li, lg) (row 16 jt + li) is one ds_read_b128 per plane.  The epilogue is mlp_stream.h's.
#pragma once
#include "mlp_stream.h"

namespace rpo_mlp_dev {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#ifndef RPO_BF3_SKIP
#define RPO_BF3_SKIP 0             // timing-only builds (HIPCC_EXTRA=-DRPO_BF3_SKIP=N, wrong results): 1 no first-layer MFMAs, 2 no split
#endif                             // (planes = the packed top halves), 4 the plane reads hoisted out of the tile's loops, 8 pass 0 only

constexpr int kBf3LdW = 144;           // bf16 between rows of a W0 plane in LDS
constexpr int kBf3Half = 128;          // hidden columns per pass
constexpr float kBf3ScaleW = 65536.0f, kBf3ScaleX = 1.0f / 65536.0f;   // see the header: 2^16 W0, 2^-16 relu(x0)

struct Bf16x3Lds {
    __attribute__((aligned(16))) unsigned short w[3][kBf3Half * kBf3LdW];   // [plane][j - 128 pass][permuted k]
    __attribute__((aligned(16))) float fl[128 * 16];            // as StreamLds
    __attribute__((aligned(16))) float bias[128];
    __attribute__((aligned(16))) float b0[256], w1a[256], w1b[256];
};

// (a, b) -> one dword of each plane: a in the low half (even k slot), b in the high half
__device__ __forceinline__ void bf3_split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned ab = __float_as_uint(a), bb = __float_as_uint(b);
    h = __builtin_amdgcn_perm(bb, ab, 0x07060302u);             // (a >> 16) | (b & 0xffff0000): truncation
    if (RPO_BF3_SKIP & 2) { m = h; l = h; return; }
    const float ra = a - __uint_as_float(ab & 0xffff0000u), rb = b - __uint_as_float(bb & 0xffff0000u);
    const unsigned rab = __float_as_uint(ra), rbb = __float_as_uint(rb);
    m = __builtin_amdgcn_perm(rbb, rab, 0x07060302u);
    const float sa = ra - __uint_as_float(rab & 0xffff0000u), sb = rb - __uint_as_float(rbb & 0xffff0000u);
    l = __builtin_amdgcn_perm(__float_as_uint(sb), __float_as_uint(sa), 0x07060302u);
}

__device__ __forceinline__ f32x4 bf3_mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// One 16-row tile of one pass by one wave.  PASS 0: stores x0, starts the head at b1 and leaves the partial in out; PASS 1: no
// x0 store, starts at that partial, finishes (out_mode).  FULL / SAVE / TWO as stream_tile.
template <int PASS, bool FULL, int SAVE, int TWO, class ARGS>
__device__ __forceinline__ void bf3_tile(const ARGS& p, const Bf16x3Lds& lds, int row0, int lane, float b1a, float b1b,
                                         const float (&in3)[3]) {
    constexpr int EIN = 128, H = 256, JT = kBf3Half / 16, CH = 2;
    const Mlp& net = p.net;
    const int li = lane & 15, lg = lane >> 4;
    const bool two = TWO < 0 ? net.n_out > 1 : TWO != 0;
    const bool save_x0 = PASS == 0 && (SAVE < 0 ? p.x0_save != nullptr : SAVE != 0);
    const bool save_h1 = SAVE < 0 ? p.h1_save != nullptr : SAVE != 0;
    const int row = row0 + li;
    const bool live = FULL || row < p.n;
    float v0 = b1a, v1 = b1b;
    if (PASS == 1 && lg == 0 && live) {                          // pass 0's partial, written by this lane (requested early)
        v0 = p.out[(size_t)row * net.n_out];
        if (two) v1 = p.out[(size_t)row * net.n_out + 1];
    }
    f32x4 acch[JT], accc[JT];
#pragma unroll
    for (int c = 0; c < JT; ++c) acch[c] = accc[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float* x0p = (save_x0 && live) ? p.x0_save + (size_t)row * EIN + lg * 4 : nullptr;
#pragma unroll 1
    for (int kb = 0; kb < EIN / 32; ++kb) {
        // ---- first layer, transposed, as stream_tile: tiles it = 2 kb, 2 kb + 1
        u32x4 bh, bm, bl;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int it = 2 * kb + t;
            f32x4 x0 = *reinterpret_cast<const f32x4*>(&lds.bias[it * 16 + lg * 4]);
            const float4 w3 = *reinterpret_cast<const float4*>(&lds.fl[((it * 16 + li) * 4 + lg) * 4]);
            if (!(RPO_BF3_SKIP & 1)) {
                x0 = mfma4(w3.x, in3[0], x0);
                x0 = mfma4(w3.y, in3[1], x0);
                x0 = mfma4(w3.z, in3[2], x0);
            }
            if (PASS == 0 && ((FULL && SAVE > 0) || x0p)) RPO_STREAM_STORE(x0, reinterpret_cast<f32x4*>(x0p + it * 16));
            unsigned h, m, l;
            bf3_split2(kBf3ScaleX * rpo_relu_bits(x0[0]), kBf3ScaleX * rpo_relu_bits(x0[1]), h, m, l);
            bh[2 * t] = h; bm[2 * t] = m; bl[2 * t] = l;
            bf3_split2(kBf3ScaleX * rpo_relu_bits(x0[2]), kBf3ScaleX * rpo_relu_bits(x0[3]), h, m, l);
            bh[2 * t + 1] = h; bm[2 * t + 1] = m; bl[2 * t + 1] = l;
        }
        // ---- hidden layer, transposed: CH column tiles at a time, consecutive MFMAs on different accumulators
        const unsigned short* wb = &lds.w[0][li * kBf3LdW + kb * 32 + lg * 8];
#pragma unroll
        for (int cc = 0; cc < JT; cc += CH) {
            u32x4 ah[CH], am[CH], al[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const unsigned short* wq = (RPO_BF3_SKIP & 4) ? &lds.w[0][li * kBf3LdW + lg * 8 + 16 * q * kBf3LdW] : wb + 16 * (cc + q) * kBf3LdW;
                ah[q] = *reinterpret_cast<const u32x4*>(wq);
                am[q] = *reinterpret_cast<const u32x4*>(wq + kBf3Half * kBf3LdW);
                al[q] = *reinterpret_cast<const u32x4*>(wq + 2 * kBf3Half * kBf3LdW);
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) accc[cc + q] = bf3_mfma(am[q], bm, accc[cc + q]);
#pragma unroll
            for (int q = 0; q < CH; ++q) acch[cc + q] = bf3_mfma(ah[q], bh, acch[cc + q]);
#pragma unroll
            for (int q = 0; q < CH; ++q) accc[cc + q] = bf3_mfma(ah[q], bl, accc[cc + q]);
#pragma unroll
            for (int q = 0; q < CH; ++q) accc[cc + q] = bf3_mfma(al[q], bh, accc[cc + q]);
#pragma unroll
            for (int q = 0; q < CH; ++q) accc[cc + q] = bf3_mfma(ah[q], bm, accc[cc + q]);
#pragma unroll
            for (int q = 0; q < CH; ++q) accc[cc + q] = bf3_mfma(am[q], bh, accc[cc + q]);
        }
    }
    // ---- epilogue (stream_tile's, on this pass's column tiles): acch + accc = h1[row li][128 PASS + 16 jt + 4 lg + i] before the bias
    typedef const f32x4 __attribute__((address_space(3))) * lds_f4;
    typedef const float __attribute__((address_space(3))) * lds_f;
    unsigned ep = (unsigned)(__UINTPTR_TYPE__)((lds_f)(&lds.b0[0])) + lg * 16 + 4 * kBf3Half * PASS;
    asm volatile("" : "+v"(ep));
    float* h1p = (save_h1 && live) ? p.h1_save + (size_t)row * H + kBf3Half * PASS + lg * 4 : nullptr;
#pragma unroll
    for (int w8 = 0; w8 < JT / 2; ++w8) {
        float q0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int jt = 2 * w8; jt < 2 * w8 + 2; ++jt) {
            const f32x4 b0 = *(lds_f4)(__UINTPTR_TYPE__)(ep + 64 * jt);
            const f32x4 wa = *(lds_f4)(__UINTPTR_TYPE__)(ep + 64 * jt + 4 * H);
            const f32x4 h = (acch[jt] + accc[jt]) + b0;
            if ((FULL && SAVE > 0) || h1p) RPO_STREAM_STORE(h, reinterpret_cast<f32x4*>(h1p + 16 * jt));
#pragma unroll
            for (int i = 0; i < 4; ++i) q0[i] = fmaf(rpo_relu_bits(h[i]), wa[i], q0[i]);
            if (two) {
                const f32x4 wb2 = *(lds_f4)(__UINTPTR_TYPE__)(ep + 64 * jt + 8 * H);
#pragma unroll
                for (int i = 0; i < 4; ++i) q1[i] = fmaf(rpo_relu_bits(h[i]), wb2[i], q1[i]);
            }
        }
        float s = (q0[0] + q0[1]) + (q0[2] + q0[3]);
        s = s + stream_xlane(s, lane ^ 16);
        s = s + stream_xlane(s, lane ^ 32);
        v0 += s;
        if (two) {
            float t = (q1[0] + q1[1]) + (q1[2] + q1[3]);
            t = t + stream_xlane(t, lane ^ 16);
            t = t + stream_xlane(t, lane ^ 32);
            v1 += t;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (lg == 0 && live) {
        float o0 = v0;
        if (PASS == 1 && p.out_mode == 1) o0 = p.scale * tanhf(o0) + p.base;
        p.out[(size_t)row * net.n_out] = o0;
        if (two) p.out[(size_t)row * net.n_out + 1] = v1;
    }
}

// The first-layer and head tables (once per workgroup) and the three planes of one half of W0 (once per pass); the caller
// synchronises.  One item = 8 consecutive k slots of a row = the two float4 at e = 32 kb + 4 lg and + 16.
template <int NW>
__device__ __forceinline__ void bf3_stage_tables(const Mlp& net, Bf16x3Lds& lds, int tid) {
    const int nin = net.S + net.A;
    for (int idx = tid; idx < 128 * 16; idx += NW * 64) {
        const int e = idx >> 4, g = (idx >> 2) & 3, ks = idx & 3, u = 4 * ks + g;
        float v = 0.0f;
        if (ks < 3) {
            if (u < net.S) v = net.Ws[e * net.S + u];
            else if (u < nin) v = net.Wa[e * net.A + (u - net.S)];
        }
        lds.fl[idx] = v;
    }
    for (int idx = tid; idx < 128; idx += NW * 64) lds.bias[idx] = net.A > 0 ? net.bs[idx] + net.ba[idx] : net.bs[idx];
    for (int idx = tid; idx < 256; idx += NW * 64) {
        lds.b0[idx] = net.b0[idx];
        lds.w1a[idx] = net.W1[idx];
        lds.w1b[idx] = net.n_out > 1 ? net.W1b[idx] : 0.0f;
    }
}

template <int NW>
__device__ __forceinline__ void bf3_stage_planes(const Mlp& net, Bf16x3Lds& lds, int pass, int tid) {
    for (int idx = tid; idx < kBf3Half * 16; idx += NW * 64) {
        const int jh = idx >> 4, kb = (idx >> 2) & 3, g = idx & 3;
        const float* src = net.W0 + (size_t)(kBf3Half * pass + jh) * 128 + 32 * kb + 4 * g;
        float4 x = *reinterpret_cast<const float4*>(src), y = *reinterpret_cast<const float4*>(src + 16);
        x.x *= kBf3ScaleW; x.y *= kBf3ScaleW; x.z *= kBf3ScaleW; x.w *= kBf3ScaleW;
        y.x *= kBf3ScaleW; y.y *= kBf3ScaleW; y.z *= kBf3ScaleW; y.w *= kBf3ScaleW;
        u32x4 h, m, l;
        unsigned a, b, c;
        bf3_split2(x.x, x.y, a, b, c); h[0] = a; m[0] = b; l[0] = c;
        bf3_split2(x.z, x.w, a, b, c); h[1] = a; m[1] = b; l[1] = c;
        bf3_split2(y.x, y.y, a, b, c); h[2] = a; m[2] = b; l[2] = c;
        bf3_split2(y.z, y.w, a, b, c); h[3] = a; m[3] = b; l[3] = c;
        const int o = jh * kBf3LdW + 32 * kb + 8 * g;
        *reinterpret_cast<u32x4*>(&lds.w[0][o]) = h;
        *reinterpret_cast<u32x4*>(&lds.w[1][o]) = m;
        *reinterpret_cast<u32x4*>(&lds.w[2][o]) = l;
    }
}

template <int PASS, int NW, class ARGS>
__device__ __forceinline__ void bf3_pass(const ARGS& p, const Bf16x3Lds& lds, int lane, int wave, float b1a, float b1b) {
    const Mlp& net = p.net;
    const int tiles = (p.n + kRows - 1) / kRows;
    const int t0 = blockIdx.x * NW + wave, dt = gridDim.x * NW;
    float in3[3] = {0.0f, 0.0f, 0.0f};
    if (t0 < tiles) stream_inputs(p, (long long)t0 * kRows, lane, in3);
    for (int t = t0; t < tiles; t += dt) {
        const int row0 = t * kRows;
        float nxt[3];
        stream_inputs(p, (long long)(t + dt < tiles ? t + dt : t) * kRows, lane, nxt);   // the next tile's inputs, one tile ahead
        const bool save = p.x0_save && p.h1_save, none = !p.x0_save && !p.h1_save, two = net.n_out > 1;
        if (row0 + kRows <= p.n && (save || none)) {
            if (save && !two) bf3_tile<PASS, true, 1, 0>(p, lds, row0, lane, b1a, b1b, in3);
            else if (none && !two) bf3_tile<PASS, true, 0, 0>(p, lds, row0, lane, b1a, b1b, in3);
            else if (save && two) bf3_tile<PASS, true, 1, 1>(p, lds, row0, lane, b1a, b1b, in3);
            else bf3_tile<PASS, true, 0, 1>(p, lds, row0, lane, b1a, b1b, in3);
        } else {
            bf3_tile<PASS, false, -1, -1>(p, lds, row0, lane, b1a, b1b, in3);   // ragged last tile / one of x0, h1 saved
        }
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) in3[ks] = nxt[ks];
    }
}

template <int NW, class ARGS4>
__device__ __forceinline__ void mlp_forward_stream_bf16x3_body(const ARGS4& p4) {
    __shared__ Bf16x3Lds lds;
    const auto& p = p4.net[blockIdx.y];
    const Mlp& net = p.net;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float b1a = net.b1[0], b1b = net.n_out > 1 ? net.b1b[0] : 0.0f;
    bf3_stage_tables<NW>(net, lds, tid);
    bf3_stage_planes<NW>(net, lds, 0, tid);
    __syncthreads();
    bf3_pass<0, NW>(p, lds, lane, wave, b1a, b1b);
    if (RPO_BF3_SKIP & 8) return;
    __syncthreads();                                             // every wave is done with the planes of pass 0
    bf3_stage_planes<NW>(net, lds, 1, tid);
    __syncthreads();
    bf3_pass<1, NW>(p, lds, lane, wave, b1a, b1b);
}

}  // namespace rpo_mlp_dev
