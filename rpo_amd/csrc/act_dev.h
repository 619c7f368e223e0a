// Launch arguments and the per-row chain of the policy_act kernels (trainer.act(), rpo_amd/algo/acting.py), shared by the
// row-tile form (act.hip) and the streaming form (act_stream.hip: a translation unit of its own, compiled without SLP
// vectorisation).  The chain -- head -> Complete -> GRG -> residuals -> stores -- is built from the functions of the
// stand-alone launches (gauss_head_row, *_explore_project, eq_ineq / the expressions of pendulum_resid_kernel), so the
// outputs are those launches' bits.
#pragma once
#include <type_traits>

#include "cartsafe_dev.h"
#include "heads_dev.h"
#include "mlp_tile.h"
#include "pendulum_dev.h"
#include "rollout_env.h"

namespace {

using rpo_mlp_dev::Mlp;

template <class ENV>
struct PolicyActArgs {
    Mlp actor;
    float scale, base;            // tanh box of the actor output (BoxConstraint)
    int gauss;                    // 0: deterministic actor (DDPG); 1: the mean head of the squashed Gaussian (SAC)
    int n;
    const float* obs;             // [n, obs_stride] caller-supplied observations
    int obs_stride;
    float* proposal;              // [n] (may be NULL)
    int* iters;                   // [n] (may be NULL)
    float* eq;                    // [n] (may be NULL)
    float* ineq;                  // [n, 6 | 1] (may be NULL)
    typename ENV::ActArgs act;    // projection parameters (RPO_NOISE_NONE), action out
};

// The outputs are written once and read by a later launch (or the host): streaming stores, as the trace rows.
typedef float act_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void act_store(float* dst, float v) { __builtin_nontemporal_store(v, dst); }
__device__ __forceinline__ void act_store(int* dst, int v) { __builtin_nontemporal_store(v, dst); }
__device__ __forceinline__ void act_store2(float* dst, float x, float y) {
    __builtin_nontemporal_store(act_v2{x, y}, reinterpret_cast<act_v2*>(dst));
}

// pendulum_resid_kernel's two expressions (pendulum.hip) with THAT kernel's rounding spelled out.  The kernel leaves contraction
// to the compiler, and what the compiler does there depends on the kernel around the expressions: the SLP vectoriser packs
// a_x a_x and a_y a_y into one v_pk_mul_f32, so the inequality is the unfused (a_x a_x + a_y a_y) - 32, while the equality's
// a_x C_p + a_y C_o becomes fma(a_x, C_p, a_y C_o).  The same source inside these kernels -- inlined or out of line -- fused
// BOTH (read off the ISA), which moved the inequality residual by an ulp.  tests/test_act_gpu.py pins the equality of the bits.
__device__ __forceinline__ float2 act_pend_resid(const float* o, float2 a) {
    RPO_FP_STRICT
    const rpo_pend_dev::Eq e = rpo_pend_dev::set_eq(o[0], o[1], o[2], o[3], o[4]);
    return make_float2(e.b - fmaf(a.x, e.C_p, a.y * e.C_o), (a.x * a.x + a.y * a.y) - rpo_pend_dev::kMaxSum);
}

template <class ENV>
__device__ __forceinline__ void act_store_resid(const PolicyActArgs<ENV>& p, const typename ENV::Consts& c, const float* obs, int i,
                                                float2 a) {
    if (!p.eq && !p.ineq) return;
    if constexpr (std::is_same<ENV, CartEnv>::value) {
        float h, g[6];
        rpo_cart_dev::eq_ineq(c, a.x, a.y, h, g);
        if (p.eq) act_store(p.eq + i, h);
        if (p.ineq) {
            float* o = p.ineq + (size_t)i * 6;
            act_store2(o, g[0], g[1]);
            act_store2(o + 2, g[2], g[3]);
            act_store2(o + 4, g[4], g[5]);
        }
    } else {
        const float2 r = act_pend_resid(obs, a);
        if (p.eq) act_store(p.eq + i, r.x);
        if (p.ineq) act_store(p.ineq + i, r.y);
    }
}

// One row: (o0, o1) = the actor's outputs (after the tanh box for gauss = 0), obs = the row's observation.
template <class ENV>
__device__ __forceinline__ void policy_act_row(const PolicyActArgs<ENV>& p, const typename ENV::Consts& c, const float* obs, int i,
                                               float o0, float o1) {
    float ap = o0;
    if (p.gauss) ap = rpo_head_dev::gauss_head_row(o0, o1, 0.0f, p.scale, p.base, p.act.box_lo, p.act.box_hi, 1, nullptr);
    int k;
    const float2 a = ENV::project(p.act, c, obs, i, ap, 0.0f, 0, k);
    act_store2(p.act.action + (size_t)i * 2, a.x, a.y);
    if (p.proposal) act_store(p.proposal + i, ap);
    if (p.iters) act_store(p.iters + i, k);
    act_store_resid<ENV>(p, c, obs, i, a);
}

}  // namespace

// The streaming form (act_stream.hip).  `args` / `consts`: a PolicyActArgs<CartEnv | PendEnv> and that env's Consts, as untyped
// pointers (the env policies live in anonymous namespaces: one type per translation unit, same layout).  g4: 64-row groups
// (G = 4) instead of 16-row ones.  Returns -1 when the form does not apply (shape, alignment of W0), 0 after a launch,
// > 0 = hipError_t.
__attribute__((visibility("hidden"))) int rpo_act_stream_launch(int env /* 0 CartSafe, 1 SpringPendulum */, const void* args,
                                                                const void* consts, int g4, void* stream);
