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

// ------------------------------------------------------------------------------------------------ projection profiles
// trainer.act(profile=True): plane b of data [K + 1, n, 4] holds, for row i, (a0, a1, eq_resid, max_j ineq_resid_j) of the
// iterate after min(b, k*) GRG steps -- what a call with the budget b returns (k*: the iteration at which the row's stop test
// fires).  Plane-major: the lanes of a wave write neighbouring 16-byte rows of one plane.
struct ActProfile {
    float* data;                  // [K + 1, n, 4], 16-byte aligned
    int K;                        // the budget of the call (max_steps of the projection)
};
struct ActNoProfile {};           // (the PROFILE = 0 instances of policy_act_kernel take no profile argument)

typedef float act_v4 __attribute__((ext_vector_type(4)));

// The GRG state of one row: Complete, the stop test's predicate and one step, in the arithmetic of cart_explore_project /
// pend_explore_project under RPO_NOISE_NONE (contraction off there and here: the same expressions round the same way).
template <class ENV>
struct ActGrgRow;

template <>
struct ActGrgRow<CartEnv> {
    float ap, ao, old_p, old_o;
    __device__ __forceinline__ void init(const rpo_cart_dev::CartConsts& c, const float*, float ap_in) {
        RPO_FP_STRICT
        ap = ap_in;
        ao = (c.b - ap * c.C_p) * c.C_o_inv;                     // complete_partial
        old_p = 0.0f; old_o = 0.0f;
    }
    __device__ __forceinline__ float2 action(const rpo_cart_dev::CartConsts& c) const {
        return c.partial == 0 ? make_float2(ap, ao) : make_float2(ao, ap);
    }
    // (eq_resid, max_j ineq_resid_j) at the iterate: eq_ineq, which is also what rpo_cartsafe_resid stores
    __device__ __forceinline__ float2 resid(const rpo_cart_dev::CartConsts& c, const float*) const {
        const float2 a = action(c);
        float h, g[6];
        rpo_cart_dev::eq_ineq(c, a.x, a.y, h, g);
        float mx = g[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) mx = fmaxf(mx, g[j]);
        return make_float2(h, mx);
    }
    __device__ __forceinline__ bool violated(const rpo_cart_dev::ActArgs& p, const rpo_cart_dev::CartConsts& c) const {
        const float2 a = action(c);
        float h, g[6];
        rpo_cart_dev::eq_ineq(c, a.x, a.y, h, g);
        float mx = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; ++j) mx = fmaxf(mx, g[j]);
        return fabsf(h) > p.corr_eps || mx > p.corr_eps;
    }
    __device__ __forceinline__ void step(const rpo_cart_dev::ActArgs& p, const rpo_cart_dev::CartConsts& c) {
        RPO_FP_STRICT
        const float gp = rpo_cart_dev::reduced_grad(c, ap);
        const float go = -(gp * c.C_p) * c.C_o_inv;
        const float sp = p.corr_lr * gp + p.corr_momentum * old_p;
        const float so = p.corr_lr * go + p.corr_momentum * old_o;
        ap -= sp; ao -= so;
        old_p = sp; old_o = so;
    }
};

template <>
struct ActGrgRow<PendEnv> {
    rpo_pend_dev::Eq e;
    float ax, ay, old_x, old_y;
    __device__ __forceinline__ void init(const PendEnv::Consts&, const float* o, float ap_in) {
        RPO_FP_STRICT
        e = rpo_pend_dev::set_eq(o[0], o[1], o[2], o[3], o[4]);
        ax = ap_in;
        ay = (e.b - ax * e.C_p) * e.C_o_inv;                     // complete_partial
        old_x = 0.0f; old_y = 0.0f;
    }
    __device__ __forceinline__ float2 action(const PendEnv::Consts&) const { return make_float2(ax, ay); }
    // rpo_pendulum_resid's bits (act_pend_resid: its equality is fused), NOT the stop test's unfused equality below
    __device__ __forceinline__ float2 resid(const PendEnv::Consts&, const float* o) const {
        return act_pend_resid(o, make_float2(ax, ay));
    }
    __device__ __forceinline__ bool violated(const rpo_pend_dev::ActArgs& p, const PendEnv::Consts&) const {
        RPO_FP_STRICT
        const float h = e.b - (ax * e.C_p + ay * e.C_o);
        const float g = ax * ax + ay * ay - rpo_pend_dev::kMaxSum;
        return fabsf(h) > p.corr_eps || g > p.corr_eps;
    }
    __device__ __forceinline__ void step(const rpo_pend_dev::ActArgs& p, const PendEnv::Consts&) {
        RPO_FP_STRICT
        float gx, gy;
        rpo_pend_dev::ipg_row(e, ax, ay, gx, gy);
        const float sx = p.corr_lr * gx + p.corr_momentum * old_x;
        const float sy = p.corr_lr * gy + p.corr_momentum * old_y;
        ax -= sx; ay -= sy;
        old_x = sx; old_y = sy;
    }
};

// ENV::project under RPO_NOISE_NONE with the budget q.K, writing the row's plane entries as it goes: at every k in 0..K the
// current iterate leaves as ONE non-temporal 16-byte store, then the row steps if it is still live (the first iteration is
// unconditional, as in the *_explore_project loops).  The loop runs to K for the whole wave: a row whose stop test has fired
// keeps storing its final iterate, so every plane is complete and none needs zeroing.  Returns the action and the iteration
// count of the budget K.  Shared by the stand-alone launch (act.hip: project_profile_kernel) and policy_act_kernel<PROFILE = 1>.
template <class ENV>
__device__ __forceinline__ float2 act_project_profile(const typename ENV::ActArgs& p, const typename ENV::Consts& c, const float* obs,
                                                      int i, int n, float ap, const ActProfile& q, int& iters) {
    ActGrgRow<ENV> r;
    r.init(c, obs, ap);
    act_v4* dst = reinterpret_cast<act_v4*>(q.data) + i;
    bool live = true;
    int its = 0;
    for (int k = 0;; ++k) {
        const float2 a = r.action(c), hg = r.resid(c, obs);
        __builtin_nontemporal_store(act_v4{a.x, a.y, hg.x, hg.y}, dst);
        if (k == q.K) break;
        dst += n;
        if (live && k > 0 && !r.violated(p, c)) live = false;
        if (live) { r.step(p, c); ++its; }
    }
    iters = its;
    return r.action(c);
}

// policy_act_row with the profile: the same head, the same stores, the projection above.
template <class ENV>
__device__ __forceinline__ void policy_act_row_profile(const PolicyActArgs<ENV>& p, const typename ENV::Consts& c, const float* obs,
                                                       int i, float o0, float o1, const ActProfile& q) {
    float ap = o0;
    if (p.gauss) ap = rpo_head_dev::gauss_head_row(o0, o1, 0.0f, p.scale, p.base, p.act.box_lo, p.act.box_hi, 1, nullptr);
    int k;
    const float2 a = act_project_profile<ENV>(p.act, c, obs, i, p.n, ap, q, k);
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
