// Policy evaluation on the device (trainer.evaluate(), rpo_amd/algo/evaluation.py): many independent episodes with the
// deterministic policy and the evaluation-time projection, no exploration, no replay scatter, no auto-reset.
//
//   eval_kernel          obs tile -> actor MLP (f32 MFMA) -> [mean head] -> Complete -> GRG -> env step -> per-episode
//                        accumulators, looped over up to `steps` env steps inside the workgroup (its own 16 * RT lanes:
//                        no grid-wide synchronisation, no co-residency assumption).  The pieces are those of
//                        rollout_kernel (fused.hip), so the bits are those of the stepwise path.
//   eval_accumulate      the stepwise path's update: reads the transition rows rpo_<env>_step wrote.
//   eval_record          the stepwise path's per-step record (rpo_eval_record); the fused kernel's REC = 1 instances write the
//                        same rows themselves (eval_dev.h: trace_store_head / trace_store_tail).
//   eval_obs_noise       the stepwise path's observation noise (rpo_eval_obs_noise); the fused kernel's NOISE = 1 instances
//                        add the same values to their staged tile (eval_dev.h: rpo_eval_noisy_obs).
//   eval_constraints     the stepwise path's per-constraint report (rpo_eval_constraints); the fused kernel's CON = 1 instances
//                        update the same rows themselves (eval_dev.h: rpo_eval_con_lane_update).
//   (no kernel)          evaluate_budgets(): the fused kernel's BUD = 1 instances (rpo_<env>_evaluate_budgets) read the projection's
//                        budget and step size per lane, so B budgets x episodes run side by side in one launch.
//   (no kernel)          evaluate_policies(): the fused kernel's POL = 1 instances (rpo_<env>_evaluate_policies) run every group of
//                        group_lanes lanes on an actor of its own out of a bank, so P policies x episodes run in one launch.
//   (no kernel)          evaluate_noise(): the fused kernel's NSW = 1 instances (rpo_<env>_evaluate_noise_sweep) run every group of
//                        group_lanes lanes under a sigma of its own out of a table and key the draw by the episode within the
//                        group, so S noise levels x episodes run in one launch on the same z.
//   summarize_*_kernel   the accumulator rows of a finished evaluation -> one row of an evaluation curve (rpo_eval_summarize).
//   keep_best_*_kernel   that row against the incumbent's on the device, and the predicated copy of the actor's parameters
//                        (rpo_eval_keep_best; the criterion is eval_dev.h: keep_best_wins).
//
// Both update a lane's accumulator row through rpo_eval_lane_update (eval_dev.h).
#include "cartsafe_dev.h"
#include "eval_dev.h"
#include "heads_dev.h"
#include "host_glue.h"
#include "mlp_tile.h"
#include "pendulum_dev.h"
#include "rollout_env.h"

namespace {

using namespace rpo_mlp_dev;
using rpo_host::check_actor;
using rpo_host::check_eval_con;
using rpo_host::check_eval_range;
using rpo_host::to_dev;
using rpo_eval_dev::con_width;
using rpo_eval_dev::nanmax;
using rpo_eval_dev::row_violations;
using rpo_eval_dev::rpo_eval_lane_update;
using rpo_eval_dev::trace_head;
using rpo_eval_dev::trace_width;

template <class ENV>
struct EvalArgs {
    Mlp actor;
    float scale, base;            // tanh box of the actor output (BoxConstraint)
    int gauss;                    // 0: deterministic actor (DDPG); 1: the mean head of the squashed Gaussian (SAC)
    int t0, steps;                // env steps [t0, t0 + steps) of the evaluation; t0 == 0 initialises the accumulators
    float* acc;                   // [n, RPO_EVAL_LEN]
    float* trace;                 // REC instances: [., trace_rows, W] per-step record (RPO_TRACE_*), lanes i < trace_rows
    int trace_rows;
    typename ENV::ActArgs act;    // projection parameters (RPO_NOISE_NONE), action out
    typename ENV::StepArgs step;  // env state and bookkeeping (rows = NULL, auto_reset = 0)
};

// The CON = 1 instances take the report behind the same arguments; the CON = 0 instances keep EvalArgs as their parameter.
template <class ENV>
struct EvalConArgs : EvalArgs<ENV> {
    float* con;                   // [n, con_width(kIneq, kEq)] per-constraint report (RPO_CON_*)
};
// The NOISE = 1 instances (evaluate(obs_noise=)) take sigma by value and the key of the draw behind the same arguments (con:
// NULL for their CON = 0 instances, which never read it); the NOISE = 0 instances keep their parameter types.
template <class ENV>
struct EvalNoiseArgs : EvalConArgs<ENV> {
    float sigma[8];               // per observation column, zeros beyond kObs; 0: the column is not drawn
    unsigned long long noise_seed;
};
// The BUD = 1 instances (evaluate_budgets()) take the lanes' budgets behind the EvalConArgs arguments (con: NULL for their
// CON = 0 instances, which never read it); the BUD = 0 instances keep their parameter types.
template <class ENV>
struct EvalBudArgs : EvalConArgs<ENV> {
    const int* lane_steps;        // [n] GRG iterations at most, in place of act.max_steps
    const float* lane_lr;         // [n] step size, in place of act.corr_lr
};
// The POL = 1 instances (evaluate_policies()) take the groups' geometry behind the EvalConArgs arguments (con: NULL for their
// CON = 0 instances, which never read it); `actor` describes policy 0 of the bank; the POL = 0 instances keep their parameter
// types.
template <class ENV>
struct EvalPolArgs : EvalConArgs<ENV> {
    int policy_stride;            // floats from one policy of the bank to the next: > 0, a multiple of 4
    int group_lanes;              // lanes per policy, padding included: a multiple of 64; n = P * group_lanes
    int episodes;                 // live lanes per group: 1 <= episodes <= group_lanes
};
// The NSW = 1 instances (evaluate_noise()) take the groups' sigma table, the key of the draw and the groups' geometry behind the
// EvalConArgs arguments (con: NULL for their CON = 0 instances, which never read it); the NSW = 0 instances keep their parameter
// types.
template <class ENV>
struct EvalNoiseSweepArgs : EvalConArgs<ENV> {
    const float* sigma_table;     // [S, 8] on the device: group g's sigma per observation column, zeros beyond kObs
    unsigned long long noise_seed;
    int group_lanes;              // lanes per noise level, padding included: a multiple of 64; n = S * group_lanes
    int episodes;                 // live lanes per group: 1 <= episodes <= group_lanes
};
template <class ENV, int CON, int NOISE, int BUD = 0, int POL = 0, int NSW = 0> struct EvalArgsOf { typedef EvalArgs<ENV> type; };
template <class ENV> struct EvalArgsOf<ENV, 1, 0, 0, 0> { typedef EvalConArgs<ENV> type; };
template <class ENV, int CON> struct EvalArgsOf<ENV, CON, 1, 0, 0> { typedef EvalNoiseArgs<ENV> type; };
template <class ENV, int CON> struct EvalArgsOf<ENV, CON, 0, 1, 0> { typedef EvalBudArgs<ENV> type; };
template <class ENV, int CON> struct EvalArgsOf<ENV, CON, 0, 0, 1> { typedef EvalPolArgs<ENV> type; };
template <class ENV, int CON> struct EvalArgsOf<ENV, CON, 1, 0, 0, 1> { typedef EvalNoiseSweepArgs<ENV> type; };

// What one env step leaves for the statistics: reward, done and the violations of the transition row, without the row --
// their maxima for the accumulators, and the row's ineq_viol / eq_viol columns themselves (gi / he) for the report.
// Observations are staged from the env's observation rows: for SpringPendulum those the stepwise path hands the actor
// and the projection (after an injected initial state they come from torch's cos / sin, not from sincosf).  `stage` writes
// element (r, q) of the tile with thread r * kObs + q (stage_noise below relies on it).
template <class ENV>
struct EvalEnv;

template <>
struct EvalEnv<CartEnv> {
    static constexpr int kObs = 6, kIneq = 6, kEq = 1;
    __device__ static __forceinline__ void stage(const rpo_cart_dev::StepArgs& p, int row0, int rows, float* in_s, int stride) {
        CartEnv::stage_obs(p, row0, rows, in_s, stride);
    }
    // the state `lane` steps: the staged row IS the state -- unless it carries noise, then the env's own row (the same bits
    // without noise: the row was staged from it)
    template <int NOISE>
    __device__ static __forceinline__ const float* true_state(const rpo_cart_dev::StepArgs& p, int i, const float* staged) {
        return NOISE ? p.state + (size_t)i * 6 : staged;
    }
    __device__ static __forceinline__ void lane(const rpo_cart_dev::StepArgs& p, const rpo_cart_dev::CartConsts& c, int i,
                                                const float* obs, float2 a, float& reward, float& done, float& ineq, float& eq,
                                                float (&gi)[kIneq], float (&he)[kEq]) {
        float s[6], ns[6], st[rpo_cart_dev::kStepStats];
        float4 row[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] = obs[q];
        rpo_cart_dev::cart_lane(p, c, i, s, a, rpo_load_episode(p.ep_len, p.ep_ret, p.ep_count, i), ns, row, st);
        rpo_cart_dev::store_state(p.state + (size_t)i * 6, ns);
        reward = row[3].z;
        done = row[3].w;
        eq = fabsf(row[4].x);
        // the ineq_viol columns in order, max with NaN propagation (Tensor.max(dim=1))
        ineq = nanmax(nanmax(nanmax(nanmax(nanmax(row[4].y, row[4].z), row[4].w), row[5].x), row[5].y), row[5].z);
        he[0] = row[4].x;
        gi[0] = row[4].y; gi[1] = row[4].z; gi[2] = row[4].w; gi[3] = row[5].x; gi[4] = row[5].y; gi[5] = row[5].z;
    }
};

template <>
struct EvalEnv<PendEnv> {
    static constexpr int kObs = 5, kIneq = 1, kEq = 1;
    __device__ static __forceinline__ void stage(const rpo_pend_dev::StepArgs& p, int row0, int rows, float* in_s, int stride) {
        const int tid = threadIdx.x;
        if (tid < rows * 5) {
            const int r = tid / 5, q = tid - r * 5;
            in_s[r * stride + q] = (row0 + r < p.n) ? p.obs[(size_t)(row0 + r) * 5 + q] : 0.0f;
        }
    }
    template <int NOISE>                                         // (`lane` reads p.internal whatever was staged)
    __device__ static __forceinline__ const float* true_state(const rpo_pend_dev::StepArgs&, int, const float* staged) {
        return staged;
    }
    __device__ static __forceinline__ void lane(const rpo_pend_dev::StepArgs& p, const PendEnv::Consts&, int i, const float*,
                                                float2 a, float& reward, float& done, float& ineq, float& eq,
                                                float (&gi)[kIneq], float (&he)[kEq]) {
        const float4 s = reinterpret_cast<const float4*>(p.internal)[i];
        float ns[4], ncs, nsn, st[rpo_pend_dev::kStepStats];
        float4 row[4];
        rpo_pend_dev::pend_lane(p, i, s, a, rpo_load_episode(p.ep_len, p.ep_ret, p.ep_count, i), ns, ncs, nsn, row, st);
        reinterpret_cast<float4*>(p.internal)[i] = make_float4(ns[0], ns[1], ns[2], ns[3]);
        rpo_pend_dev::store_obs(p.obs + (size_t)i * 5, ncs, nsn, ns[1], ns[2], ns[3]);
        reward = row[3].x;
        done = row[3].y;
        eq = fabsf(row[3].z);
        ineq = row[3].w;
        he[0] = row[3].z;
        gi[0] = row[3].w;
    }
};

// REC = 1: a live lane i < p.trace_rows also writes row (s, i) of the trace -- the head before ENV::lane runs (the pendulum lane
// overwrites its observation row), the tail after it.  Nothing of the record is computed in, or alive across, the MFMA loops.
// CON = 1: a live lane also folds the step's per-constraint values into row i of p.con, read and written in global memory
// inside the step (rpo_eval_con_lane_update) -- likewise nothing of it crosses the MFMA loops.
// NOISE = 1: the thread that staged element (r, q) of the tile adds sigma[q] * z(row0 + r, s, q) to it in LDS
// (rpo_eval_noisy_obs) before the forward's barrier -- the actor, the projection and the record's head read the noisy tile, the
// env steps its own state (EvalEnv::true_state).  The draw ends in that LDS word: nothing of it is alive in the MFMA loops.
template <class ENV, class ARGS>
__device__ __forceinline__ void stage_noise(const ARGS& p, int row0, int rows, int n, int s, float* in_s, int stride) {
    constexpr int kObs = EvalEnv<ENV>::kObs;
    const int tid = threadIdx.x;
    if (tid >= rows * kObs) return;
    const int r = tid / kObs, q = tid - r * kObs;
    if (row0 + r >= n) return;
    float sigma = 0.0f;
#pragma unroll
    for (int u = 0; u < kObs; ++u)                               // (selects on constant indices: the by-value array stays in SGPRs)
        if (q == u) sigma = p.sigma[u];
    float* o = in_s + r * stride + q;
    *o = rpo_eval_dev::rpo_eval_noisy_obs(*o, sigma, p.noise_seed, row0 + r, s, q);
}

// NSW = 1: the workgroup's lanes belong to ONE group g (a scalar, as under POL = 1).  The thread that staged element (r, q) reads
// the group's sigma out of the table (sigma_table[8 g + q]) and keys the draw by the EPISODE within the group,
// e = row0 + r - g * group_lanes, not by the lane: level g on episode e draws the z(e, s, q) every other level draws, and the
// one evaluate(obs_noise=) draws for its lane e.  A padding lane (e >= episodes) is not drawn for.  As in stage_noise the draw
// ends in the LDS word.
template <class ENV, class ARGS>
__device__ __forceinline__ void stage_noise_group(const ARGS& p, int row0, int rows, int g, int s, float* in_s, int stride) {
    constexpr int kObs = EvalEnv<ENV>::kObs;
    const int tid = threadIdx.x;
    if (tid >= rows * kObs) return;
    const int r = tid / kObs, q = tid - r * kObs;
    const int e = row0 + r - g * p.group_lanes;
    if (e >= p.episodes) return;
    const float sigma = p.sigma_table[(size_t)g * 8 + q];
    float* o = in_s + r * stride + q;
    *o = rpo_eval_dev::rpo_eval_noisy_obs(*o, sigma, p.noise_seed, e, s, q);
}

// BUD = 1: a live lane reads its own budget and step size (p.lane_steps[i], p.lane_lr[i]) behind the forward and projects with
// them in place of p.act.max_steps / p.act.corr_lr: two more VGPRs and a vector loop bound in a loop that rows of one wave
// already leave at different iterations; everything else of p.act stays launch-uniform, nothing of it crosses the MFMA loops.
template <class ENV, int BUD, class ARGS>
__device__ __forceinline__ float2 eval_project(const ARGS& p, const typename ENV::Consts& c, const float* obs, int i, float ap,
                                               int& k) {
    if constexpr (BUD) return ENV::project_budget(p.act, c, obs, i, ap, p.lane_steps[i], p.lane_lr[i], k);
    else return ENV::project(p.act, c, obs, i, ap, 0.0f, 0, k);
}

// POL = 1: the workgroup's 16 * RT lanes belong to ONE group g = row0 / group_lanes (group_lanes is a multiple of 64), a
// function of blockIdx alone that is pinned to a scalar register; the workgroup runs the loop on a copy of the descriptor
// whose non-NULL pointers are advanced by g * policy_stride floats -- scalar adds in front of the loop, nothing per policy
// in a vector register.  A lane is `mine` only inside its group's first `episodes` lanes: padding lanes are never live, so
// they never step, never write a row and never keep the workgroup alive (an all-padding workgroup leaves at the first
// __syncthreads_or); their env rows are staged like any lane's and their outputs dropped.
__device__ __forceinline__ const float* policy_ptr(const float* p, size_t off) { return p ? p + off : p; }
__device__ __forceinline__ Mlp policy_of_group(const Mlp& a, int g, int policy_stride) {
    const size_t off = (size_t)g * (size_t)policy_stride;
    Mlp m = a;
    m.Ws = policy_ptr(a.Ws, off); m.bs = policy_ptr(a.bs, off); m.Wa = policy_ptr(a.Wa, off); m.ba = policy_ptr(a.ba, off);
    m.W0 = policy_ptr(a.W0, off); m.b0 = policy_ptr(a.b0, off); m.W1 = policy_ptr(a.W1, off); m.b1 = policy_ptr(a.b1, off);
    m.W1b = policy_ptr(a.W1b, off); m.b1b = policy_ptr(a.b1b, off);
    return m;
}

template <class ENV, int EIN, int H, int RT, int REC, int CON, int NOISE, int BUD = 0, int POL = 0, int NSW = 0>
__global__ __launch_bounds__(kFwdThreads) void eval_kernel(typename EvalArgsOf<ENV, CON, NOISE, BUD, POL, NSW>::type p, typename ENV::Consts c) {
    static_assert(!BUD || (!REC && !NOISE), "per-lane budgets: no record, no observation noise");
    static_assert(!POL || (!REC && !NOISE && !BUD), "an actor per group: no record, no observation noise, one budget");
    static_assert(!NSW || (NOISE && !REC && !BUD && !POL), "a sigma per group: the noisy instance, no record, one budget, one actor");
    typedef TileLds<EIN, RT, 8, 8> Lds;                          // 16 * RT lanes per workgroup; OBS <= 8
    __shared__ Lds lds;
    constexpr int kInS = Lds::kS;
    constexpr int kLanes = rpo_mlp_dev::kRows * RT;
    const int row0 = blockIdx.x * kLanes;
    const int tid = threadIdx.x;
    const int n = p.step.n;
    const int i = row0 + tid;
    bool mine = tid < kLanes && i < n;
    Mlp group_actor;
    if constexpr (POL) {
        const int g = __builtin_amdgcn_readfirstlane(row0 / p.group_lanes);
        mine = mine && i - g * p.group_lanes < p.episodes;
        group_actor = policy_of_group(p.actor, g, p.policy_stride);
    }
    int noise_group = 0;                                         // NSW = 1: the workgroup's group, a scalar like POL's g
    if constexpr (NSW) {
        noise_group = __builtin_amdgcn_readfirstlane(row0 / p.group_lanes);
        mine = mine && i - noise_group * p.group_lanes < p.episodes;
    }
    const Mlp& actor = POL ? group_actor : p.actor;
    for (int s = p.t0; s < p.t0 + p.steps; ++s) {
        // a lane's state is read from its accumulator row at every step (nothing of it stays live across the MFMA loops)
        const bool live = mine && (s == 0 || (__float_as_int(p.acc[(size_t)i * RPO_EVAL_LEN + 7]) & RPO_EVAL_ALIVE));
        if (!__syncthreads_or(live)) return;                     // (also the barrier in front of the LDS tiles' reuse)
        EvalEnv<ENV>::stage(p.step, row0, kLanes, lds.in_s, kInS);
        if constexpr (NSW) stage_noise_group<ENV>(p, row0, kLanes, noise_group, s, lds.in_s, kInS);
        else if constexpr (NOISE) stage_noise<ENV>(p, row0, kLanes, n, s, lds.in_s, kInS);
        mlp_tile_forward<EIN, H, RT, Lds>(actor, lds, row0, n, nullptr, nullptr, p.gauss ? 0 : 1, p.scale, p.base);
        if (live) {
            float ap = lds.out[tid * 2];
            if (p.gauss) ap = rpo_head_dev::gauss_head_row(ap, lds.out[tid * 2 + 1], 0.0f, p.scale, p.base, p.act.box_lo,
                                                           p.act.box_hi, 1, nullptr);
            int k;
            const float2 a = eval_project<ENV, BUD>(p, c, lds.in_s + tid * kInS, i, ap, k);
            reinterpret_cast<float2*>(p.act.action)[i] = a;
            constexpr int kObs = EvalEnv<ENV>::kObs, kW = trace_width(kObs, 1, 2);
            if (REC && i < p.trace_rows)
                rpo_eval_dev::trace_store_head<kObs>(p.trace + ((size_t)s * p.trace_rows + i) * kW, lds.in_s + tid * kInS, ap, a, k);
            float reward, done, ineq, eq, gi[EvalEnv<ENV>::kIneq], he[EvalEnv<ENV>::kEq];
            EvalEnv<ENV>::lane(p.step, c, i, EvalEnv<ENV>::template true_state<NOISE>(p.step, i, lds.in_s + tid * kInS), a, reward,
                               done, ineq, eq, gi, he);
            if (REC && i < p.trace_rows)
                rpo_eval_dev::trace_store_tail(p.trace + ((size_t)s * p.trace_rows + i) * kW + trace_head(kObs, 1, 2), reward, done,
                                               ineq, eq);
            if constexpr (CON)
                rpo_eval_dev::rpo_eval_con_lane_update(p.con + (size_t)i * con_width(EvalEnv<ENV>::kIneq, EvalEnv<ENV>::kEq), s, gi, he,
                                                       p.step.viol_thresh);
            rpo_eval_lane_update(p.acc + (size_t)i * RPO_EVAL_LEN, s, reward, ineq, eq, done, k, p.step.viol_thresh);
        }
        __syncthreads();                                         // every lane has read its observation out of the LDS tile
    }
}

template <class ENV, int REC, int CON, int NOISE = 0, int BUD = 0, int POL = 0, int NSW = 0>
int launch_eval(const typename EvalArgsOf<ENV, CON, NOISE, BUD, POL, NSW>::type& args, const typename ENV::Consts& c, int n, void* stream) {
    // the rollout's tile rule (fused.hip launch_rollout): 64 lanes per workgroup once that still fills the chip.  E = 128
    // only: the E = 256 instance spills (~150 bytes of scratch per lane) -- such actors evaluate on the stepwise path.
    if (args.actor.E != 128) return RPO_ERR_ARG;
    if (n >= 64 * 192) {
        hipLaunchKernelGGL((eval_kernel<ENV, 128, 256, 4, REC, CON, NOISE, BUD, POL, NSW>), dim3((n + 63) / 64), dim3(kFwdThreads), 0, (hipStream_t)stream, args, c);
    } else {
        hipLaunchKernelGGL((eval_kernel<ENV, 128, 256, 1, REC, CON, NOISE, BUD, POL, NSW>), dim3((n + 15) / 16), dim3(kFwdThreads), 0, (hipStream_t)stream, args, c);
    }
    RPO_LAUNCH_CHECK();
    return 0;
}

// The sigma of the *_evaluate_noisy entry points: `len` host floats, finite and >= 0 (checked before any HIP call).
struct EvalNoise {
    const float* sigma_host;
    int len;
    unsigned long long seed;
};
int check_eval_noise(const EvalNoise& nz, int obs_dim) {
    if (!nz.sigma_host) return RPO_ERR_NULL;
    if (nz.len != obs_dim) return RPO_ERR_ARG;
    for (int q = 0; q < obs_dim; ++q)
        if (!(nz.sigma_host[q] >= 0.0f) || !__builtin_isfinite(nz.sigma_host[q])) return RPO_ERR_ARG;
    return 0;
}

// The per-lane budgets of the *_evaluate_budgets entry points: device arrays [n], 4-byte aligned.
struct EvalLanes {
    const int* steps;
    const float* lr;
};
int check_eval_lanes(const EvalLanes& l) {
    if (!l.steps || !l.lr) return RPO_ERR_NULL;
    return (reinterpret_cast<uintptr_t>(l.steps) | reinterpret_cast<uintptr_t>(l.lr)) % 4 ? RPO_ERR_ARG : 0;
}

// The groups of the *_evaluate_policies entry points (checked before any HIP call).
struct EvalGroups {
    int policy_stride, group_lanes, episodes;
};
int check_eval_groups(const EvalGroups& g, int n) {
    if (g.policy_stride <= 0 || g.policy_stride % 4 || g.group_lanes <= 0 || g.group_lanes % 64) return RPO_ERR_ARG;
    if (g.episodes < 1 || g.episodes > g.group_lanes || n < g.group_lanes || n % g.group_lanes) return RPO_ERR_ARG;
    return 0;
}

// The noise levels of the *_evaluate_noise_sweep entry points (checked before any HIP call): the table is on the DEVICE, so its
// values are the caller's to check.
struct EvalNoiseGroups {
    const float* sigma_table;
    unsigned long long seed;
    int group_lanes, episodes;
};
int check_eval_noise_groups(const EvalNoiseGroups& g, int n) {
    if (!g.sigma_table) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(g.sigma_table) % 4) return RPO_ERR_ARG;
    if (g.group_lanes <= 0 || g.group_lanes % 64) return RPO_ERR_ARG;
    if (g.episodes < 1 || g.episodes > g.group_lanes || n < g.group_lanes || n % g.group_lanes) return RPO_ERR_ARG;
    return 0;
}

// What every rpo_<env>_evaluate* entry point takes (the EVAL_COMMON list at the entry points fills it in this order).  CartSafe's
// observation IS its state: obs = state there; SpringPendulum has no constants: consts_host = NULL.
struct EvalCommon {
    const rpo_mlp* actor_host;
    void* stream;
    int gauss, n, t0, steps, max_steps, max_episode_steps, partial;
    float scale, base, box_lo, box_hi, corr_lr, corr_eps, corr_momentum, viol_thresh;
    float *state, *obs, *action, *ep_ret, *acc;
    int* ep_len;
    unsigned* ep_count;
    long long* ctrl;
    const float* consts_host;
};

// What an entry point adds to rpo_<env>_evaluate; value-initialised: nothing.  One variant at most, by construction.
enum EvalVariant { kEvalPlain, kEvalNoisy, kEvalBudgets, kEvalPolicies, kEvalNoiseSweep };   // from kEvalBudgets on: no record
struct EvalOpts {
    int rec, with_con;            // the entry point takes a record / a report at all: a NULL one is then RPO_ERR_NULL
    float *trace, *con;
    int trace_rows, trace_steps;
    EvalVariant variant;          // which of the four below counts
    EvalNoise noise;              // -> the NOISE = 1 instances
    EvalLanes lanes;              // -> the BUD = 1 instances
    EvalGroups groups;            // -> the POL = 1 instances
    EvalNoiseGroups sweep;        // -> the NSW = 1 instances
};

// The instance's arguments: the base copied, con set (NULL for the CON = 0 instances, which never read it), the rest zero.
template <class ARGS, class ENV>
ARGS eval_args_of(const EvalArgs<ENV>& args, float* con) {
    ARGS a{};
    static_cast<EvalArgs<ENV>&>(a) = args;
    a.con = con;
    return a;
}

// The options of the entry points -> the instance; no report: the launches of rpo_<env>_evaluate[_record] as they were.
template <class ENV>
int launch_eval_any(const EvalArgs<ENV>& args, const typename ENV::Consts& c, int n, const EvalOpts& o, void* stream) {
    const int rec = o.rec;
    float* con = o.with_con ? o.con : nullptr;
    if (o.variant == kEvalNoiseSweep) {
        auto sa = eval_args_of<EvalNoiseSweepArgs<ENV>>(args, con);
        sa.sigma_table = o.sweep.sigma_table;
        sa.noise_seed = o.sweep.seed;
        sa.group_lanes = o.sweep.group_lanes;
        sa.episodes = o.sweep.episodes;
        return con ? launch_eval<ENV, 0, 1, 1, 0, 0, 1>(sa, c, n, stream) : launch_eval<ENV, 0, 0, 1, 0, 0, 1>(sa, c, n, stream);
    }
    if (o.variant == kEvalPolicies) {
        auto pa = eval_args_of<EvalPolArgs<ENV>>(args, con);
        pa.policy_stride = o.groups.policy_stride;
        pa.group_lanes = o.groups.group_lanes;
        pa.episodes = o.groups.episodes;
        return con ? launch_eval<ENV, 0, 1, 0, 0, 1>(pa, c, n, stream) : launch_eval<ENV, 0, 0, 0, 0, 1>(pa, c, n, stream);
    }
    if (o.variant == kEvalBudgets) {
        auto ba = eval_args_of<EvalBudArgs<ENV>>(args, con);
        ba.lane_steps = o.lanes.steps;
        ba.lane_lr = o.lanes.lr;
        return con ? launch_eval<ENV, 0, 1, 0, 1>(ba, c, n, stream) : launch_eval<ENV, 0, 0, 0, 1>(ba, c, n, stream);
    }
    if (o.variant == kEvalNoisy) {
        auto na = eval_args_of<EvalNoiseArgs<ENV>>(args, con);
        for (int q = 0; q < o.noise.len; ++q) na.sigma[q] = o.noise.sigma_host[q];
        na.noise_seed = o.noise.seed;
        if (!con) return rec ? launch_eval<ENV, 1, 0, 1>(na, c, n, stream) : launch_eval<ENV, 0, 0, 1>(na, c, n, stream);
        return rec ? launch_eval<ENV, 1, 1, 1>(na, c, n, stream) : launch_eval<ENV, 0, 1, 1>(na, c, n, stream);
    }
    if (!con) return rec ? launch_eval<ENV, 1, 0>(args, c, n, stream) : launch_eval<ENV, 0, 0>(args, c, n, stream);
    const auto ca = eval_args_of<EvalConArgs<ENV>>(args, con);
    return rec ? launch_eval<ENV, 1, 1>(ca, c, n, stream) : launch_eval<ENV, 0, 1>(ca, c, n, stream);
}

// The trace arguments of the *_evaluate_record entry points: 1 <= R <= n rows per step, steps [t0, t0 + steps) inside the
// buffer's T steps, 16-byte aligned for the float4 stores.
int check_eval_trace(const float* trace, int n, int trace_rows, int trace_steps, int t0, int steps) {
    if (!trace) return RPO_ERR_NULL;
    if (trace_rows <= 0 || trace_rows > n || trace_steps <= 0 || (long long)t0 + steps > trace_steps) return RPO_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(trace) % 16) return RPO_ERR_ARG;
    return 0;
}

// ------------------------------------------------------------------------------------------- stepwise accumulation
struct AccArgs {
    int n;
    const float* rows;
    int stride, reward_col, done_col, eq_col, eq_num, ineq_col, ineq_num;
    const int* iters;
    int step;
    float viol_thresh;
    float* acc;
};

__global__ __launch_bounds__(RPO_BLOCK) void eval_accumulate_kernel(AccArgs p) {
    for (int i = blockIdx.x * RPO_BLOCK + threadIdx.x; i < p.n; i += gridDim.x * RPO_BLOCK) {
        const float* r = p.rows + (size_t)i * p.stride;
        float ineq, eq;
        row_violations(r, p.ineq_col, p.ineq_num, p.eq_col, p.eq_num, ineq, eq);
        rpo_eval_lane_update(p.acc + (size_t)i * RPO_EVAL_LEN, p.step, r[p.reward_col], ineq, eq, r[p.done_col],
                             p.iters ? p.iters[i] : 0, p.viol_thresh);
    }
}

// ------------------------------------------------------------------------------------------- stepwise record
struct RecArgs {
    AccArgs a;                    // the transition rows and their columns, the step, the accumulators (liveness)
    const float *obs, *proposal, *action;
    int obs_stride, O, P, A;
    float* trace;                 // [., R, W]
    int R, head, W;
};

// element c of lane i's row head: obs | proposal | action | iterations | zeros
__device__ __forceinline__ float record_head_element(const RecArgs& p, int i, int c) {
    if (c < p.O) return p.obs[(size_t)i * p.obs_stride + c];
    c -= p.O;
    if (c < p.P) return p.proposal[(size_t)i * p.P + c];
    c -= p.P;
    if (c < p.A) return p.action[(size_t)i * p.A + c];
    return c == p.A && p.a.iters ? (float)p.a.iters[i] : 0.0f;
}

// One thread per 16-byte chunk of a row: the chunks of a step's R rows are contiguous, so a wave stores 1 KiB in a piece.
__global__ __launch_bounds__(RPO_BLOCK) void eval_record_kernel(RecArgs p) {
    const int chunks = p.W / 4;
    const long long total = (long long)p.R * chunks;
    for (long long t = (long long)blockIdx.x * RPO_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * RPO_BLOCK) {
        const int i = (int)(t / chunks), c = (int)(t - (long long)i * chunks) * 4;
        if (p.a.step > 0 && !(__float_as_int(p.a.acc[(size_t)i * RPO_EVAL_LEN + RPO_EVAL_WORD]) & RPO_EVAL_ALIVE)) continue;
        float* dst = p.trace + ((size_t)p.a.step * p.R + i) * p.W + c;
        if (c < p.head) {
            rpo_eval_dev::trace_store(dst, record_head_element(p, i, c), record_head_element(p, i, c + 1),
                                      record_head_element(p, i, c + 2), record_head_element(p, i, c + 3));
        } else {
            const float* r = p.a.rows + (size_t)i * p.a.stride;
            float ineq, eq;
            row_violations(r, p.a.ineq_col, p.a.ineq_num, p.a.eq_col, p.a.eq_num, ineq, eq);
            rpo_eval_dev::trace_store_tail(dst, r[p.a.reward_col], r[p.a.done_col], ineq, eq);
        }
    }
}

// ------------------------------------------------------------------------------------------- stepwise observation noise
struct NoiseArgs {
    int n;
    const float* obs;
    int obs_stride, O;
    const float* sigma;           // device, [O]
    uint64_t seed;
    int step;
    float* out;
    int out_stride;
};

// One thread per element: a wave reads and writes neighbouring columns of neighbouring rows.
__global__ __launch_bounds__(RPO_BLOCK) void eval_obs_noise_kernel(NoiseArgs p) {
    const long long total = (long long)p.n * p.O;
    for (long long t = (long long)blockIdx.x * RPO_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * RPO_BLOCK) {
        const int i = (int)(t / p.O), q = (int)(t - (long long)i * p.O);
        p.out[(size_t)i * p.out_stride + q] =
            rpo_eval_dev::rpo_eval_noisy_obs(p.obs[(size_t)i * p.obs_stride + q], p.sigma[q], p.seed, i, p.step, q);
    }
}

// ------------------------------------------------------------------------------------------- stepwise per-constraint report
struct ConArgs {
    int n;
    const float* rows;
    int stride, eq_col, eq_num, ineq_col, ineq_num, step;
    float viol_thresh;
    const float* acc;
    float* con;                   // [n, W]
    int W;
};

// One thread per (lane, cell): the threads of a wave read neighbouring columns of a transition row (ineq_viol twice, then
// eq_viol) and store neighbouring cells -- the cells of a step's lanes are contiguous.  Every cell has one owner.
__global__ __launch_bounds__(RPO_BLOCK) void eval_constraints_kernel(ConArgs p) {
    const long long total = (long long)p.n * p.W;
    for (long long t = (long long)blockIdx.x * RPO_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * RPO_BLOCK) {
        const int i = (int)(t / p.W), c = (int)(t - (long long)i * p.W);
        if (p.step > 0 && !(__float_as_int(p.acc[(size_t)i * RPO_EVAL_LEN + RPO_EVAL_WORD]) & RPO_EVAL_ALIVE)) continue;
        const int j = rpo_eval_dev::con_cell_source(c, p.ineq_num, p.eq_num);
        const float v = j < 0 ? 0.0f : p.rows[(size_t)i * p.stride + (c < 2 * p.ineq_num ? p.ineq_col : p.eq_col) + j];
        const float old = p.step > 0 ? p.con[t] : 0.0f;
        p.con[t] = rpo_eval_dev::rpo_eval_con_cell(c, p.ineq_num, p.eq_num, old, v, p.viol_thresh);
    }
}

// ------------------------------------------------------------------------------------------- curve rows (rpo_eval_summarize)
// Eight float64 sums per evaluation: the five summarised accumulator columns (RPO_EVAL_RET .. RPO_EVAL_MAX_EQ, widened), the
// lengths, the violating steps and the non-finite episodes (counts: exact in a double whatever the order).  Workgroup b owns
// rows [b * chunk, (b + 1) * chunk) and slot b of the workspace; nothing is added atomically.
constexpr int kSumK = 8, kSumStats = 5, kSumSlots = 256, kSumRowsPerBlock = 1024;
static_assert(RPO_CURVE_WS >= 2 * kSumSlots * kSumK, "workspace: two planes of per-workgroup partials");
static_assert(RPO_CURVE_MAX_EPISODES <= kSumSlots * 4096, "chunks of at most 4096 rows");

__device__ __forceinline__ double wave_sum_f64(double v) {       // rpo_wave_sum's butterfly on doubles
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, RPO_WAVE);
    return v;
}

// Sum of v[k] over the 256 threads of the workgroup, the same bits in every thread: butterfly inside each wave, then
// (w0 + w1) + (w2 + w3).  lds: [4 * kSumK] doubles.
__device__ __forceinline__ void block_sum_f64(double (&v)[kSumK], double* lds) {
    const int lane = threadIdx.x & (RPO_WAVE - 1), wave = threadIdx.x / RPO_WAVE;
#pragma unroll
    for (int k = 0; k < kSumK; ++k) {
        const double r = wave_sum_f64(v[k]);
        if (lane == 0) lds[wave * kSumK + k] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSumK; ++k) v[k] = (lds[k] + lds[kSumK + k]) + (lds[2 * kSumK + k] + lds[3 * kSumK + k]);
    __syncthreads();                                             // (the caller may reuse lds)
}

// The slots of one workspace plane combined in slot order: thread t holds slot t (zeros beyond `slots`), then block_sum_f64.
__device__ __forceinline__ void combine_slots(const double* plane, int slots, double (&v)[kSumK], double* lds) {
#pragma unroll
    for (int k = 0; k < kSumK; ++k) v[k] = (int)threadIdx.x < slots ? plane[threadIdx.x * kSumK + k] : 0.0;
    block_sum_f64(v, lds);
}

// phase 0: the eight sums of the workgroup's rows; phase 1: the squared deviations of the five columns about mean[] (slots
// kSumStats.. stay zero)
__device__ __forceinline__ void chunk_sums(const float* acc, int n, int chunk, int phase, const double (&mean)[kSumK],
                                           double (&v)[kSumK], double* lds) {
    const int lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
#pragma unroll
    for (int k = 0; k < kSumK; ++k) v[k] = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += RPO_BLOCK) {
        const float* r = acc + (size_t)i * RPO_EVAL_LEN;
        if (phase == 0) {
#pragma unroll
            for (int k = 0; k < kSumStats; ++k) v[k] += (double)r[RPO_EVAL_RET + k];
            const int word = __float_as_int(r[RPO_EVAL_WORD]);
            v[5] += (double)(word >> RPO_EVAL_LEN_SHIFT);
            v[6] += (double)r[RPO_EVAL_VIOL_STEPS];
            v[7] += (word & RPO_EVAL_NONFINITE) ? 1.0 : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < kSumStats; ++k) {
                const double d = (double)r[RPO_EVAL_RET + k] - mean[k];
                v[k] += d * d;
            }
        }
    }
    block_sum_f64(v, lds);
}

__device__ __forceinline__ void write_curve_row(double* row, const long long* ctrl, int n, const double (&sum)[kSumK],
                                                const double (&mean)[kSumK], const double (&sq)[kSumK]) {
    if (threadIdx.x != 0) return;
    row[RPO_CURVE_STEP] = (double)ctrl[RPO_CTRL_T];
    row[RPO_CURVE_EPISODES] = (double)n;
#pragma unroll
    for (int k = 0; k < kSumStats; ++k) {
        row[RPO_CURVE_STATS + 2 * k] = mean[k];
        row[RPO_CURVE_STATS + 2 * k + 1] = sqrt(sq[k] / (double)n);
    }
    row[RPO_CURVE_LENGTH] = sum[5];
    row[RPO_CURVE_VIOL_STEPS] = sum[6];
    row[RPO_CURVE_NONFINITE] = sum[7];
    row[RPO_CURVE_LEN - 1] = 0.0;
}

__device__ __forceinline__ void means_of(const double (&sum)[kSumK], int n, double (&mean)[kSumK]) {
#pragma unroll
    for (int k = 0; k < kSumK; ++k) mean[k] = k < kSumStats ? sum[k] / (double)n : 0.0;
}

// n <= kSumRowsPerBlock: everything in one workgroup
__global__ __launch_bounds__(RPO_BLOCK) void summarize_one_kernel(int n, const float* acc, const long long* ctrl, double* row) {
    __shared__ double lds[4 * kSumK];
    double sum[kSumK], mean[kSumK], sq[kSumK];
#pragma unroll
    for (int k = 0; k < kSumK; ++k) mean[k] = 0.0;
    chunk_sums(acc, n, n, 0, mean, sum, lds);
    means_of(sum, n, mean);
    chunk_sums(acc, n, n, 1, mean, sq, lds);
    write_curve_row(row, ctrl, n, sum, mean, sq);
}

// launches 1 and 2 of the large form: plane 0 <- chunk sums; plane 1 <- chunk sums of squared deviations about the mean every
// workgroup derives from plane 0 by the same combine
__global__ __launch_bounds__(RPO_BLOCK) void summarize_chunks_kernel(int n, const float* acc, int chunk, int phase, double* ws) {
    __shared__ double lds[4 * kSumK];
    double sum[kSumK], mean[kSumK], v[kSumK];
#pragma unroll
    for (int k = 0; k < kSumK; ++k) mean[k] = 0.0;
    if (phase == 1) {
        combine_slots(ws, gridDim.x, sum, lds);
        means_of(sum, n, mean);
    }
    chunk_sums(acc, n, chunk, phase, mean, v, lds);
    if (threadIdx.x < kSumK) {
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < kSumK; ++k)
            if ((int)threadIdx.x == k) mine = v[k];
        ws[(size_t)phase * kSumSlots * kSumK + blockIdx.x * kSumK + threadIdx.x] = mine;
    }
}

__global__ __launch_bounds__(RPO_BLOCK) void summarize_combine_kernel(int n, int slots, const double* ws, const long long* ctrl,
                                                                      double* row) {
    __shared__ double lds[4 * kSumK];
    double sum[kSumK], mean[kSumK], sq[kSumK];
    combine_slots(ws, slots, sum, lds);
    means_of(sum, n, mean);
    combine_slots(ws + kSumSlots * kSumK, slots, sq, lds);
    write_curve_row(row, ctrl, n, sum, mean, sq);
}

// ------------------------------------------------------------------------------------------- keep-best (rpo_eval_keep_best)
// decide: ONE wave.  Every lane reads both rows and the held point (wave-uniform loads) and evaluates the criterion, so the
// verdict is uniform; the loads of all lanes precede the stores in program order, and the stores have one owner each:
// lane c < RPO_CURVE_LEN writes best_row[c], lane RPO_CURVE_LEN writes best_point[0].  A losing candidate writes nothing.
__global__ __launch_bounds__(RPO_WAVE) void keep_best_decide_kernel(const double* row, double* best_row, long long* best_point,
                                                                    long long point, double max_violation_rate) {
    static_assert(RPO_CURVE_LEN < RPO_WAVE, "one lane per word of the row and one for the point");
    const int lane = threadIdx.x;
    const double mine = lane < RPO_CURVE_LEN ? row[lane] : 0.0;
    const bool wins = rpo_eval_dev::keep_best_wins(row, best_row, best_point[0], max_violation_rate);
    if (!wins) return;
    if (lane < RPO_CURVE_LEN) best_row[lane] = mine;
    else if (lane == RPO_CURVE_LEN) best_point[0] = point;
}

typedef float keep_v4 __attribute__((ext_vector_type(4)));

// copy: predicated on the word the decide launch left (stream order makes it visible).  head: the floats in front of the
// first 16-byte boundary of BOTH pointers -- all n when they sit at different offsets from one; then n4 16-byte chunks;
// then the tail.  Grid-stride loops, 64-bit indices; every float of best has one writer.
__global__ __launch_bounds__(RPO_BLOCK) void keep_best_copy_kernel(long long n, long long head, long long n4,
                                                                   const float* __restrict__ src, float* __restrict__ best,
                                                                   const long long* best_point, long long point) {
    if (best_point[0] != point) return;
    const long long tid = (long long)blockIdx.x * RPO_BLOCK + threadIdx.x, stride = (long long)gridDim.x * RPO_BLOCK;
    const keep_v4* s4 = reinterpret_cast<const keep_v4*>(src + head);
    keep_v4* d4 = reinterpret_cast<keep_v4*>(best + head);
    for (long long i = tid; i < n4; i += stride) d4[i] = s4[i];
    for (long long i = tid; i < head; i += stride) best[i] = src[i];
    for (long long i = head + 4 * n4 + tid; i < n; i += stride) best[i] = src[i];
}

// Host side of the entry points: what the two envs differ in beyond EvalEnv<ENV>::kObs, overloaded on the env's types -- loading
// the constants and building ActArgs / StepArgs (projection: RPO_NOISE_NONE; step: rows = NULL, auto_reset = 0).
int eval_consts(rpo_cart_dev::CartConsts& c, const EvalCommon& q) { return rpo_cart_dev::load_consts(c, q.consts_host, q.partial); }
int eval_consts(PendEnv::Consts& c, const EvalCommon&) { c.unused = 0; return 0; }

void eval_env_args(const EvalCommon& q, rpo_cart_dev::ActArgs& act, rpo_cart_dev::StepArgs& step) {
    act = rpo_cart_dev::ActArgs{q.n, nullptr, nullptr, q.action, nullptr, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f, q.box_lo, q.box_hi,
                                q.max_steps, q.corr_lr, q.corr_eps, q.corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    step = rpo_cart_dev::StepArgs{q.n, q.state, q.action, q.ep_len, q.ep_ret, q.ep_count, nullptr, 1, nullptr, 0, q.ctrl,
                                  q.max_episode_steps, 0, q.viol_thresh, 0ull, 0u, 0};
}
void eval_env_args(const EvalCommon& q, rpo_pend_dev::ActArgs& act, rpo_pend_dev::StepArgs& step) {
    act = rpo_pend_dev::ActArgs{q.n, nullptr, 5, nullptr, nullptr, q.action, nullptr, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f, q.box_lo,
                                q.box_hi, q.max_steps, q.corr_lr, q.corr_eps, q.corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    step = rpo_pend_dev::StepArgs{q.n, q.state, q.obs, q.action, q.ep_len, q.ep_ret, q.ep_count, nullptr, 1, nullptr, 0, q.ctrl,
                                  q.max_episode_steps, 0, q.viol_thresh, 0ull, 0u};
}

// Every rpo_<env>_evaluate* entry point: the validation in one order, then the launch.
template <class ENV>
int evaluate_entry(const EvalCommon& q, const EvalOpts& o) {
    constexpr int kObs = EvalEnv<ENV>::kObs;
    if (!q.actor_host) return RPO_ERR_NULL;
    if (int e = check_eval_range(q.n, q.t0, q.steps, q.max_episode_steps, q.max_steps)) return e;
    if (o.variant == kEvalNoisy)
        if (int e = check_eval_noise(o.noise, kObs)) return e;
    if (!q.state || !q.obs || !q.action || !q.ep_len || !q.ep_ret || !q.ep_count || !q.acc) return RPO_ERR_NULL;
    if (int e = o.variant == kEvalBudgets      ? check_eval_lanes(o.lanes)
                : o.variant == kEvalPolicies   ? check_eval_groups(o.groups, q.n)
                : o.variant == kEvalNoiseSweep ? check_eval_noise_groups(o.sweep, q.n)
                                               : 0)
        return e;
    // which variants exclude each other (the host's statement of eval_kernel's static_asserts): EvalOpts holds one variant at
    // most, and per-lane budgets, policy groups and noise groups run without a record
    if (o.rec && o.variant >= kEvalBudgets) return RPO_ERR_ARG;
    if (o.rec)
        if (int e = check_eval_trace(o.trace, q.n, o.trace_rows, o.trace_steps, q.t0, q.steps)) return e;
    if (o.with_con)
        if (int e = check_eval_con(o.con)) return e;
    EvalArgs<ENV> args{};
    args.actor = to_dev(q.actor_host);
    if (int e = check_actor(args.actor, kObs, q.gauss)) return e;
    typename ENV::Consts c;
    if (int e = eval_consts(c, q)) return e;
    args.scale = q.scale; args.base = q.base; args.gauss = q.gauss ? 1 : 0; args.t0 = q.t0; args.steps = q.steps; args.acc = q.acc;
    eval_env_args(q, args.act, args.step);
    args.trace = o.rec ? o.trace : nullptr;
    args.trace_rows = o.rec ? o.trace_rows : 0;
    return launch_eval_any<ENV>(args, c, q.n, o, q.stream);
}

// The record and the report where the caller handed one over (the arguments of the entry points from _constraints on).
EvalOpts eval_opts(float* trace, int trace_rows, int trace_steps, float* con, EvalVariant variant = kEvalPlain) {
    EvalOpts o{};
    o.rec = trace ? 1 : 0; o.trace = trace; o.trace_rows = trace_rows; o.trace_steps = trace_steps;
    o.with_con = con ? 1 : 0; o.con = con;
    o.variant = variant;
    return o;
}

}  // namespace

extern "C" {

int rpo_eval_summarize(int n, const float* acc, const long long* ctrl, double* row_out, double* ws, void* stream) {
    if (n <= 0 || n > RPO_CURVE_MAX_EPISODES) return RPO_ERR_ARG;
    if (!acc || !ctrl || !row_out || !ws) return RPO_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    if (n <= kSumRowsPerBlock) {
        hipLaunchKernelGGL(summarize_one_kernel, dim3(1), dim3(RPO_BLOCK), 0, s, n, acc, ctrl, row_out);
        RPO_LAUNCH_CHECK();
        return 0;
    }
    // slots and chunk are functions of n alone: min(256, ceil(n / 1024)) workgroups, equal chunks rounded up to whole blocks
    const int slots = min(kSumSlots, (n + kSumRowsPerBlock - 1) / kSumRowsPerBlock);
    const int chunk = ((n + slots - 1) / slots + RPO_BLOCK - 1) / RPO_BLOCK * RPO_BLOCK;
    for (int phase = 0; phase < 2; ++phase) {
        hipLaunchKernelGGL(summarize_chunks_kernel, dim3(slots), dim3(RPO_BLOCK), 0, s, n, acc, chunk, phase, ws);
        RPO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(summarize_combine_kernel, dim3(1), dim3(RPO_BLOCK), 0, s, n, slots, (const double*)ws, ctrl, row_out);
    RPO_LAUNCH_CHECK();
    return 0;
}

int rpo_eval_keep_best(long long n_params, const float* src, float* best, const double* row, double* best_row,
                       long long* best_point, long long point, double max_violation_rate, void* stream) {
    if (n_params < 1 || point < 0 || !(max_violation_rate >= 0.0)) return RPO_ERR_ARG;
    if (!src || !best || !row || !best_row || !best_point) return RPO_ERR_NULL;
    const unsigned so = (unsigned)((uintptr_t)src & 15u), bo = (unsigned)((uintptr_t)best & 15u);
    if (((so | bo) & 3u) || (((uintptr_t)row | (uintptr_t)best_row | (uintptr_t)best_point) & 7u)) return RPO_ERR_ARG;
    // the same offset from a 16-byte boundary: scalar floats up to it, 16-byte chunks, scalar tail; otherwise all scalar
    const long long to_boundary = ((16u - so) & 15u) / 4u;
    const long long head = so != bo ? n_params : (to_boundary < n_params ? to_boundary : n_params);
    const long long n4 = (n_params - head) / 4;
    const long long widest = n4 > head ? n4 : head;            // (the tail is at most 3 floats: one workgroup at least)
    const long long want = (widest + RPO_BLOCK - 1) / RPO_BLOCK;
    const int blocks = (int)(want < 1 ? 1 : (want > RPO_MAX_GRID ? RPO_MAX_GRID : want));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(keep_best_decide_kernel, dim3(1), dim3(RPO_WAVE), 0, s, row, best_row, best_point, point,
                       max_violation_rate);
    RPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(keep_best_copy_kernel, dim3(blocks), dim3(RPO_BLOCK), 0, s, n_params, head, n4, src, best,
                       (const long long*)best_point, point);
    RPO_LAUNCH_CHECK();
    return 0;
}

// The arguments every rpo_<env>_evaluate* entry point declares under these names, in EvalCommon's order.
#define EVAL_COMMON(STATE, OBS, CONSTS, PARTIAL)                                                                                  \
    EvalCommon{actor_host, stream, gauss, n_envs, t0, steps, max_steps, max_episode_steps, PARTIAL, scale, base, box_lo, box_hi,  \
               corr_lr, corr_eps, corr_momentum, viol_thresh, STATE, OBS, action, ep_ret, acc, ep_len, ep_count, ctrl, CONSTS}
#define EVAL_CART EVAL_COMMON(state, state, consts_host, partial)
#define EVAL_PEND EVAL_COMMON(internal, obs, nullptr, 0)

int rpo_cartsafe_evaluate(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                          float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc, int t0,
                          int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                          float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                          float viol_thresh, void* stream) {
    return evaluate_entry<CartEnv>(EVAL_CART, EvalOpts{});
}

int rpo_cartsafe_evaluate_record(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                 float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                 int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                 float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                 float viol_thresh, float* trace, int trace_rows, int trace_steps, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, nullptr);
    o.rec = 1;
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                          float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                          float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                          float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, void* stream) {
    return evaluate_entry<PendEnv>(EVAL_PEND, EvalOpts{});
}

int rpo_pendulum_evaluate_record(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                 float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                 float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                 float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                 int trace_rows, int trace_steps, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, nullptr);
    o.rec = 1;
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_cartsafe_evaluate_constraints(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                      float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                      float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                      float corr_eps, float corr_momentum, const float* consts_host, int partial,
                                      int max_episode_steps, float viol_thresh, float* trace, int trace_rows, int trace_steps,
                                      float* con, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con);
    o.with_con = 1;
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate_constraints(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs,
                                      float* internal, float* obs, float* action, int* ep_len, float* ep_ret,
                                      unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, float box_lo,
                                      float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                      int max_episode_steps, float viol_thresh, float* trace, int trace_rows, int trace_steps,
                                      float* con, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con);
    o.with_con = 1;
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_cartsafe_evaluate_noisy(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                float viol_thresh, float* trace, int trace_rows, int trace_steps, float* con,
                                const float* sigma_host, int sigma_len, unsigned long long noise_seed, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con, kEvalNoisy);
    o.noise = EvalNoise{sigma_host, sigma_len, noise_seed};
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate_noisy(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                int trace_rows, int trace_steps, float* con, const float* sigma_host, int sigma_len,
                                unsigned long long noise_seed, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con, kEvalNoisy);
    o.noise = EvalNoise{sigma_host, sigma_len, noise_seed};
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_cartsafe_evaluate_budgets(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                  float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                  int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                  float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                  float viol_thresh, float* trace, int trace_rows, int trace_steps, float* con,
                                  const int* lane_steps, const float* lane_lr, void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con, kEvalBudgets);
    o.lanes = EvalLanes{lane_steps, lane_lr};
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate_budgets(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                  float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                  float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                  float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                  int trace_rows, int trace_steps, float* con, const int* lane_steps, const float* lane_lr,
                                  void* stream) {
    EvalOpts o = eval_opts(trace, trace_rows, trace_steps, con, kEvalBudgets);
    o.lanes = EvalLanes{lane_steps, lane_lr};
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_cartsafe_evaluate_policies(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                   float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                   int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                   float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                   float viol_thresh, float* con, int policy_stride, int group_lanes, int episodes,
                                   void* stream) {
    EvalOpts o = eval_opts(nullptr, 0, 0, con, kEvalPolicies);
    o.groups = EvalGroups{policy_stride, group_lanes, episodes};
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate_policies(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                   float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                   float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                   float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* con,
                                   int policy_stride, int group_lanes, int episodes, void* stream) {
    EvalOpts o = eval_opts(nullptr, 0, 0, con, kEvalPolicies);
    o.groups = EvalGroups{policy_stride, group_lanes, episodes};
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_cartsafe_evaluate_noise_sweep(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                      float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                      float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                      float corr_eps, float corr_momentum, const float* consts_host, int partial,
                                      int max_episode_steps, float viol_thresh, float* con, const float* sigma_table,
                                      unsigned long long noise_seed, int group_lanes, int episodes, void* stream) {
    EvalOpts o = eval_opts(nullptr, 0, 0, con, kEvalNoiseSweep);
    o.sweep = EvalNoiseGroups{sigma_table, noise_seed, group_lanes, episodes};
    return evaluate_entry<CartEnv>(EVAL_CART, o);
}

int rpo_pendulum_evaluate_noise_sweep(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs,
                                      float* internal, float* obs, float* action, int* ep_len, float* ep_ret,
                                      unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, float box_lo,
                                      float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                      int max_episode_steps, float viol_thresh, float* con, const float* sigma_table,
                                      unsigned long long noise_seed, int group_lanes, int episodes, void* stream) {
    EvalOpts o = eval_opts(nullptr, 0, 0, con, kEvalNoiseSweep);
    o.sweep = EvalNoiseGroups{sigma_table, noise_seed, group_lanes, episodes};
    return evaluate_entry<PendEnv>(EVAL_PEND, o);
}

int rpo_eval_obs_noise(int n, const float* obs, int obs_stride, int obs_dim, const float* sigma, unsigned long long seed,
                       int step, float* out, int out_stride, void* stream) {
    if (n <= 0 || step < 0 || step >= (1 << 24) || obs_dim <= 0 || obs_dim > 4096 || obs_stride < obs_dim || out_stride < obs_dim)
        return RPO_ERR_ARG;
    if (!obs || !sigma || !out) return RPO_ERR_NULL;
    if (out == obs) return RPO_ERR_ARG;
    const NoiseArgs a{n, obs, obs_stride, obs_dim, sigma, (uint64_t)seed, step, out, out_stride};
    hipLaunchKernelGGL(eval_obs_noise_kernel, dim3(rpo_grid_for((long long)n * obs_dim)), dim3(RPO_BLOCK), 0, (hipStream_t)stream, a);
    RPO_LAUNCH_CHECK();
    return 0;
}

int rpo_eval_constraints(int n, const float* rows, int row_stride, int eq_col, int eq_num, int ineq_col, int ineq_num, int step,
                         float viol_thresh, const float* acc, float* con, void* stream) {
    if (n <= 0 || step < 0 || step >= (1 << 24) || eq_num <= 0 || ineq_num <= 0 || eq_col < 0 || ineq_col < 0 || eq_num > 4096 ||
        ineq_num > 4096)
        return RPO_ERR_ARG;
    if (eq_col + eq_num > row_stride || ineq_col + ineq_num > row_stride) return RPO_ERR_ARG;
    if (!rows || !acc || !con) return RPO_ERR_NULL;
    const int W = con_width(ineq_num, eq_num);
    const ConArgs a{n, rows, row_stride, eq_col, eq_num, ineq_col, ineq_num, step, viol_thresh, acc, con, W};
    hipLaunchKernelGGL(eval_constraints_kernel, dim3(rpo_grid_for((long long)n * W)), dim3(RPO_BLOCK), 0, (hipStream_t)stream, a);
    RPO_LAUNCH_CHECK();
    return 0;
}

int rpo_eval_accumulate(int n, const float* rows, int row_stride, int reward_col, int done_col, int eq_col, int eq_num,
                        int ineq_col, int ineq_num, const int* iters, int step, float viol_thresh, float* acc, void* stream) {
    if (n <= 0 || step < 0 || step >= (1 << 24) || eq_num <= 0 || ineq_num <= 0 || reward_col < 0 || done_col < 0 || eq_col < 0 ||
        ineq_col < 0)
        return RPO_ERR_ARG;
    if (reward_col >= row_stride || done_col >= row_stride || eq_col + eq_num > row_stride || ineq_col + ineq_num > row_stride)
        return RPO_ERR_ARG;
    if (!rows || !acc) return RPO_ERR_NULL;
    const AccArgs a{n, rows, row_stride, reward_col, done_col, eq_col, eq_num, ineq_col, ineq_num, iters, step, viol_thresh, acc};
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(rpo_grid_for(n)), dim3(RPO_BLOCK), 0, (hipStream_t)stream, a);
    RPO_LAUNCH_CHECK();
    return 0;
}

int rpo_eval_record(int n, const float* rows, int row_stride, int reward_col, int done_col, int eq_col, int eq_num,
                    int ineq_col, int ineq_num, const float* obs, int obs_stride, int obs_dim, const float* proposal,
                    int partial_dim, const float* action, int action_dim, const int* iters, int step, const float* acc,
                    float* trace, int trace_rows, int trace_steps, void* stream) {
    if (n <= 0 || step < 0 || step >= (1 << 24) || eq_num <= 0 || ineq_num <= 0 || reward_col < 0 || done_col < 0 || eq_col < 0 ||
        ineq_col < 0)
        return RPO_ERR_ARG;
    if (reward_col >= row_stride || done_col >= row_stride || eq_col + eq_num > row_stride || ineq_col + ineq_num > row_stride)
        return RPO_ERR_ARG;
    if (obs_dim <= 0 || partial_dim <= 0 || action_dim <= 0 || obs_dim > 4096 || partial_dim > 4096 || action_dim > 4096 ||
        obs_stride < obs_dim)
        return RPO_ERR_ARG;
    if (trace_rows <= 0 || trace_rows > n || step >= trace_steps) return RPO_ERR_ARG;
    if (!rows || !obs || !proposal || !action || !acc || !trace) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(trace) % 16) return RPO_ERR_ARG;
    RecArgs r{};
    r.a = AccArgs{n, rows, row_stride, reward_col, done_col, eq_col, eq_num, ineq_col, ineq_num, iters, step, 0.0f,
                  const_cast<float*>(acc)};              // (read only: liveness)
    r.obs = obs; r.proposal = proposal; r.action = action;
    r.obs_stride = obs_stride; r.O = obs_dim; r.P = partial_dim; r.A = action_dim;
    r.trace = trace; r.R = trace_rows;
    r.head = trace_head(obs_dim, partial_dim, action_dim);
    r.W = trace_width(obs_dim, partial_dim, action_dim);
    hipLaunchKernelGGL(eval_record_kernel, dim3(rpo_grid_for((long long)trace_rows * (r.W / 4))), dim3(RPO_BLOCK), 0,
                       (hipStream_t)stream, r);
    RPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
