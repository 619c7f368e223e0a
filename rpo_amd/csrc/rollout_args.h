// Launch arguments of the one-launch rollout, shared by its row-tile form (fused.hip) and its streaming form
// (rollout_stream.hip: a translation unit of its own, compiled without SLP vectorisation).
#pragma once
#include "mlp_tile.h"
#include "rollout_env.h"

namespace {

using rpo_mlp_dev::Mlp;

template <class ENV>
struct RolloutArgs {
    Mlp actor;
    float scale, base;            // tanh box of the actor output (BoxConstraint)
    int gauss;                    // 0: deterministic actor + exploration noise (DDPG); 1: squashed-Gaussian sample (SAC)
    int defer_clock;              // 1: the caller's next launch advances ctrl[T] and clears the next statistics row
    typename ENV::ActArgs act;    // exploration / projection parameters, action out
    typename ENV::StepArgs step;  // env state, bookkeeping, ring, statistics, ctrl
};

// ENV::ActArgs / StepArgs out of a rollout's arguments (rpo_rollout_rider carries the fields of rpo_*_rollout): the one-launch
// rollout (fused.hip) and the riding one (nsplit.hip)
inline void rollout_env_args(const rpo_rollout_rider& r, rpo_cart_dev::ActArgs& act, rpo_cart_dev::StepArgs& step) {
    act = rpo_cart_dev::ActArgs{r.n_envs, nullptr, nullptr, r.action, nullptr, r.noise_mode, r.eps_start, r.eps_end, r.eps_decay,
                                r.box_lo, r.box_hi, r.max_steps, r.corr_lr, r.corr_eps, r.corr_momentum, (uint64_t)r.seed,
                                (uint32_t)r.env_id_base, r.ctrl, r.stats, r.stats_cap};
    step = rpo_cart_dev::StepArgs{r.n_envs, r.state, r.action, r.ep_len, r.ep_ret, r.ep_count, r.rows, r.cap_steps, r.stats,
                                  r.stats_cap, r.ctrl, r.max_episode_steps, r.auto_reset, r.viol_thresh, (uint64_t)r.seed,
                                  (uint32_t)r.env_id_base, 0};
}

inline void rollout_env_args(const rpo_rollout_rider& r, rpo_pend_dev::ActArgs& act, rpo_pend_dev::StepArgs& step) {
    act = rpo_pend_dev::ActArgs{r.n_envs, nullptr, 5, nullptr, nullptr, r.action, nullptr, r.noise_mode, r.eps_start, r.eps_end,
                                r.eps_decay, r.box_lo, r.box_hi, r.max_steps, r.corr_lr, r.corr_eps, r.corr_momentum,
                                (uint64_t)r.seed, (uint32_t)r.env_id_base, r.ctrl, r.stats, r.stats_cap};
    step = rpo_pend_dev::StepArgs{r.n_envs, r.state, r.obs, r.action, r.ep_len, r.ep_ret, r.ep_count, r.rows, r.cap_steps, r.stats,
                                  r.stats_cap, r.ctrl, r.max_episode_steps, r.auto_reset, r.viol_thresh, (uint64_t)r.seed,
                                  (uint32_t)r.env_id_base};
}

}  // namespace

// The streaming form (rollout_stream.hip).  `args` / `consts`: a RolloutArgs<CartEnv | PendEnv> and that env's Consts -- passed as
// untyped pointers because the env policies live in anonymous namespaces (one type per translation unit, same layout).
// Returns -1 when the form does not apply (shape, missing observation rows), 0 after a launch, > 0 = hipError_t.
__attribute__((visibility("hidden"))) int rpo_rollout_stream_launch(int env /* 0 CartSafe, 1 SpringPendulum */, const void* args,
                                                                    const void* consts, int n_envs, void* stream);
