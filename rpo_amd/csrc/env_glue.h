// What the stand-alone entry points of cartsafe.hip and pendulum.hip share: the checks of *_step and *_act_project in the order both
// units had them, and the deterministic form of *_lagrangian with its one reduce kernel.
#pragma once
#include "common.h"
#include "launch.h"

namespace rpo_env_glue {

using rpo_host::launch;

// *_step.  state: CartSafe's state, SpringPendulum's internal state (its obs may be NULL)
inline int check_step(int n_envs, int max_episode_steps, const void* state, const void* action, const void* ep_len, const void* ep_ret,
                      const void* ep_count, const void* rows, long long cap_steps, const void* stats, int stats_cap) {
    if (n_envs <= 0 || max_episode_steps <= 0) return RPO_ERR_ARG;
    if (!state || !action || !ep_len || !ep_ret || !ep_count) return RPO_ERR_NULL;
    if (rows && cap_steps <= 0) return RPO_ERR_ARG;
    if (stats && stats_cap <= 0) return RPO_ERR_ARG;
    return 0;
}

// *_act_project.  obs_dim: 0 where the projection does not read the observation (CartSafe: obs and obs_stride are not tested)
inline int check_act_project(int n, int max_steps, int noise_mode, int obs_dim, const void* obs, int obs_stride, const void* ap_raw,
                             const void* noise, const void* action, const void* stats, int stats_cap) {
    if (n <= 0 || max_steps < 0 || (obs_dim && obs_stride < obs_dim) || noise_mode < RPO_NOISE_NONE || noise_mode > RPO_NOISE_CLIP_ONLY)
        return RPO_ERR_ARG;
    if ((obs_dim && !obs) || !action || (noise_mode != RPO_NOISE_UNIFORM && !ap_raw)) return RPO_ERR_NULL;
    if (noise_mode == RPO_NOISE_EXPLICIT && !noise) return RPO_ERR_NULL;
    if (stats && stats_cap <= 0) return RPO_ERR_ARG;
    return 0;
}

namespace {

// Sum of G per-workgroup partial vectors [G][8] (K <= 8 used) in a FIXED order: thread t takes workgroups t, t + 256, ..., the 256
// sums meet in an LDS tree; out_k[0] += total_k for the non-NULL outputs.  One workgroup.
__global__ __launch_bounds__(RPO_BLOCK) void lagrangian_reduce_kernel(int G, int K, const float* __restrict__ partials,
                                                                      float* __restrict__ loss_out, float* __restrict__ grad_nu) {
    __shared__ float red[RPO_BLOCK];
    for (int k = 0; k < K; ++k) {
        float acc = 0.0f;
        for (int b = threadIdx.x; b < G; b += RPO_BLOCK) acc += partials[(size_t)b * 8 + k];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int off = RPO_BLOCK / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            float* dst = k == 0 ? loss_out : (grad_nu ? grad_nu + k - 1 : nullptr);
            if (dst) *dst += red[0];
        }
        __syncthreads();
    }
}

}  // namespace

// The launches of *_lagrangian.  kernel: the env's (n, action, nu, scale, loss_out, grad_action, grad_nu, consts..., partials_out),
// which adds its workgroup's K sums (CartSafe 7: the loss and six distances; SpringPendulum 2) into loss_out / grad_nu with float
// atomics, or leaves them in partials_out [G][8].
//
// More than one workgroup would add its partial sums in arrival order (found in round 4: the 2^20-row updates were not bitwise
// reproducible from run to run).  Deterministic form: every workgroup leaves its sums in a scratch area, ONE workgroup adds them
// in a fixed order, then the elementwise launch writes grad_action -- whose first 8 G floats ARE the scratch area: for
// n > RPO_BLOCK, G = rpo_grid_for(n) <= ceil(n / 256), so 8 G <= n / 32 + 8 < 2 n, the floats of grad_action, always.  Without a
// grad_action buffer one workgroup recomputes and sums every row.
template <class... P, class... C>
int launch_lagrangian(void (*kernel)(P...), int K, int n, const float* action, const float* nu, float scale, float* loss_out,
                      float* grad_action, float* grad_nu, void* stream, const C&... consts) {
    float* const none = nullptr;
    const dim3 grid(rpo_grid_for(n));
    if (n <= RPO_BLOCK || (!loss_out && !grad_nu))
        return launch(kernel, grid, RPO_BLOCK, 0, stream, n, action, nu, scale, loss_out, grad_action, grad_nu, consts..., none);
    if (!grad_action) return launch(kernel, dim3(1), RPO_BLOCK, 0, stream, n, action, nu, scale, loss_out, none, grad_nu, consts..., none);
    if (int e = launch(kernel, grid, RPO_BLOCK, 0, stream, n, action, nu, scale, none, none, none, consts..., grad_action)) return e;
    if (int e = launch(lagrangian_reduce_kernel, dim3(1), RPO_BLOCK, 0, stream, (int)grid.x, K, (const float*)grad_action, loss_out, grad_nu))
        return e;
    return launch(kernel, grid, RPO_BLOCK, 0, stream, n, action, nu, scale, none, grad_action, none, consts..., none);
}

}  // namespace rpo_env_glue
