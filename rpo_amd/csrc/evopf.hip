// EVOPF-v0 kernels (reference: rpo/env/electrical_grid/evopf.py, data/demand.py, data/price.py; projection loop of
// rpo/algo/rpo_ddpg.py:72-77,266-305).  One wavefront per env lane / batch row -- see evopf_dev.h.
#include "evopf_dev.h"
#include "heads_dev.h"
#include "launch.h"

using namespace rpo_evopf_dev;
using rpo_host::launch;

namespace {

// Env lanes per workgroup of the one-wave-per-lane kernels: four waves = one on each SIMD of a CU.  As 64-thread workgroups the
// dispatcher packed several waves onto one SIMD while others stayed empty -- and two issue-bound waves on a SIMD run at 3/4 of
// the speed each: the 1024-lane projection took 171 us inside the training windows and 123 us in this form.
constexpr int kActWaves = 4;

// ------------------------------------------------------------------------------------------------------- reset
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_reset_kernel(int n, float* __restrict__ state, int* __restrict__ ep_len,
                                                               float* __restrict__ ep_ret,
                                                               const unsigned* __restrict__ ep_count,
                                                               const float* __restrict__ consts, uint64_t seed,
                                                               uint32_t env_id_base) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    load_consts(w, consts);
    sync();
    episode_obs(w, w.s, seed, env_id_base + (uint32_t)i, ep_count ? ep_count[i] : 0u, 0);
    if (tid < NE) w.s[2 * NB + tid] = kBInit;
    sync();
    for (int k = tid; k < NS; k += RPO_WAVE) state[(size_t)i * NS + k] = w.s[k];
    if (tid == 0) { ep_len[i] = 0; ep_ret[i] = 0.0f; }
}

// -------------------------------------------------------------------------------------------------------- step
// (StepArgs and evopf_step_lane: evopf_dev.h -- the fused evaluation steps its lanes with them too)
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_step_kernel(StepArgs p) {
    __shared__ Ws wss[kActWaves];
    __shared__ __align__(16) float rows_s[kActWaves][RPO_EVOPF_ROW];
    const int wave = threadIdx.x / RPO_WAVE, i = blockIdx.x * kActWaves + wave;
    const long long t = p.ctrl ? p.ctrl[RPO_CTRL_T] : 0;
    if (i < p.n) evopf_step_lane(p, wss[wave], rows_s[wave], i, t);   // (every wave reaches the epilogue's workgroup barrier)
    rpo_step_epilogue(p.ctrl, t, p.stats, p.stats_cap);
}

// ---------------------------------------------------------------------------------------------------- scenarios
// The day lane env_id_base + i is dealt in episode ep_count[i] (NULL: 0), in the table layout: episode_obs itself for every
// hour, so the bits are the ones the reset and the step draw.  Price: the hour-0 window; hours 24..47 are zero.
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_scenario_table_kernel(int n, float* __restrict__ table,
                                                                        const unsigned* __restrict__ ep_count,
                                                                        const float* __restrict__ consts, uint64_t seed,
                                                                        uint32_t env_id_base) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    load_consts(w, consts);
    sync();
    float* day = table + (size_t)i * RPO_EVOPF_SCEN_DAY;
    const unsigned ep = ep_count ? ep_count[i] : 0u;
    for (int t = 0; t < T; ++t) {
        episode_obs(w, w.s, seed, env_id_base + (uint32_t)i, ep, t);
        if (tid < 2 * NB) day[2 * NAHEAD + t * 2 * NB + tid] = w.s[tid];
        if (t == 0 && tid < NAHEAD) { day[tid] = w.s[2 * NB + NE + tid]; day[NAHEAD + tid] = 0.0f; }
        sync();
    }
}

// rpo_evopf_reset from a table: hour 0 of day[i], state of charge kBInit
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_reset_scenario_kernel(int n, float* __restrict__ state, int* __restrict__ ep_len,
                                                                        float* __restrict__ ep_ret, TableDays days) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    scenario_obs(w, w.s, days.table, days.days, days.day[i], 0);
    if (tid < NE) w.s[2 * NB + tid] = kBInit;
    sync();
    for (int k = tid; k < NS; k += RPO_WAVE) state[(size_t)i * NS + k] = w.s[k];
    if (tid == 0) { ep_len[i] = 0; ep_ret[i] = 0.0f; }
}

// evopf_step_kernel with the table as the data source (p.auto_reset = 0: an evaluation seam)
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_step_scenario_kernel(StepArgs p, TableDays days) {
    __shared__ Ws wss[kActWaves];
    __shared__ __align__(16) float rows_s[kActWaves][RPO_EVOPF_ROW];
    const int wave = threadIdx.x / RPO_WAVE, i = blockIdx.x * kActWaves + wave;
    const long long t = p.ctrl ? p.ctrl[RPO_CTRL_T] : 0;
    if (i < p.n) evopf_step_lane(p, wss[wave], rows_s[wave], i, t, days);
    rpo_step_epilogue(p.ctrl, t, p.stats, p.stats_cap);
}

// ------------------------------------------------------------------------------------------------ scenario bank
// Training on the caller's days: the table is a bank, and a lane is dealt a row of it anew for every episode (bank_day,
// evopf_dev.h).  rpo_evopf_reset from the bank: hour 0 of the day dealt for episode ep_count[i] (NULL: 0).
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_reset_bank_kernel(int n, float* __restrict__ state, int* __restrict__ ep_len,
                                                                    float* __restrict__ ep_ret,
                                                                    const unsigned* __restrict__ ep_count, BankDays days,
                                                                    uint64_t seed, uint32_t env_id_base) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    const int day = bank_day(seed, env_id_base + (uint32_t)i, ep_count ? ep_count[i] : 0u, days.days, days.deal, days.stride);
    scenario_obs(w, w.s, days.table, days.days, day, 0);
    if (tid < NE) w.s[2 * NB + tid] = kBInit;
    sync();
    for (int k = tid; k < NS; k += RPO_WAVE) state[(size_t)i * NS + k] = w.s[k];
    if (tid == 0) { ep_len[i] = 0; ep_ret[i] = 0.0f; }
}

// evopf_step_kernel with the bank as the data source; p.auto_reset is the caller's: a finished lane goes on with its next deal
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_step_bank_kernel(StepArgs p, BankDays days) {
    __shared__ Ws wss[kActWaves];
    __shared__ __align__(16) float rows_s[kActWaves][RPO_EVOPF_ROW];
    const int wave = threadIdx.x / RPO_WAVE, i = blockIdx.x * kActWaves + wave;
    const long long t = p.ctrl ? p.ctrl[RPO_CTRL_T] : 0;
    if (i < p.n) evopf_step_lane(p, wss[wave], rows_s[wave], i, t, days);
    rpo_step_epilogue(p.ctrl, t, p.stats, p.stats_cap);
}

// Which day every lane is on: day[i] = bank_day of episode ep_count[i] (NULL: 0).  One thread per lane.
__global__ __launch_bounds__(RPO_BLOCK) void evopf_bank_days_kernel(int n, const unsigned* __restrict__ ep_count, int days, int deal,
                                                                    uint32_t stride, uint64_t seed, uint32_t env_id_base,
                                                                    int* __restrict__ day) {
    for (long long i = (long long)blockIdx.x * RPO_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RPO_BLOCK)
        day[i] = bank_day(seed, env_id_base + (uint32_t)i, ep_count ? ep_count[i] : 0u, days, deal, stride);
}

// ------------------------------------------------------------------------------- explore + complete + project
struct ActArgs {
    int n;
    const float* state;
    int state_stride;
    const float* ap_raw;
    const float* noise;
    float* action;
    int* iters;
    int noise_mode;
    int ap_is_raw;
    float eps_start, eps_end, eps_decay;
    int max_steps;
    float corr_lr, corr_eps, corr_momentum;
    float newton_tol;
    int newton_iters;
    const float* consts;
    uint64_t seed;
    uint32_t env_id_base;
    const long long* ctrl;
    float* stats;
    int stats_cap;
    int place;     // rpo_tuning(RPO_TUNE_EVOPF_PLACE): 0 none; 1 only the workgroups on XCDs 0-1 work; 2 only those on XCDs 2-7
};

// take_action's exploration + clip to the state-dependent box (agent/ddpg_pa.py:101-112, model/utils.py:53-62,90-101,
// EVOPFEnv.update evopf.py:769-783) -> complete_partial -> grad_steps, one lane per wave.
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_act_project_kernel(ActArgs p) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    // A projection of a sampled BATCH (<= 512 rows: the target actions of the critic update, on the iteration's critical path)
    // shares the chip with the 1024-lane projection of the next rollout (one wave per SIMD, the other branch of the window,
    // which has slack): its waves then sit on SIMDs that already hold a wave, and both are bound by instruction issue.  Raised
    // priority gives the batch's waves the issue slots: 171 -> 1xx us measured for it, the rollout's waves on those SIMDs lag.
    int blk = blockIdx.x;
    if (p.place) {                                               // (experiment: block b runs on XCD b % 8 -- observed, not promised)
        const int x = blk & 7, q = blk >> 3;
        if (p.place == 1) { if (x >= 2) return; blk = q * 2 + x; }
        else { if (x < 2) return; blk = q * 6 + (x - 2); }
    }
    if ((p.place ? p.n : (int)gridDim.x * kActWaves) <= 512) __builtin_amdgcn_s_setprio(3);
    const int i = blk * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= p.n) return;                                        // (waves never meet at a workgroup barrier)
    const long long t = p.ctrl ? p.ctrl[RPO_CTRL_T] : 0;
    load_consts(w, p.consts);
    load_row(w.s, p.state + (size_t)i * p.state_stride, NS);
    sync();
    float z = 0.0f;
    if (tid < NP) {
        const float eps_t = fmaxf(p.eps_end, p.eps_start - p.eps_decay * (float)t);
        const uint32_t env_id = p.env_id_base + (uint32_t)i;
        float lo, hi;
        partial_box(w, tid, lo, hi);
        z = (p.noise_mode == RPO_NOISE_UNIFORM) ? 0.0f : p.ap_raw[(size_t)i * NP + tid];
        if (p.ap_is_raw && p.noise_mode != RPO_NOISE_UNIFORM) z = tanh_box_raw(z, lo, hi);
        if (p.noise_mode == RPO_NOISE_EXPLICIT) {
            z = rpo_clamp(z + eps_t * p.noise[(size_t)i * NP + tid], lo, hi);
        } else if (p.noise_mode == RPO_NOISE_PHILOX) {
            const rpo_u4 r = rpo_philox(p.seed, env_id, (uint32_t)t, RPO_STREAM_ACT, (uint32_t)(tid >> 1));
            const float nz = (tid & 1) ? rpo_normal(r.z, r.w) : rpo_normal(r.x, r.y);
            z = rpo_clamp(z + eps_t * nz, lo, hi);
        } else if (p.noise_mode == RPO_NOISE_UNIFORM) {
            const rpo_u4 r = rpo_philox(p.seed, env_id, (uint32_t)t, RPO_STREAM_ACT, (uint32_t)(tid >> 2));
            const uint32_t word = (tid & 3) == 0 ? r.x : ((tid & 3) == 1 ? r.y : ((tid & 3) == 2 ? r.z : r.w));
            const float scale = (hi - lo) * 0.5f;
            z = scale * (2.0f * rpo_u01(word) - 1.0f) + (lo + scale);
        } else if (p.noise_mode == RPO_NOISE_CLIP_ONLY) {
            z = rpo_clamp(z, lo, hi);
        }
    }
    const RowLane L = make_row_lane(w);
    complete_partial_v2(w, L, z, p.newton_tol, p.newton_iters);
    const int k = grad_steps_v2(w, L, p.max_steps, p.corr_lr, p.corr_eps, p.corr_momentum);
    if (tid < NY) p.action[(size_t)i * NY + tid] = w.a[tid];
    if (tid == 0) {
        if (p.iters) p.iters[i] = k;
        if (p.stats && k) atomicAdd(rpo_stats_row(p.stats, p.stats_cap, t) + RPO_STAT_PROJ_ITERS, (float)k);
    }
}

// ------------------------------------------------------------------------------------- complete + project + profile
struct ProfileArgs {
    int n;
    const float* state;
    int state_stride;
    const float* ap_raw;
    int ap_is_raw;
    float* action;
    int* iters;
    int max_steps;
    float corr_lr, corr_eps, corr_momentum;
    float newton_tol;
    int newton_iters;
    const float* consts;
    float* profile;               // [max_steps + 1, n, 4], 16-byte aligned
};

// evopf_act_project_kernel under RPO_NOISE_NONE (no clamp, no generator, no clock, no statistics, no placement, no raised
// priority) that also writes the row's projection profile: plane b, row i of profile = (a[0], a[1], eq*, ineq*) of the iterate
// after min(b, iters[i]) GRG iterations (evopf_dev.h: profile_entry, grad_steps_profile_v2).  The same geometry: one lane per
// wave, a workspace each, and the waves never meet at a workgroup barrier.  The residual pass between two iterations may
// clobber w.cs, w.sn, w.vr, w.vi, w.t1, w.t2, w.eq and w.ineq: the v2 solver and GRG iteration read none of them (they keep
// w.a, w.old, w.c, w.s and the RowLane; w.vec and w.fp are rewritten before use, with static pivots and in the fallback).
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_project_profile_kernel(ProfileArgs p) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= p.n) return;                                        // (waves never meet at a workgroup barrier)
    load_consts(w, p.consts);
    load_row(w.s, p.state + (size_t)i * p.state_stride, NS);
    sync();
    float z = 0.0f;
    if (tid < NP) {
        float lo, hi;
        partial_box(w, tid, lo, hi);
        z = p.ap_raw[(size_t)i * NP + tid];
        if (p.ap_is_raw) z = tanh_box_raw(z, lo, hi);
    }
    const RowLane L = make_row_lane(w);
    complete_partial_v2(w, L, z, p.newton_tol, p.newton_iters);
    const int k = grad_steps_profile_v2(w, L, p.max_steps, p.corr_lr, p.corr_eps, p.corr_momentum, p.profile + (size_t)i * 4,
                                        (size_t)p.n * 4);
    if (tid < NY) p.action[(size_t)i * NY + tid] = w.a[tid];
    if (tid == 0 && p.iters) p.iters[i] = k;
}

// PFFunction.backward (evopf.py:857-910) with the Jacobians re-evaluated at the completed action (the reference keeps
// those of the last Newton point, one update of size < tol earlier).  grad_ap [n,14] = dL/dz.
__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_complete_bwd_kernel(int n, const float* __restrict__ action,
                                                                      const float* __restrict__ grad_action,
                                                                      const float* __restrict__ grad_action_b,
                                                                      const float* __restrict__ grad_action2,
                                                                      float* __restrict__ grad_ap,
                                                                      const float* __restrict__ consts) {
    RPO_FP_STRICT
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    load_consts(w, consts);
    load_row(w.a, action + (size_t)i * NY, NY);
    // dl_dy = (grad_action [+ grad_action_b]) [+ grad_action2]: d(-Q)/da from the critic (twin critics: the two terms) + the
    // Lagrangian term, rpo_ddpg.py:319 / rpo_sac.py:331-337, added here instead of by launches of their own -- the same float
    // additions in the same order
    for (int j = tid; j < NY; j += RPO_WAVE) {
        float v = grad_action[(size_t)i * NY + j];
        if (grad_action_b) v = v + grad_action_b[(size_t)i * NY + j];
        if (grad_action2) v = v + grad_action2[(size_t)i * NY + j];
        w.dir[j] = v;
    }
    sync();
    flows(w);
    // step 3 (:865-880): dl/d(vm, va) through pg_slack = -eq[0] and qg_j = -eq[14 + spv_j]
    if (tid < 2 * NB) {
        float acc = jac_entry(w, 0, VM0 + tid) * w.dir[PG0];
        for (int j = 0; j < NG; ++j) acc += jac_entry(w, NB + kSpv[j], VM0 + tid) * w.dir[QG0 + j];
        w.vec[tid] = w.dir[VM0 + tid] - acc;                            // dl_dy_total on the voltage block (:886)
    }
    sync();
    // step 1 (:889-891): d_int = inv(J_newton)^T dl_dy_total[newton vars]
    const bool force_dyn = w.c[RPO_EVOPF_C_FLAGS] != RPO_EVOPF_STATIC_OK;
    // (the row is written out in both branches: built by one helper function or lambda, the gradient came out with other last
    //  bits on the device -- the kernel is then 4.7 KB shorter, the second build reuses values of the first; no further cause found)
    bool solved = false;
    float num = 0.0f, piv = 1.0f;                                       // d_int = num / piv of the unknown `mycol`
    int mycol = tid;
    if (!force_dyn) {                                                   // static order (evopf_dev.h), accepted by its pivots
        float row[NN + 1];                                              // row tid of [J_newton^T | rhs]
#pragma unroll
        for (int c = 0; c < NN; ++c) row[c] = tid < NN ? jac_entry(w, kKeep[c], kNewtonVars[tid]) : 0.0f;
        row[NN] = tid < NN ? w.vec[kNewtonVars[tid] - VM0] : 0.0f;
        piv = gj_static<0, NN, 0, 0, NN + 1, TabNewtonT, true>(row);    // (with the exact reciprocal)
        solved = pivots_ok<NN, 0>(piv);
        num = row[NN];
    }
    if (!solved) {                                                      // partial pivoting
        float row[NN + 1];
#pragma unroll
        for (int c = 0; c < NN; ++c) row[c] = tid < NN ? jac_entry(w, kKeep[c], kNewtonVars[tid]) : 0.0f;
        row[NN] = tid < NN ? w.vec[kNewtonVars[tid] - VM0] : 0.0f;
        piv = gj_dynamic<0, NN, 0, NN + 1>(row, mycol);
        num = row[NN];
    }
    const float dint = num / piv;
    sync();
    if (tid < NN) w.old[mycol] = dint;                                  // d_int, indexed like kKeep
    sync();
    if (tid < NP) {
        float g;
        if (tid < 4) {                                                  // pg at pv gens (:894) + direct term (:907)
            g = -w.old[kPvPos[tid]] + w.dir[PG0 + 1 + tid];
        } else if (tid < 9) {                                           // vm at generator buses (:895-896)
            const int var = VM0 + kSpv[tid - 4];
            float acc = 0.0f;
            for (int r = 0; r < NN; ++r) acc += jac_entry(w, kKeep[r], var) * w.old[r];
            g = -acc + w.vec[var - VM0];
        } else if (tid == 9) {                                          // pe at the slack generator (:898)
            g = w.dir[PG0] + w.dir[PE0];
        } else {                                                        // pe at pv gens (:897)
            g = w.old[kPvPos[tid - 10]] + w.dir[PE0 + tid - 9];
        }
        grad_ap[(size_t)i * NP + tid] = g;
    }
}

__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_resid_kernel(int n, const float* __restrict__ state, int state_stride,
                                                               const float* __restrict__ action, float* __restrict__ eq_out,
                                                               float* __restrict__ ineq_out,
                                                               const float* __restrict__ consts) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    load_consts(w, consts);
    load_row(w.s, state + (size_t)i * state_stride, NS);
    load_row(w.a, action + (size_t)i * NY, NY);
    sync();
    flows(w);
    eq_resid(w);
    ineq_resid(w);
    if (eq_out && tid < NEQ) eq_out[(size_t)i * NEQ + tid] = w.eq[tid];
    if (ineq_out && tid < NINEQ) ineq_out[(size_t)i * NINEQ + tid] = w.ineq[tid];
}

__global__ __launch_bounds__(RPO_WAVE * kActWaves) void evopf_ipg_kernel(int n, const float* __restrict__ state, int state_stride,
                                                             const float* __restrict__ action, float* __restrict__ step_out,
                                                             const float* __restrict__ consts) {
    __shared__ Ws wss[kActWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kActWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= n) return;
    load_consts(w, consts);
    load_row(w.s, state + (size_t)i * state_stride, NS);
    load_row(w.a, action + (size_t)i * NY, NY);
    sync();
    if (tid < NY) w.dir[tid] = 0.0f;                           // (all 43 components are written below: 28 others + 15 partial vars)
    sync();
    const RowLane L = make_row_lane(w);
    sync();
    grg_iteration_v2(w, L, true, 0.0f, 0.0f, 0.0f, false, w.dir);
    if (tid < NY) step_out[(size_t)i * NY + tid] = w.dir[tid];
}

// Vector-Jacobian product of eq_resid: out[v] = sum_r grad_eq[r] * d eq_resid[r] / d action[v] with the entries of
// eq_jac (evopf.py:614-661) -- what torch autograd computes through eq_resid (:520-546) in the Lagrangian baselines'
// actor loss (ddpg_lag.py:257-263), except for the battery columns, where autograd differentiates the +pe of the
// residual (:532) while eq_jac carries -I (hazard E1): `autograd_sign` != 0 flips them to the autograd value.
__global__ __launch_bounds__(RPO_WAVE) void evopf_eq_vjp_kernel(int n, const float* __restrict__ action,
                                                                const float* __restrict__ grad_eq, float* __restrict__ out,
                                                                int autograd_sign, const float* __restrict__ consts) {
    __shared__ Ws w;
    const int i = blockIdx.x, tid = threadIdx.x;
    load_consts(w, consts);
    load_row(w.a, action + (size_t)i * NY, NY);
    load_row(w.eq, grad_eq + (size_t)i * NEQ, NEQ);
    sync();
    flows(w);
    if (tid < NY) {
        float acc = 0.0f;
        for (int r = 0; r < NEQ; ++r) acc = fmaf(w.eq[r], jac_entry(w, r, tid), acc);
        if (autograd_sign && tid >= PE0) acc = -acc;
        out[(size_t)i * NY + tid] = acc;
    }
}

// mean_b sum_j nu_j relu(g_j(s_b, a_b)) with its gradients (Dual.forward dual.py:63-65 on ineq_dist, rpo_ddpg.py:312-319).
// The 58 inequalities are box bounds on single variables, so the work is elementwise: thread v of each of the 4 waves owns
// action component v (its upper and its lower bound) for the rows b = wave (mod 4); the four partial sums are combined in
// a fixed order by wave 0 -- one workgroup, no float atomics between workgroups, bitwise reproducible.
__global__ __launch_bounds__(RPO_BLOCK) void evopf_lagrangian_kernel(int n, const float* __restrict__ state, int state_stride,
                                                                     const float* __restrict__ action,
                                                                     const float* __restrict__ nu, float scale,
                                                                     float* __restrict__ loss_out,
                                                                     float* __restrict__ grad_action,
                                                                     float* __restrict__ grad_nu,
                                                                     const float* __restrict__ consts, int overwrite) {
    RPO_FP_STRICT
    __shared__ float red[RPO_BLOCK / RPO_WAVE][2 * RPO_WAVE];
    const int v = threadIdx.x & (RPO_WAVE - 1), q = threadIdx.x / RPO_WAVE;
    int up = -1, lo = -1;                                        // rows of ineq_resid (evopf.py:550-561) bounding component v
    float hi_b = 0.0f, lo_b = 0.0f;
    if (v < QG0) { up = v; lo = 5 + v; hi_b = consts[RPO_EVOPF_C_PMAX + v]; lo_b = consts[RPO_EVOPF_C_PMIN + v]; }
    else if (v < VM0) { up = 10 + v - QG0; lo = 15 + v - QG0; hi_b = consts[RPO_EVOPF_C_QMAX + v - QG0]; lo_b = consts[RPO_EVOPF_C_QMIN + v - QG0]; }
    else if (v < VA0) { up = 20 + v - VM0; lo = 34 + v - VM0; hi_b = consts[RPO_EVOPF_C_VMAX + v - VM0]; lo_b = consts[RPO_EVOPF_C_VMIN + v - VM0]; }
    else if (v >= PE0 && v < NY) { up = 48 + v - PE0; lo = 53 + v - PE0; }
    const float nu_up = up >= 0 ? nu[up] : 0.0f, nu_lo = lo >= 0 ? nu[lo] : 0.0f;
    float acc_up = 0.0f, acc_lo = 0.0f;
    if (v < NY) {
        // 64 rows of loads in flight (a whole batch of 256 in one round trip), then the rows in order (the sums keep their association; one dependent round trip per
        // row made this one-workgroup launch 25 us at batch 256)
        constexpr int W = RPO_BLOCK / RPO_WAVE, CH = 64;
        for (int b0 = q; b0 < n; b0 += W * CH) {
            float av[CH], sv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int b = b0 + u * W, bc = b < n ? b : n - 1;
                av[u] = up >= 0 ? action[(size_t)bc * NY + v] : 0.0f;
                sv[u] = v >= PE0 ? state[(size_t)bc * state_stride + 2 * NB + v - PE0] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int b = b0 + u * W;
                if (b < n) {
                    float g = 0.0f;
                    if (up >= 0) {
                        const float a = av[u];
                        if (v >= PE0) battery_bounds(sv[u], hi_b, lo_b);
                        const float ru = a - hi_b, rl = lo_b - a;
                        acc_up += fmaxf(ru, 0.0f);
                        acc_lo += fmaxf(rl, 0.0f);
                        g = (ru > 0.0f ? nu_up : 0.0f) - (rl > 0.0f ? nu_lo : 0.0f);      // ineq_jac^T (nu * 1[g > 0]), :663-707
                    }
                    if (grad_action) grad_action[(size_t)b * NY + v] = scale * g;
                }
            }
        }
    }
    red[q][v] = acc_up;
    red[q][RPO_WAVE + v] = acc_lo;
    __syncthreads();
    if (q == 0) {
        float su = 0.0f, sl = 0.0f;
        for (int w = 0; w < RPO_BLOCK / RPO_WAVE; ++w) { su += red[w][v]; sl += red[w][RPO_WAVE + v]; }
        if (grad_nu && up >= 0) { grad_nu[up] += scale * su; grad_nu[lo] += scale * sl; }   // one writer per address
        const float total = rpo_wave_sum(nu_up * su + nu_lo * sl);
        if (v == 0 && loss_out) *loss_out = overwrite ? 0.0f + scale * total : *loss_out + scale * total;
    }
}

// Box of basic action j of row i straight from global memory (EVOPFEnv.update, evopf.py:769-783)
__device__ __forceinline__ void row_box(const float* __restrict__ state, int state_stride, const float* __restrict__ consts,
                                        int i, int j, float& lo, float& hi) {
    basic_box(consts, state + (size_t)i * state_stride + 2 * NB, j, lo, hi);
}

// Squashed-Gaussian policy head with the state-dependent box (GaussianSharedPolicy.forward, model/policy.py:53-66, with
// BoxConstraint.update_box; PDSAC_PA.take_action's clip, agent/sac_pa.py:111): raw [n,28] = (mean[14] | log-std[14]),
// eps [n,14] -> ap [n,14], logp [n] = sum over the 14 dimensions.  One 16-lane group per row.
__global__ __launch_bounds__(RPO_BLOCK) void evopf_gauss_head_kernel(int n, const float* __restrict__ state, int state_stride,
                                                                     const float* __restrict__ raw,
                                                                     const float* __restrict__ eps, int deterministic,
                                                                     float* __restrict__ ap, float* __restrict__ logp,
                                                                     const float* __restrict__ consts) {
    const int j = threadIdx.x & 15;
    for (int i = blockIdx.x * (RPO_BLOCK / 16) + (threadIdx.x >> 4); i < n; i += gridDim.x * (RPO_BLOCK / 16)) {
        float lp = 0.0f;
        if (j < NP) {
            float lo, hi;
            row_box(state, state_stride, consts, i, j, lo, hi);
            const float scale = (hi - lo) * 0.5f;
            ap[(size_t)i * NP + j] = rpo_head_dev::gauss_head_row(raw[(size_t)i * 2 * NP + j], raw[(size_t)i * 2 * NP + NP + j],
                                                                  eps[(size_t)i * NP + j], scale, lo + scale, lo, hi,
                                                                  deterministic, &lp);
        }
        lp += __shfl_xor(lp, 1, 16); lp += __shfl_xor(lp, 2, 16); lp += __shfl_xor(lp, 4, 16); lp += __shfl_xor(lp, 8, 16);
        if (j == 0 && logp) logp[i] = lp;
    }
}

// its backward: draw [n,28] = d loss / d (mean | log-std heads) given dap [n,14] and the coefficient of log pi
__global__ __launch_bounds__(RPO_BLOCK) void evopf_gauss_head_bwd_kernel(int n, const float* __restrict__ state,
                                                                         int state_stride, const float* __restrict__ raw,
                                                                         const float* __restrict__ eps,
                                                                         const float* __restrict__ dap, float dlogp,
                                                                         float* __restrict__ draw,
                                                                         const float* __restrict__ consts) {
    for (int idx = blockIdx.x * RPO_BLOCK + threadIdx.x; idx < n * NP; idx += gridDim.x * RPO_BLOCK) {
        const int i = idx / NP, j = idx - i * NP;
        float lo, hi;
        row_box(state, state_stride, consts, i, j, lo, hi);
        const float scale = (hi - lo) * 0.5f;
        const float2 g = rpo_head_dev::gauss_head_bwd_row(raw[(size_t)i * 2 * NP + j], raw[(size_t)i * 2 * NP + NP + j], eps[idx],
                                                          dap[idx], dlogp, scale, lo + scale, lo, hi);
        draw[(size_t)i * 2 * NP + j] = g.x;
        draw[(size_t)i * 2 * NP + NP + j] = g.y;
    }
}

// d/d(raw) of ap = clip(scale(s) * tanh(raw) + base(s) + eps_t * noise, lo(s), hi(s)) (SharedPolicy.forward
// model/policy.py:24-33 with the volatile box of evopf.py:769-783, then take_action ddpg_pa.py:108-110); elementwise.
__global__ __launch_bounds__(RPO_BLOCK) void evopf_tanh_box_bwd_kernel(int n, const float* __restrict__ state,
                                                                       int state_stride, const float* __restrict__ raw,
                                                                       const float* __restrict__ noise, float eps_start,
                                                                       float eps_end, float eps_decay,
                                                                       const long long* __restrict__ ctrl,
                                                                       const float* __restrict__ dap,
                                                                       float* __restrict__ dout,
                                                                       const float* __restrict__ consts) {
    RPO_FP_STRICT
    const long long t = ctrl ? ctrl[RPO_CTRL_T] : 0;
    const float eps_t = fmaxf(eps_end, eps_start - eps_decay * (float)t);
    for (int idx = blockIdx.x * RPO_BLOCK + threadIdx.x; idx < n * NP; idx += gridDim.x * RPO_BLOCK) {
        const int i = idx / NP, j = idx - i * NP;
        float lo, hi;
        row_box(state, state_stride, consts, i, j, lo, hi);
        const float scale = (hi - lo) * 0.5f;
        const float th = tanhf(raw[idx]);
        float g = dap[idx] * scale * (1.0f - th * th);
        if (noise) {
            const float pre = scale * th + (lo + scale) + eps_t * noise[idx];
            if (pre < lo || pre > hi) g = 0.0f;                      // torch.clip's backward: zero outside [lo, hi]
        }
        dout[idx] = g;
    }
}

// the grid and workgroup of the one-wave-per-lane kernels
constexpr int kActThreads = RPO_WAVE * kActWaves;
dim3 lane_grid(int n) { return dim3((n + kActWaves - 1) / kActWaves); }

int check_common(int n, const void* a, const void* b, const float* consts) {
    if (n <= 0) return RPO_ERR_ARG;
    if (!a || !b || !consts) return RPO_ERR_NULL;
    return 0;
}

// a bank's words: days >= 1, deal 0 "uniform" or 1 "cycle", and a stride >= 1 for the cycle (bank_day divides by days)
int check_deal(int days, int deal, int stride) {
    if (days < 1 || deal < RPO_EVOPF_DEAL_UNIFORM || deal > RPO_EVOPF_DEAL_CYCLE) return RPO_ERR_ARG;
    if (deal == RPO_EVOPF_DEAL_CYCLE && stride < 1) return RPO_ERR_ARG;
    return 0;
}
int check_bank(const float* table, int days, int deal, int stride) { return table ? check_deal(days, deal, stride) : RPO_ERR_NULL; }

}  // namespace

// ====================================================================================================== C ABI
extern "C" {

int rpo_evopf_reset(int n_envs, float* state, int* ep_len, float* ep_ret, const unsigned* ep_count,
                    const float* consts_dev, unsigned long long seed, unsigned env_id_base, void* stream) {
    if (int e = check_common(n_envs, state, ep_len, consts_dev)) return e;
    if (!ep_ret) return RPO_ERR_NULL;
    return launch(evopf_reset_kernel, lane_grid(n_envs), kActThreads, 0, stream, n_envs, state, ep_len, ep_ret, ep_count, consts_dev,
                  (uint64_t)seed, (uint32_t)env_id_base);
}

int rpo_evopf_step(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count,
                   float* rows, long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps,
                   int auto_reset, float viol_thresh, const float* consts_dev, unsigned long long seed,
                   unsigned env_id_base, void* stream) {
    if (int e = check_common(n_envs, state, action, consts_dev)) return e;
    if (!ep_len || !ep_ret || !ep_count) return RPO_ERR_NULL;
    if (max_episode_steps <= 0 || (rows && cap_steps <= 0) || (stats && stats_cap <= 0)) return RPO_ERR_ARG;
    StepArgs p{n_envs, state, action, ep_len, ep_ret, ep_count, rows, cap_steps, stats, stats_cap, ctrl, max_episode_steps,
               auto_reset, viol_thresh, consts_dev, (uint64_t)seed, (uint32_t)env_id_base};
    return launch(evopf_step_kernel, lane_grid(n_envs), kActThreads, 0, stream, p);
}

int rpo_evopf_scenario_table(int n, float* table_out, const unsigned* ep_count, const float* consts_dev, unsigned long long seed,
                             unsigned env_id_base, void* stream) {
    if (n <= 0) return RPO_ERR_ARG;
    if (!table_out || !consts_dev) return RPO_ERR_NULL;
    return launch(evopf_scenario_table_kernel, lane_grid(n), kActThreads, 0, stream, n, table_out, ep_count, consts_dev, (uint64_t)seed,
                  (uint32_t)env_id_base);
}

int rpo_evopf_reset_scenario(int n_envs, float* state, int* ep_len, float* ep_ret, const float* table, int days, const int* day,
                             const float* consts_dev, void* stream) {
    if (int e = check_common(n_envs, state, ep_len, consts_dev)) return e;
    if (days <= 0) return RPO_ERR_ARG;
    if (!ep_ret || !table || !day) return RPO_ERR_NULL;
    return launch(evopf_reset_scenario_kernel, lane_grid(n_envs), kActThreads, 0, stream, n_envs, state, ep_len, ep_ret,
                  TableDays{table, days, day});
}

int rpo_evopf_step_scenario(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count,
                            float* rows, long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps,
                            float viol_thresh, const float* consts_dev, const float* table, int days, const int* day, void* stream) {
    if (int e = check_common(n_envs, state, action, consts_dev)) return e;
    if (days <= 0) return RPO_ERR_ARG;
    if (!ep_len || !ep_ret || !ep_count || !table || !day) return RPO_ERR_NULL;
    if (max_episode_steps <= 0 || (rows && cap_steps <= 0) || (stats && stats_cap <= 0)) return RPO_ERR_ARG;
    StepArgs p{n_envs, state, action, ep_len, ep_ret, ep_count, rows, cap_steps, stats, stats_cap, ctrl, max_episode_steps,
               0, viol_thresh, consts_dev, 0ull, 0u};
    return launch(evopf_step_scenario_kernel, lane_grid(n_envs), kActThreads, 0, stream, p, TableDays{table, days, day});
}

int rpo_evopf_reset_bank(int n_envs, float* state, int* ep_len, float* ep_ret, const unsigned* ep_count, const float* table, int days,
                         int deal, int stride, unsigned long long seed, unsigned env_id_base, void* stream) {
    if (n_envs <= 0) return RPO_ERR_ARG;
    if (!state || !ep_len || !ep_ret) return RPO_ERR_NULL;
    if (int e = check_bank(table, days, deal, stride)) return e;
    return launch(evopf_reset_bank_kernel, lane_grid(n_envs), kActThreads, 0, stream, n_envs, state, ep_len, ep_ret, ep_count,
                  BankDays{table, days, deal, (uint32_t)stride}, (uint64_t)seed, (uint32_t)env_id_base);
}

int rpo_evopf_step_bank(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count, float* rows,
                        long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps, int auto_reset,
                        float viol_thresh, const float* consts_dev, unsigned long long seed, unsigned env_id_base, const float* table,
                        int days, int deal, int stride, void* stream) {
    if (int e = check_common(n_envs, state, action, consts_dev)) return e;
    if (!ep_len || !ep_ret || !ep_count) return RPO_ERR_NULL;
    if (int e = check_bank(table, days, deal, stride)) return e;
    if (max_episode_steps <= 0 || (rows && cap_steps <= 0) || (stats && stats_cap <= 0)) return RPO_ERR_ARG;
    StepArgs p{n_envs, state, action, ep_len, ep_ret, ep_count, rows, cap_steps, stats, stats_cap, ctrl, max_episode_steps,
               auto_reset, viol_thresh, consts_dev, (uint64_t)seed, (uint32_t)env_id_base};
    return launch(evopf_step_bank_kernel, lane_grid(n_envs), kActThreads, 0, stream, p, BankDays{table, days, deal, (uint32_t)stride});
}

int rpo_evopf_bank_days(int n, const unsigned* ep_count, int days, int deal, int stride, unsigned long long seed, unsigned env_id_base,
                        int* day_out, void* stream) {
    if (n <= 0) return RPO_ERR_ARG;
    if (!day_out) return RPO_ERR_NULL;
    if (int e = check_deal(days, deal, stride)) return e;
    return launch(evopf_bank_days_kernel, dim3(rpo_grid_for(n)), RPO_BLOCK, 0, stream, n, ep_count, days, deal, (uint32_t)stride,
                  (uint64_t)seed, (uint32_t)env_id_base, day_out);
}

int rpo_evopf_act_project(int n, const float* state, int state_stride, const float* ap_raw, const float* noise, float* action, int* iters,
                          int noise_mode, int ap_is_raw, float eps_start, float eps_end, float eps_decay, int max_steps,
                          float corr_lr, float corr_eps, float corr_momentum, float newton_tol, int newton_max_iters,
                          const float* consts_dev, unsigned long long seed, unsigned env_id_base, const long long* ctrl,
                          float* stats, int stats_cap, void* stream) {
    if (int e = check_common(n, state, action, consts_dev)) return e;
    if (max_steps < 0 || newton_max_iters <= 0 || (stats && stats_cap <= 0)) return RPO_ERR_ARG;
    if (noise_mode < RPO_NOISE_NONE || noise_mode > RPO_NOISE_CLIP_ONLY) return RPO_ERR_ARG;
    if (noise_mode != RPO_NOISE_UNIFORM && !ap_raw) return RPO_ERR_NULL;
    if (noise_mode == RPO_NOISE_EXPLICIT && !noise) return RPO_ERR_NULL;
    if (state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    ActArgs p{n, state, state_stride, ap_raw, noise, action, iters, noise_mode, ap_is_raw, eps_start, eps_end, eps_decay, max_steps, corr_lr,
              corr_eps, corr_momentum, newton_tol, newton_max_iters, consts_dev, (uint64_t)seed, (uint32_t)env_id_base, ctrl,
              stats, stats_cap, 0};
    int blocks = (n + kActWaves - 1) / kActWaves;
    if (rpo_tune(RPO_TUNE_EVOPF_PLACE)) {
        p.place = n <= 512 ? 1 : 2;
        const int per = p.place == 1 ? 2 : 6;
        blocks = (blocks + per - 1) / per * 8;
    }
    return launch(evopf_act_project_kernel, dim3(blocks), kActThreads, 0, stream, p);
}

int rpo_evopf_project_profile(int n, const float* state, int state_stride, const float* ap_raw, int ap_is_raw, float* action, int* iters,
                              int max_steps, float corr_lr, float corr_eps, float corr_momentum, float newton_tol, int newton_max_iters,
                              const float* consts_dev, float* profile, void* stream) {
    if (n <= 0 || max_steps < 0 || newton_max_iters <= 0 || state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    if (!state || !ap_raw || !action || !consts_dev || !profile) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(profile) % 16) return RPO_ERR_ARG;                       // (written with 16-byte stores)
    if (16ll * ((long long)max_steps + 1) * (long long)n > (long long)RPO_TRACE_MAX_BYTES) return RPO_ERR_ARG;
    ProfileArgs p{n, state, state_stride, ap_raw, ap_is_raw, action, iters, max_steps, corr_lr, corr_eps, corr_momentum, newton_tol,
                  newton_max_iters, consts_dev, profile};
    return launch(evopf_project_profile_kernel, lane_grid(n), kActThreads, 0, stream, p);
}

int rpo_evopf_tanh_box_bwd(int n, const float* state, int state_stride, const float* raw, const float* noise,
                           float eps_start, float eps_end, float eps_decay, const long long* ctrl, const float* dap,
                           float* dout, const float* consts_dev, void* stream) {
    if (int e = check_common(n, state, raw, consts_dev)) return e;
    if (!dap || !dout) return RPO_ERR_NULL;
    if (state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    return launch(evopf_tanh_box_bwd_kernel, dim3(rpo_grid_for((long long)n * NP)), RPO_BLOCK, 0, stream, n, state, state_stride, raw,
                  noise, eps_start, eps_end, eps_decay, ctrl, dap, dout, consts_dev);
}

int rpo_evopf_gauss_head(int n, const float* state, int state_stride, const float* raw, const float* eps, int deterministic,
                         float* ap_out, float* logp_out, const float* consts_dev, void* stream) {
    if (int e = check_common(n, state, raw, consts_dev)) return e;
    if (!eps || !ap_out) return RPO_ERR_NULL;
    if (state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    return launch(evopf_gauss_head_kernel, dim3(rpo_grid_for((long long)n * 16)), RPO_BLOCK, 0, stream, n, state, state_stride, raw,
                  eps, deterministic, ap_out, logp_out, consts_dev);
}

int rpo_evopf_gauss_head_bwd(int n, const float* state, int state_stride, const float* raw, const float* eps,
                             const float* dap, float dlogp, float* draw, const float* consts_dev, void* stream) {
    if (int e = check_common(n, state, raw, consts_dev)) return e;
    if (!eps || !dap || !draw) return RPO_ERR_NULL;
    if (state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    return launch(evopf_gauss_head_bwd_kernel, dim3(rpo_grid_for((long long)n * NP)), RPO_BLOCK, 0, stream, n, state, state_stride,
                  raw, eps, dap, dlogp, draw, consts_dev);
}

int rpo_evopf_complete_bwd(int n, const float* action, const float* grad_action, const float* grad_action_b, const float* grad_action2,
                           float* grad_ap, const float* consts_dev, void* stream) {
    if (int e = check_common(n, action, grad_action, consts_dev)) return e;
    if (!grad_ap) return RPO_ERR_NULL;
    return launch(evopf_complete_bwd_kernel, lane_grid(n), kActThreads, 0, stream, n, action, grad_action, grad_action_b, grad_action2,
                  grad_ap, consts_dev);
}

int rpo_evopf_resid(int n, const float* state, int state_stride, const float* action, float* eq_out, float* ineq_out,
                    const float* consts_dev, void* stream) {
    if (int e = check_common(n, state, action, consts_dev)) return e;
    return launch(evopf_resid_kernel, lane_grid(n), kActThreads, 0, stream, n, state, state_stride, action, eq_out, ineq_out,
                  consts_dev);
}

int rpo_evopf_ineq_partial_grad(int n, const float* state, int state_stride, const float* action, float* step_out, const float* consts_dev,
                                void* stream) {
    if (int e = check_common(n, state, action, consts_dev)) return e;
    if (!step_out) return RPO_ERR_NULL;
    return launch(evopf_ipg_kernel, lane_grid(n), kActThreads, 0, stream, n, state, state_stride, action, step_out, consts_dev);
}

int rpo_evopf_eq_vjp(int n, const float* action, const float* grad_eq, float* grad_action, int autograd_sign,
                     const float* consts_dev, void* stream) {
    if (int e = check_common(n, action, grad_eq, consts_dev)) return e;
    if (!grad_action) return RPO_ERR_NULL;
    return launch(evopf_eq_vjp_kernel, dim3(n), RPO_WAVE, 0, stream, n, action, grad_eq, grad_action, autograd_sign, consts_dev);
}

int rpo_evopf_lagrangian(int n, const float* state, int state_stride, const float* action, const float* nu, float scale, float* loss_out,
                         float* grad_action, float* grad_nu, const float* consts_dev, int overwrite, void* stream) {
    if (int e = check_common(n, state, action, consts_dev)) return e;
    if (!nu) return RPO_ERR_NULL;
    return launch(evopf_lagrangian_kernel, dim3(1), RPO_BLOCK, 0, stream, n, state, state_stride, action, nu, scale, loss_out,
                  grad_action, grad_nu, consts_dev, overwrite);
}

}  // extern "C"
