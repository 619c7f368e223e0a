// Per-episode statistics of trainer.evaluate(): one device function shared by the fused evaluation kernel and the
// stepwise path's rpo_eval_accumulate (evaluate.hip), so that both paths have one definition of the statistics.
#pragma once
#include "common.h"

namespace rpo_eval_dev {

// torch.maximum / Tensor.max(dim): a NaN operand propagates (fmaxf would drop it)
__device__ __forceinline__ float nanmax(float a, float b) {
    return a != a ? a : (b != b ? b : (b > a ? b : a));
}

// the step's max inequality violation / max |equality residual| of a transition row, columns in order (the stepwise path's
// kernels read the row rpo_<env>_step wrote; the fused EVOPF evaluation the row its lane keeps in LDS)
__device__ __forceinline__ void row_violations(const float* r, int ineq_col, int ineq_num, int eq_col, int eq_num, float& ineq,
                                               float& eq) {
    ineq = r[ineq_col];
    eq = fabsf(r[eq_col]);
    for (int j = 1; j < ineq_num; ++j) ineq = nanmax(ineq, r[ineq_col + j]);
    for (int j = 1; j < eq_num; ++j) eq = nanmax(eq, fabsf(r[eq_col + j]));
}

// One env step of one lane into its accumulator row acc[RPO_EVAL_LEN] (include/rpo_hip.h: RPO_EVAL_*), with the arithmetic
// of RPOTrainerBase.eval() in its order: `step` is the 0-based step index of the evaluation (every lane starts at 0; step 0
// initialises the row), `ineq` / `eq` the step's max inequality violation / max |equality residual|.  A lane that is no
// longer alive keeps its row.  The running means multiply by the f32 reciprocal of (step + 1): that is what torch's GPU
// kernel for `tensor / python_int` computes (a * (1 / b)), which eval()'s `(x - m) / (i + 1)` runs through.
__device__ __forceinline__ void rpo_eval_lane_update(float* __restrict__ acc, int step, float reward, float ineq, float eq,
                                                     float done, int iters, float viol_thresh) {
    RPO_FP_STRICT
    float4* a4 = reinterpret_cast<float4*>(acc);
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int word = RPO_EVAL_ALIVE;
    if (step > 0) {
        lo = a4[0];
        hi = a4[1];
        word = __float_as_int(hi.w);
        if (!(word & RPO_EVAL_ALIVE)) return;
    }
    const float inv = 1.0f / (float)(step + 1);
    lo.x = lo.x + reward;                                        // ret
    lo.y = lo.y + (ineq - lo.y) * inv;                           // mean_ineq
    lo.z = lo.z + (eq - lo.z) * inv;                             // mean_eq
    lo.w = nanmax(lo.w, ineq);                                   // max_ineq
    hi.x = nanmax(hi.x, eq);                                     // max_eq
    hi.y = hi.y + ((ineq > viol_thresh) ? 1.0f : 0.0f);          // viol_steps
    hi.z = hi.z + (float)iters;                                  // proj_iters
    const bool bad = !__builtin_isfinite(reward) || !__builtin_isfinite(ineq) || !__builtin_isfinite(eq);
    word += 1 << RPO_EVAL_LEN_SHIFT;                             // length
    if (bad) word |= RPO_EVAL_NONFINITE;
    if (done != 0.0f) word &= ~RPO_EVAL_ALIVE;
    hi.w = __int_as_float(word);
    a4[0] = lo;
    a4[1] = hi;
}

// ------------------------------------------------------------------------------------------------ observation noise
// evaluate(obs_noise=): ONE definition of the perturbed observation for the fused kernel's NOISE = 1 instances and
// rpo_eval_obs_noise.  Column q of episode i at the evaluation's absolute step: o + sigma * z, z = the normal of
// rpo_philox_normal(seed, id_base 0, salt step, RPO_STREAM_EVAL_OBS + 0x100 * q) -- the reset's idiom for further blocks of
// one stream -- as an f32 multiply and an f32 add (torch's obs + sigma * z).  sigma == 0: not drawn, the bits of o.
__device__ __forceinline__ float rpo_eval_noisy_obs(float o, float sigma, uint64_t seed, int i, int step, int q) {
    RPO_FP_STRICT
    if (sigma == 0.0f) return o;
    const rpo_u4 r = rpo_philox(seed, (uint32_t)i, (uint32_t)step, (uint32_t)RPO_STREAM_EVAL_OBS + 0x100u * (uint32_t)q);
    const float z = rpo_normal(r.x, r.y);
    const float d = sigma * z;
    return o + d;
}

// ------------------------------------------------------------------------------------------------ per-constraint report
// Row layout of the report (include/rpo_hip.h: RPO_CON_*): ineq_max[NI] | ineq_steps[NI] | eq_max[NE] | zeros, and ONE
// definition of a cell's update for the fused kernel's CON = 1 instances and rpo_eval_constraints.
__host__ __device__ constexpr int con_width(int ineq_num, int eq_num) {
    return (2 * ineq_num + eq_num + RPO_CON_ALIGN - 1) / RPO_CON_ALIGN * RPO_CON_ALIGN;
}

// index into ineq_viol (cells < 2 NI) or eq_viol (the NE cells behind them) of the value cell c folds in; -1: padding
__device__ __forceinline__ int con_cell_source(int c, int ineq_num, int eq_num) {
    return c < ineq_num ? c : (c < 2 * ineq_num ? c - ineq_num : (c < 2 * ineq_num + eq_num ? c - 2 * ineq_num : -1));
}

// Cell c of a live lane's row after a step: `old` the cell before it (0 at step 0), `v` the transition row's ineq_viol[j] /
// eq_viol[j] for j = con_cell_source(c).  The maxima start at 0 and propagate a NaN, the count compares like viol_steps:
// rpo_eval_lane_update's expressions, per constraint.
__device__ __forceinline__ float rpo_eval_con_cell(int c, int ineq_num, int eq_num, float old, float v, float viol_thresh) {
    RPO_FP_STRICT
    if (c < ineq_num) return nanmax(old, v);                     // ineq_max
    if (c < 2 * ineq_num) return old + ((v > viol_thresh) ? 1.0f : 0.0f);   // ineq_steps
    if (c < 2 * ineq_num + eq_num) return nanmax(old, fabsf(v)); // eq_max
    return 0.0f;
}

// The whole row of one live lane (the fused kernels: NI, NE and so every cell's kind are compile-time): W / 4 16-byte loads
// (none at step 0) and stores.  Plain (cached) accesses: the row is read again at the lane's next step.
template <int NI, int NE>
__device__ __forceinline__ void rpo_eval_con_lane_update(float* __restrict__ con, int step, const float (&ineq)[NI],
                                                         const float (&eq)[NE], float viol_thresh) {
    constexpr int kW = con_width(NI, NE);
    float4* c4 = reinterpret_cast<float4*>(con);
    float r[kW];
#pragma unroll
    for (int q = 0; q < kW / 4; ++q) {
        const float4 x = step > 0 ? c4[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r[4 * q] = x.x; r[4 * q + 1] = x.y; r[4 * q + 2] = x.z; r[4 * q + 3] = x.w;
    }
#pragma unroll
    for (int c = 0; c < kW; ++c) {
        const int j = con_cell_source(c, NI, NE);
        r[c] = rpo_eval_con_cell(c, NI, NE, r[c], j < 0 ? 0.0f : (c < 2 * NI ? ineq[j] : eq[j]), viol_thresh);
    }
#pragma unroll
    for (int q = 0; q < kW / 4; ++q) c4[q] = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}

// ------------------------------------------------------------------------------------------------ keep-best criterion
// ONE definition of "the candidate's curve row beats the incumbent's" (rpo_eval_keep_best; include/rpo_hip.h states it in
// words, tests/test_keep_best_gpu.py in numpy).  A plain constexpr function: no launch-side qualifier, so the same
// text compiles for the decide kernel and for host code.  IEEE comparisons only: a NaN compares false everywhere, so a
// candidate whose rate is a NaN is unsafe and beats no incumbent.
constexpr double keep_best_rate(const double* row) {
    return row[RPO_CURVE_LENGTH] == 0.0 ? __builtin_huge_val() : row[RPO_CURVE_VIOL_STEPS] / row[RPO_CURVE_LENGTH];
}

constexpr bool keep_best_wins(const double* row, const double* best_row, long long best_point, double max_violation_rate) {
    const double ret = row[RPO_CURVE_STATS];
    if (row[RPO_CURVE_NONFINITE] > 0.0 || ret != ret) return false;          // ineligible: never taken
    if (best_point < 0) return true;                                         // no incumbent
    const double rate = keep_best_rate(row), best_rate = keep_best_rate(best_row), best_ret = best_row[RPO_CURVE_STATS];
    const bool safe = rate <= max_violation_rate, best_safe = best_rate <= max_violation_rate;
    if (safe != best_safe) return safe;
    if (safe) return ret > best_ret;
    return rate < best_rate || (rate == best_rate && ret > best_ret);
}

// ------------------------------------------------------------------------------------------------ per-step record
// Row layout of the trace buffer (include/rpo_hip.h: RPO_TRACE_*), one definition for the fused kernel and rpo_eval_record.
__host__ __device__ constexpr int trace_head(int obs_dim, int partial_dim, int action_dim) {
    return (obs_dim + partial_dim + action_dim + 1 + RPO_TRACE_ALIGN - 1) / RPO_TRACE_ALIGN * RPO_TRACE_ALIGN;
}
__host__ __device__ constexpr int trace_width(int obs_dim, int partial_dim, int action_dim) {
    return trace_head(obs_dim, partial_dim, action_dim) + RPO_TRACE_TAIL;
}

typedef float trace_v4 __attribute__((ext_vector_type(4)));

// 16-byte streaming store: the trace is written once and read by the host much later
__device__ __forceinline__ void trace_store(float* dst, float x, float y, float z, float w) {
    __builtin_nontemporal_store(trace_v4{x, y, z, w}, reinterpret_cast<trace_v4*>(dst));
}

// Head of a row of the fused kernels (P = 1, A = 2): everything the step knows before the env runs.
template <int OBS>
__device__ __forceinline__ void trace_store_head(float* __restrict__ row, const float* obs, float proposal, float2 action, int iters) {
    constexpr int kHead = trace_head(OBS, 1, 2);
    float h[kHead];
#pragma unroll
    for (int q = 0; q < kHead; ++q) h[q] = q < OBS ? obs[q] : 0.0f;
    h[OBS] = proposal;
    h[OBS + 1] = action.x;
    h[OBS + 2] = action.y;
    h[OBS + 3] = (float)iters;
#pragma unroll
    for (int q = 0; q < kHead; q += 4) trace_store(row + q, h[q], h[q + 1], h[q + 2], h[q + 3]);
}

// Tail of a row: what the env step produced, in the RPO_TRACE_* slots.
__device__ __forceinline__ void trace_store_tail(float* __restrict__ tail, float reward, float done, float ineq, float eq) {
    static_assert(RPO_TRACE_REWARD == 0 && RPO_TRACE_DONE == 1 && RPO_TRACE_INEQ == 2 && RPO_TRACE_EQ == 3 && RPO_TRACE_TAIL == 4,
                  "the tail is one 16-byte store in slot order");
    trace_store(tail, reward, done, ineq, eq);
}

}  // namespace rpo_eval_dev
