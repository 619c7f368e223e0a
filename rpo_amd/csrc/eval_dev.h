// Per-episode statistics of trainer.evaluate(): one device function shared by the fused evaluation kernel and the
// stepwise path's rpo_eval_accumulate (evaluate.hip), so that both paths have one definition of the statistics.
#pragma once
#include "common.h"

namespace rpo_eval_dev {

// torch.maximum / Tensor.max(dim): a NaN operand propagates (fmaxf would drop it)
__device__ __forceinline__ float nanmax(float a, float b) {
    return a != a ? a : (b != b ? b : (b > a ? b : a));
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

}  // namespace rpo_eval_dev
