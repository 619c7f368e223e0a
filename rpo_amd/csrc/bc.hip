// Behaviour-cloning head of trainer.pretrain() (rpo_amd/algo/pretrain.py): the loss of the actor's tanh-box output against a
// demonstrated basic action, in BOX-NORMALISED coordinates, and its gradient w.r.t. the raw actor output -- what sits between
// rpo_mlp_forward (raw outputs, no box) and rpo_mlp_backward in a cloning step.  include/rpo_hip.h (rpo_bc_head) has the formulas.
//
// One kernel, templated on where the box of (row i, component j) comes from: ConstBox -- P pairs in the launch arguments
// (CartSafe / SpringPendulum: the constant partial box) -- or EvopfBox -- basic_box of evopf_dev.h on the row's observation (the
// state-of-charge dependent battery box; the one definition EVOPFEnv.update, the projection and evopf_tanh_box_bwd_kernel share).
//
// Geometry: a DPP row of 16 lanes per batch row (P <= 16), 16 batch rows per workgroup pass = one GROUP = one loss partial.
// Group g is always rows [16 g, 16 g + 16), whatever the grid: a workgroup strides over the groups, sums a row's terms with the
// fixed butterfly of rpo_row16_sum_lane0, the 16 row sums one after the other in row order, and WRITES loss_parts[g] -- no atomics,
// no dependence on the grid size or on which workgroup arrives when.  Every element of draw has exactly one writer.
// Bandwidth-trivial: 3 floats in, 1 - 2 out per term.
#include "evopf_dev.h"
#include "launch.h"

using rpo_host::launch;

namespace {

constexpr int kBcLanes = 16;                          // lanes per batch row (>= P)
constexpr int kBcRows = RPO_BLOCK / kBcLanes;         // batch rows per group
constexpr float kBcMinScale = 1e-6f;                  // boxes at most this wide (half-width) are empty: their terms are 0

struct BcArgs {
    int n, P, heads;
    const float* raw;                                 // [n, heads * P]
    const float* target;                              // [n, P], rows target_stride floats apart
    int target_stride;
    float clip, inv_bp;                               // inv_bp = 1 / (n P)
    float* draw;                                      // [n, heads * P]
    float* loss_parts;                                // [(n + 15) / 16]
    float w[kBcLanes];                                // per-component weights (1 without any)
};

// element j of a small table in the launch arguments, by a chain of selects: a lane-dependent index into kernel arguments would
// otherwise be served from a private copy of the table
__device__ __forceinline__ float pick16(const float (&a)[kBcLanes], int j) {
    float v = a[0];
#pragma unroll
    for (int k = 1; k < kBcLanes; ++k) v = j == k ? a[k] : v;
    return v;
}

struct ConstBox {
    float lo[kBcLanes], hi[kBcLanes];
    __device__ __forceinline__ void get(long long, int j, float& l, float& h) const { l = pick16(lo, j); h = pick16(hi, j); }
};

struct EvopfBox {
    const float* state;
    int state_stride;
    const float* consts;
    __device__ __forceinline__ void get(long long i, int j, float& l, float& h) const {
        rpo_evopf_dev::basic_box(consts, state + (size_t)i * state_stride + 2 * rpo_evopf_dev::NB, j, l, h);
    }
};

template <class Box>
__global__ __launch_bounds__(RPO_BLOCK) void bc_head_kernel(BcArgs p, Box box) {
    RPO_FP_STRICT
    __shared__ float red[kBcRows];
    const int j = threadIdx.x & (kBcLanes - 1), r = threadIdx.x / kBcLanes;
    const long long groups = ((long long)p.n + kBcRows - 1) / kBcRows;
    const int width = p.heads * p.P;
    const float w = pick16(p.w, j);
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long i = g * kBcRows + r;
        float term = 0.0f;
        if (i < p.n && j < p.P) {
            float lo, hi;
            box.get(i, j, lo, hi);
            const float scale = (hi - lo) * 0.5f, base = lo + scale;
            float grad = 0.0f;
            if (!(scale <= kBcMinScale)) {            // (a NaN box is not an empty one: it reaches the outputs)
                const float u = rpo_clamp((p.target[(size_t)i * p.target_stride + j] - base) / scale, -p.clip, p.clip);
                const float y = tanhf(p.raw[(size_t)i * width + j]);         // a NaN raw output stays NaN in draw and in the loss
                const float d = y - u;
                term = w * d * d;
                grad = 2.0f * w * p.inv_bp * d * (1.0f - y * y);
            }
            p.draw[(size_t)i * width + j] = grad;
            if (p.heads == 2) p.draw[(size_t)i * width + p.P + j] = 0.0f;    // the log-std head takes no part in the loss
        }
        term = rpo_row16_sum_lane0(term);             // (every lane of the workgroup is here: rows past n and lanes past P add 0)
        if (j == 0) red[r] = term;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.0f;
            for (int k = 0; k < kBcRows; ++k) s += red[k];
            p.loss_parts[g] = s * p.inv_bp;
        }
        __syncthreads();                              // red is written again by the next group
    }
}

// the checks the two entry points share, and the arguments they produce
int bc_args(BcArgs& a, int n, int P, int heads, const float* raw, const float* target, int target_stride, const float* weights,
            float clip, float* draw, float* loss_parts) {
    if (n <= 0 || P <= 0 || P > kBcLanes || (heads != 1 && heads != 2) || target_stride < P) return RPO_ERR_ARG;
    if (!(clip > 0.0f && clip <= 1.0f)) return RPO_ERR_ARG;
    if (!raw || !target || !draw || !loss_parts) return RPO_ERR_NULL;
    a = BcArgs{n, P, heads, raw, target, target_stride, clip, (float)(1.0 / ((double)n * (double)P)), draw, loss_parts, {}};
    for (int j = 0; j < kBcLanes; ++j) a.w[j] = j < P ? (weights ? weights[j] : 1.0f) : 0.0f;
    for (int j = 0; j < P; ++j)
        if (!(a.w[j] >= 0.0f)) return RPO_ERR_ARG;
    return 0;
}

int bc_grid(int n) { return rpo_grid_for(((long long)n + kBcRows - 1) / kBcRows, 1); }

}  // namespace

extern "C" {

int rpo_bc_head(int n, int P, int heads, const float* raw, const float* target, int target_stride, const float* lo_host,
                const float* hi_host, const float* weights_host, float clip, float* draw, float* loss_parts, void* stream) {
    BcArgs a;
    if (int e = bc_args(a, n, P, heads, raw, target, target_stride, weights_host, clip, draw, loss_parts)) return e;
    if (!lo_host || !hi_host) return RPO_ERR_NULL;
    ConstBox box{};
    for (int j = 0; j < P; ++j) { box.lo[j] = lo_host[j]; box.hi[j] = hi_host[j]; }
    return launch(bc_head_kernel<ConstBox>, dim3(bc_grid(n)), RPO_BLOCK, 0, stream, a, box);
}

int rpo_evopf_bc_head(int n, int heads, const float* state, int state_stride, const float* raw, const float* target,
                      int target_stride, const float* weights_host, float clip, float* draw, float* loss_parts,
                      const float* consts_dev, void* stream) {
    BcArgs a;
    if (int e = bc_args(a, n, rpo_evopf_dev::NP, heads, raw, target, target_stride, weights_host, clip, draw, loss_parts)) return e;
    if (!state || !consts_dev) return RPO_ERR_NULL;
    if (state_stride < RPO_EVOPF_STATE) return RPO_ERR_ARG;
    return launch(bc_head_kernel<EvopfBox>, dim3(bc_grid(n)), RPO_BLOCK, 0, stream, a, EvopfBox{state, state_stride, consts_dev});
}

}  // extern "C"
