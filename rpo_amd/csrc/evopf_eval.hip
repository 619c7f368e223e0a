// Fused policy evaluation on EVOPF-v0 (trainer.evaluate() under schedule fused_eval_evopf=1, rpo_amd/algo/evaluation.py):
// actor -> head -> Complete -> GRG -> env step -> per-episode statistics, looped over the env steps inside one launch.
//
// Geometry: that of the other EVOPF kernels (evopf.hip) -- workgroup = 4 waves = 4 episodes, one wave per SIMD, a solver
// workspace per wave.  The solver phases are per wave; the actor's three layers are workgroup phases between barriers: the four
// observation rows are rows 0..3 of a 16-row MFMA tile (rows 4..15 zero), the activations x0 / h1 stay in LDS, and every
// output tile is the ordered chain of the stepwise path's launch of that layer (mlp_gemm.h: gemm_forward) --
//   first layer   one chain over K = 57 (padded to 64) per 16-column tile          == mlp_gemm_kernel<true, 4>
//   hidden layer  four chains over a quarter of K = 256 each, ((q0 + q1) + q2) + q3 == mlp_gemm_ksplit_kernel<true>
//   heads         the same, one problem per head (W1 | W1b)
// through gemm_chain / gemm_chain_range themselves (mlp_gemm_dev.h), + bias in the launches' expression, relu where the
// consumer would stage the tile.  The per-lane phase is act_project's and the step kernel's own device code (evopf_dev.h).
//
// Every wave of a workgroup -- also one whose lane has finished or lies beyond n -- reaches every barrier of every step: the
// only exit is the workgroup-uniform __syncthreads_or at the top of the loop.
#include "eval_dev.h"
#include "evopf_dev.h"
#include "heads_dev.h"
#include "host_glue.h"
#include "mlp_gemm_dev.h"

using namespace rpo_evopf_dev;
using rpo_host::launch;
using rpo_mlp_dev::f32x4;
using rpo_mlp_dev::gemm_chain;
using rpo_mlp_dev::gemm_chain_range;
using rpo_mlp_dev::kRows;
using rpo_mlp_dev::Mlp;

namespace {

constexpr int kWaves = 4;                                        // episodes per workgroup, one wave each
constexpr int kE = 256;                                          // actor width (embed and hidden)
constexpr int kLdIn = 64 + 4, kLdAct = kE + 4;                   // row strides of the LDS tiles (the launches' ldk = kw + 4)
constexpr int kConW = rpo_eval_dev::con_width(NINEQ, NEQ);       // 144
constexpr int kColReward = 2 * NS + NY, kColDone = kColReward + 1, kColEq = kColReward + 2, kColIneq = kColEq + NEQ;

struct EvalArgs {
    Mlp actor;
    int vec_hidden, vec_heads;    // the launches' vec_w of the hidden layer / the heads (16-byte aligned weight rows)
    int t0, steps;                // env steps [t0, t0 + steps) of the evaluation; t0 == 0 initialises the rows
    float* acc;                   // [n, RPO_EVAL_LEN]
    float* con;                   // CON instances: [n, kConW]
    float* action;                // [n, NY]
    int max_steps;                // projection budget and parameters (RPO_NOISE_NONE)
    float corr_lr, corr_eps, corr_momentum, newton_tol;
    int newton_iters;
    StepArgs step;                // env state and bookkeeping (rows = stats = NULL, auto_reset = 0)
};

// the launches' epilogue operand: (bias ? bias[n] : 0) + (bias2 ? bias2[n] : 0) with bias2 == NULL
__device__ __forceinline__ float gemm_bias(const float* __restrict__ bias, int nc) { return bias[nc] + 0.0f; }

// one quarter (chunk q of four) of the k range of a K = 256 tile, from a zero accumulator: a wave of mlp_gemm_ksplit_kernel
__device__ __forceinline__ f32x4 quarter_chain(const float* a_s, const float* __restrict__ W, int N, int n, int li, int lg, int q,
                                               bool vec) {
    const f32x4 zero = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (vec) return gemm_chain_range<true, true, 4>(a_s, kLdAct, W, kE, kE, N, n, li, lg, zero, q, q + 1);
    return gemm_chain_range<true, false, 4>(a_s, kLdAct, W, kE, kE, N, n, li, lg, zero, q, q + 1);
}

// Registers: 256 VGPRs + 75..117 AGPRs, no scratch, so ONE wave per SIMD -- rpo_evopf_act_project (215 VGPRs) fits two, which
// above 1024 lanes is 1.5 x the lanes per time (two solver waves on a SIMD run at 3/4 speed each).  Asking for two
// here (__launch_bounds__(256, 2)) spills 280..452 bytes per lane and was not taken.
template <int GAUSS, int CON>
__global__ __launch_bounds__(RPO_WAVE * kWaves) void evopf_eval_kernel(EvalArgs p) {
    __shared__ Ws wss[kWaves];
    __shared__ __align__(16) float rows_s[kWaves][RPO_EVOPF_ROW];
    __shared__ __align__(16) float in_s[kRows * kLdIn];           // observations, rows 4..15 and columns 57..63 zero
    __shared__ __align__(16) float act_s[kRows * kLdAct];         // relu(x0), then relu(h1); rows 4..15 zero
    __shared__ float h_s[kWaves][kE];                             // h1 before the relu, parked while x0 is being read
    __shared__ __align__(16) float red_s[1 + GAUSS][kWaves][16][4];   // the heads' quarter tiles, rows 0..3
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / RPO_WAVE), tid = lane_id();
    const int li = tid & 15, lg = tid >> 4;
    const int i = blockIdx.x * kWaves + wave;
    const Mlp& net = p.actor;
    Ws& w = wss[wave];
    float* row = rows_s[wave];
    for (int k = threadIdx.x; k < kRows * kLdIn; k += RPO_WAVE * kWaves) in_s[k] = 0.0f;
    for (int k = threadIdx.x; k < kRows * kLdAct; k += RPO_WAVE * kWaves) act_s[k] = 0.0f;
    // a lane's liveness is wave-uniform and kept in a scalar: from its accumulator row where an earlier launch wrote it,
    // afterwards from the `done` of its own steps
    bool live = i < p.step.n;
    if (live && p.t0 > 0)
        live = (__builtin_amdgcn_readfirstlane(__float_as_int(p.acc[(size_t)i * RPO_EVAL_LEN + RPO_EVAL_WORD])) & RPO_EVAL_ALIVE) != 0;
    for (int s = p.t0; s < p.t0 + p.steps; ++s) {
        if (!__syncthreads_or(live)) return;                     // the ONE exit; also the barrier in front of the tiles' reuse
        // ---- observations: wave r stages row r (a lane beyond n keeps its zeros)
        if (i < p.step.n && tid < NS) in_s[wave * kLdIn + tid] = p.step.state[(size_t)i * NS + tid];
        __syncthreads();
        // ---- first layer: 16 column tiles, four per wave
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
            const int n = (wave * 4 + t) * 16 + li;
            const f32x4 acc = gemm_chain<true, false, 4>(in_s, kLdIn, net.Ws, NS, NS, kE, n, li, lg, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
            const float bv = gemm_bias(net.bs, n);
            if (lg == 0) {
#pragma unroll
                for (int r = 0; r < kWaves; ++r) act_s[r * kLdAct + n] = rpo_relu(acc[r] + bv);
            }
        }
        __syncthreads();
        // ---- hidden layer: 16 column tiles x 4 quarter chains; a wave owns the four quarters of its tiles and adds them itself
        // (h_s: the thread that writes a column of h1 reads it back below -- act_s is still x0 to the other waves)
#pragma unroll 1
        for (int t = 0; t < 4; ++t) {
            const int n = (wave * 4 + t) * 16 + li;
            const f32x4 q0 = quarter_chain(act_s, net.W0, kE, n, li, lg, 0, p.vec_hidden != 0);
            const f32x4 q1 = quarter_chain(act_s, net.W0, kE, n, li, lg, 1, p.vec_hidden != 0);
            const f32x4 q2 = quarter_chain(act_s, net.W0, kE, n, li, lg, 2, p.vec_hidden != 0);
            const f32x4 q3 = quarter_chain(act_s, net.W0, kE, n, li, lg, 3, p.vec_hidden != 0);
            const f32x4 acc = ((q0 + q1) + q2) + q3;
            const float bv = gemm_bias(net.b0, n);
            if (lg == 0) {
#pragma unroll
                for (int r = 0; r < kWaves; ++r) h_s[r][n] = acc[r] + bv;
            }
        }
        __syncthreads();                                         // every wave has read x0: h1 takes its place
        if (lg == 0) {
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                const int n = (wave * 4 + t) * 16 + li;
#pragma unroll
                for (int r = 0; r < kWaves; ++r) act_s[r * kLdAct + n] = rpo_relu(h_s[r][n]);
            }
        }
        __syncthreads();
        // ---- heads: one 14-column tile per head, wave q takes quarter q; the quarters meet in LDS
#pragma unroll
        for (int hd = 0; hd <= GAUSS; ++hd) {
            const f32x4 acc = quarter_chain(act_s, hd ? net.W1b : net.W1, NP, li, li, lg, wave, p.vec_heads != 0);
            if (lg == 0) *reinterpret_cast<f32x4*>(red_s[hd][wave][li]) = acc;
        }
        __syncthreads();
        // ---- the wave's own lane: head, Complete, GRG, env step, statistics
        if (live) {
            load_consts(w, p.step.consts);                       // (as act_project: the wave's workspace, this step)
            load_row(w.s, p.step.state + (size_t)i * NS, NS);
            sync();
            float z = 0.0f;
            if (tid < NP) {
                float raw[1 + GAUSS];
#pragma unroll
                for (int hd = 0; hd <= GAUSS; ++hd)
                    raw[hd] = (((red_s[hd][0][tid][wave] + red_s[hd][1][tid][wave]) + red_s[hd][2][tid][wave]) + red_s[hd][3][tid][wave]) +
                              gemm_bias(hd ? net.b1b : net.b1, tid);
                float lo, hi;
                partial_box(w, tid, lo, hi);                     // (basic_box, as row_box of the Gaussian head kernel: the same table and state)
                if (GAUSS) {
                    const float scale = (hi - lo) * 0.5f;
                    z = rpo_head_dev::gauss_head_row(raw[0], raw[GAUSS], 0.0f, scale, lo + scale, lo, hi, 1, nullptr);
                } else {
                    z = tanh_box_raw(raw[0], lo, hi);
                }
            }
            const RowLane L = make_row_lane(w);
            complete_partial_v2(w, L, z, p.newton_tol, p.newton_iters);
            const int k = grad_steps_v2(w, L, p.max_steps, p.corr_lr, p.corr_eps, p.corr_momentum);
            if (tid < NY) p.action[(size_t)i * NY + tid] = w.a[tid];
            evopf_step_lane(p.step, w, row, i, 0);               // (reads the action back: the same thread wrote it)
            if (CON) {                                           // one cell per thread and round, as rpo_eval_constraints
                float* con = p.con + (size_t)i * kConW;
                for (int c = tid; c < kConW; c += RPO_WAVE) {
                    const int j = rpo_eval_dev::con_cell_source(c, NINEQ, NEQ);
                    const float v = j < 0 ? 0.0f : row[(c < 2 * NINEQ ? kColIneq : kColEq) + j];
                    con[c] = rpo_eval_dev::rpo_eval_con_cell(c, NINEQ, NEQ, s > 0 ? con[c] : 0.0f, v, p.step.viol_thresh);
                }
            }
            float ineq, eq;
            rpo_eval_dev::row_violations(row, kColIneq, NINEQ, kColEq, NEQ, ineq, eq);
            const float done = row[kColDone];
            if (tid == 0)
                rpo_eval_dev::rpo_eval_lane_update(p.acc + (size_t)i * RPO_EVAL_LEN, s, row[kColReward], ineq, eq, done, k,
                                                   p.step.viol_thresh);
            live = __builtin_amdgcn_readfirstlane(__float_as_int(done)) == 0;
        }
    }
}

template <int GAUSS>
int launch_eval(const EvalArgs& args, void* stream) {
    const dim3 grid((args.step.n + kWaves - 1) / kWaves);
    if (args.con) return launch(evopf_eval_kernel<GAUSS, 1>, grid, RPO_WAVE * kWaves, 0, stream, args);
    return launch(evopf_eval_kernel<GAUSS, 0>, grid, RPO_WAVE * kWaves, 0, stream, args);
}

// gemm_launch's vec_w of a forward layer with K = 256: rows of 256 floats from a 16-byte aligned base
bool weight_rows_aligned(const float* W) { return (reinterpret_cast<uintptr_t>(W) & 15u) == 0; }

}  // namespace

extern "C" int rpo_evopf_evaluate(const rpo_mlp* actor_host, int gauss, int n_envs, float* state, float* action, int* ep_len,
                                  float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, int max_steps,
                                  float corr_lr, float corr_eps, float corr_momentum, float newton_tol, int newton_max_iters,
                                  const float* consts_dev, int max_episode_steps, float viol_thresh, unsigned long long seed,
                                  unsigned env_id_base, float* con, void* stream) {
    if (!actor_host) return RPO_ERR_NULL;
    if (int e = rpo_host::check_eval_range(n_envs, t0, steps, max_episode_steps, max_steps)) return e;
    if (newton_max_iters <= 0) return RPO_ERR_ARG;
    if (!state || !action || !ep_len || !ep_ret || !ep_count || !acc || !consts_dev) return RPO_ERR_NULL;
    if (con)
        if (int e = rpo_host::check_eval_con(con)) return e;
    EvalArgs args{};
    args.actor = rpo_host::to_dev(actor_host);
    const Mlp& a = args.actor;
    if (a.S != NS || a.A != 0 || a.E != kE || a.H != kE || a.cat || a.hd != NP || a.n_out != (gauss ? 2 : 1) || !a.Ws || !a.bs || !a.W0 ||
        !a.b0 || !a.W1 || !a.b1 || (gauss && (!a.W1b || !a.b1b)))
        return RPO_ERR_ARG;
    args.vec_hidden = weight_rows_aligned(a.W0);
    args.vec_heads = weight_rows_aligned(a.W1) && (!gauss || weight_rows_aligned(a.W1b));
    args.t0 = t0; args.steps = steps; args.acc = acc; args.con = con; args.action = action;
    args.max_steps = max_steps; args.corr_lr = corr_lr; args.corr_eps = corr_eps; args.corr_momentum = corr_momentum;
    args.newton_tol = newton_tol; args.newton_iters = newton_max_iters;
    args.step = StepArgs{n_envs, state, action, ep_len, ep_ret, ep_count, nullptr, 1, nullptr, 0, ctrl, max_episode_steps, 0,
                         viol_thresh, consts_dev, (uint64_t)seed, (uint32_t)env_id_base};
    return gauss ? launch_eval<1>(args, stream) : launch_eval<0>(args, stream);
}
