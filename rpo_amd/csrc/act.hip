// Projected actions for caller-supplied observations (trainer.act(), rpo_amd/algo/acting.py): one launch from n observation
// rows to the completed, projected actions, the proposals, the GRG iteration counts and the signed residuals.
//
//   policy_act_kernel    the ROW-TILE form: eval_kernel (evaluate.hip) without the step loop, the accumulators and the env
//                        lane -- obs tile (from the caller's rows) -> actor MLP (f32 MFMA) -> [mean head] -> Complete -> GRG ->
//                        residuals -> stores; 16 rows per workgroup, 64 once that still fills the chip.
//   (act_stream.hip)     the STREAMING form from RPO_ROLLOUT_STREAM_FROM rows: rollout_stream_kernel's structure.
//
// Nothing is carried between rows, no env state, control word or generator is touched.  The per-row chain is act_dev.h's.
#include "act_dev.h"

namespace {

using namespace rpo_mlp_dev;

Mlp act_to_dev(const rpo_mlp* h) {
    return Mlp{h->Ws, h->bs, h->Wa, h->ba, h->W0, h->b0, h->W1, h->b1, h->W1b, h->b1b, h->S, h->A, h->E, h->H, h->n_out, h->cat, h->head_dim};
}

template <class ENV, int RT>
__global__ __launch_bounds__(kFwdThreads) void policy_act_kernel(PolicyActArgs<ENV> p, typename ENV::Consts c) {
    typedef TileLds<128, RT, 8, 8> Lds;                          // 16 * RT rows per workgroup; OBS <= 8
    __shared__ Lds lds;
    constexpr int kInS = Lds::kS, kRowsWg = kRows * RT, OBS = ENV::OBS;
    const int row0 = blockIdx.x * kRowsWg;
    const int tid = threadIdx.x;
    if (tid < kRowsWg * OBS) {                                   // the observation tile, from the caller's rows
        const int r = tid / OBS, q = tid - r * OBS;
        lds.in_s[r * kInS + q] = (row0 + r < p.n) ? p.obs[(size_t)(row0 + r) * p.obs_stride + q] : 0.0f;
    }
    mlp_tile_forward<128, 256, RT, Lds>(p.actor, lds, row0, p.n, nullptr, nullptr, p.gauss ? 0 : 1, p.scale, p.base);
    const int i = row0 + tid;
    if (tid < kRowsWg && i < p.n)                                // (nothing per-row was alive across the MFMA loops)
        policy_act_row<ENV>(p, c, lds.in_s + tid * kInS, i, lds.out[tid * 2], lds.out[tid * 2 + 1]);
}

int check_act_actor(const Mlp& actor, int obs_dim, int gauss) {  // (check_eval_actor's conditions; E below)
    if (actor.hd > 1 || actor.S != obs_dim || actor.A != 0 || actor.n_out != (gauss ? 2 : 1) || actor.cat || actor.H != 256 || !actor.Ws ||
        !actor.bs || !actor.W0 || !actor.b0 || !actor.W1 || !actor.b1 || (gauss && (!actor.W1b || !actor.b1b)))
        return RPO_ERR_ARG;
    if (actor.E != 128) return RPO_ERR_ARG;                      // the E = 256 instance of the tile spills (evaluate.hip)
    return 0;
}

// form: 0 by size (the rollout's rule: launch_stream in rollout_stream.hip), 1 row tile, 2 streaming G = 1, 3 streaming G = 4
template <class ENV>
int launch_act(const PolicyActArgs<ENV>& args, const typename ENV::Consts& c, int env, int form, void* stream) {
    const int n = args.n;
    if (form < 0 || form > 3) return RPO_ERR_ARG;
    if (form == 0 && n >= RPO_ROLLOUT_STREAM_FROM) {
        const int e = rpo_act_stream_launch(env, &args, &c, n >= 4 * kRows * 16 * rpo_cu_count(), stream);
        if (e >= 0) return e;                                    // (-1: the form does not apply: the row tile below)
    } else if (form >= 2) {
        const int e = rpo_act_stream_launch(env, &args, &c, form == 3, stream);
        return e < 0 ? RPO_ERR_ARG : e;
    }
    if (n >= 64 * 192) {                                         // launch_eval's tile rule
        hipLaunchKernelGGL((policy_act_kernel<ENV, 4>), dim3((n + 63) / 64), dim3(kFwdThreads), 0, (hipStream_t)stream, args, c);
    } else {
        hipLaunchKernelGGL((policy_act_kernel<ENV, 1>), dim3((n + 15) / 16), dim3(kFwdThreads), 0, (hipStream_t)stream, args, c);
    }
    RPO_LAUNCH_CHECK();
    return 0;
}

template <class ENV>
int fill_act_args(PolicyActArgs<ENV>& args, const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                  int obs_stride, float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid, int max_steps) {
    if (!actor_host) return RPO_ERR_NULL;
    if (n <= 0 || obs_stride < ENV::OBS || max_steps < 0) return RPO_ERR_ARG;
    if (!obs || !action) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(action) % 8) return RPO_ERR_ARG;                       // 8-byte stores of the action rows
    if (std::is_same<ENV, CartEnv>::value && reinterpret_cast<uintptr_t>(ineq_resid) % 8) return RPO_ERR_ARG;   // ... and of g[0..5]
    args.actor = act_to_dev(actor_host);
    if (int e = check_act_actor(args.actor, ENV::OBS, gauss)) return e;
    args.scale = scale; args.base = base; args.gauss = gauss ? 1 : 0; args.n = n; args.obs = obs; args.obs_stride = obs_stride;
    args.proposal = proposal; args.iters = iters; args.eq = eq_resid; args.ineq = ineq_resid;
    return 0;
}

}  // namespace

extern "C" {

int rpo_cartsafe_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs, int obs_stride,
                            float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid, float box_lo,
                            float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                            const float* consts_host, int partial, int form, void* stream) {
    PolicyActArgs<CartEnv> args{};
    if (int e = fill_act_args<CartEnv>(args, actor_host, gauss, scale, base, n, obs, obs_stride, action, proposal, iters, eq_resid,
                                       ineq_resid, max_steps))
        return e;
    rpo_cart_dev::CartConsts c;
    if (int e = rpo_cart_dev::load_consts(c, consts_host, partial)) return e;
    args.act = rpo_cart_dev::ActArgs{n, nullptr, nullptr, action, nullptr, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f, box_lo, box_hi,
                                     max_steps, corr_lr, corr_eps, corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    return launch_act<CartEnv>(args, c, 0, form, stream);
}

int rpo_pendulum_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs, int obs_stride,
                            float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid, float box_lo,
                            float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum, int form,
                            void* stream) {
    PolicyActArgs<PendEnv> args{};
    if (int e = fill_act_args<PendEnv>(args, actor_host, gauss, scale, base, n, obs, obs_stride, action, proposal, iters, eq_resid,
                                       ineq_resid, max_steps))
        return e;
    args.act = rpo_pend_dev::ActArgs{n, nullptr, 5, nullptr, nullptr, action, nullptr, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f,
                                     box_lo, box_hi, max_steps, corr_lr, corr_eps, corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    const PendEnv::Consts c{0};
    return launch_act<PendEnv>(args, c, 1, form, stream);
}

}  // extern "C"
