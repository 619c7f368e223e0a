// Projected actions for caller-supplied observations (trainer.act(), rpo_amd/algo/acting.py): one launch from n observation
// rows to the completed, projected actions, the proposals, the GRG iteration counts and the signed residuals.
//
//   policy_act_kernel    the ROW-TILE form: eval_kernel (evaluate.hip) without the step loop, the accumulators and the env
//                        lane -- obs tile (from the caller's rows) -> actor MLP (f32 MFMA) -> [mean head] -> Complete -> GRG ->
//                        residuals -> stores; 16 rows per workgroup, 64 once that still fills the chip.
//   (act_stream.hip)     the STREAMING form from RPO_ROLLOUT_STREAM_FROM rows: rollout_stream_kernel's structure.
//
//   project_profile_kernel  the stand-alone projection of trainer.act(profile=True)'s stepwise path; policy_act_kernel's
//                        PROFILE = 1 instances are its fused path.
//
// Nothing is carried between rows, no env state, control word or generator is touched.  The per-row chain is act_dev.h's.
#include "act_dev.h"
#include "host_glue.h"

namespace {

using namespace rpo_mlp_dev;
using rpo_host::launch;
using rpo_host::to_dev;

// PROFILE = 1: the row's projection also writes its entries of the profile planes (act_dev.h: act_project_profile); the
// PROFILE = 0 instances take no profile argument and are the kernel as it was.  The profile is touched behind the forward only.
template <class ENV, int RT, int PROFILE>
__global__ __launch_bounds__(kFwdThreads) void policy_act_kernel(PolicyActArgs<ENV> p, typename ENV::Consts c,
                                                                 typename std::conditional<PROFILE != 0, ActProfile, ActNoProfile>::type prof) {
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
    if (tid < kRowsWg && i < p.n) {                              // (nothing per-row was alive across the MFMA loops)
        if constexpr (PROFILE != 0) policy_act_row_profile<ENV>(p, c, lds.in_s + tid * kInS, i, lds.out[tid * 2], lds.out[tid * 2 + 1], prof);
        else policy_act_row<ENV>(p, c, lds.in_s + tid * kInS, i, lds.out[tid * 2], lds.out[tid * 2 + 1]);
    }
}

// The stand-alone profiled projection (the stepwise path's launch behind the proposal launches): one thread per row, as
// *_act_project under RPO_NOISE_NONE; obs: SpringPendulum's rows (CartSafe's projection does not read the state).
template <class ENV>
__global__ __launch_bounds__(RPO_BLOCK) void project_profile_kernel(typename ENV::ActArgs p, typename ENV::Consts c, const float* obs,
                                                                    int obs_stride, ActProfile q) {
    for (int i = blockIdx.x * RPO_BLOCK + threadIdx.x; i < p.n; i += gridDim.x * RPO_BLOCK) {
        int k;
        const float2 a = act_project_profile<ENV>(p, c, obs ? obs + (size_t)i * obs_stride : nullptr, i, p.n, p.ap_raw[i], q, k);
        act_store2(p.action + (size_t)i * 2, a.x, a.y);
        if (p.iters) act_store(p.iters + i, k);
    }
}

int check_profile(const float* profile, int K) {                 // [K + 1, n, 4]: written with 16-byte stores
    if (!profile || K < 0 || reinterpret_cast<uintptr_t>(profile) % 16) return RPO_ERR_ARG;
    return 0;
}

int check_act_actor(const Mlp& actor, int obs_dim, int gauss) {  // (host_glue.h's check_actor and every bias; E below)
    if (actor.hd > 1 || actor.S != obs_dim || actor.A != 0 || actor.n_out != (gauss ? 2 : 1) || actor.cat || actor.H != 256 || !actor.Ws ||
        !actor.bs || !actor.W0 || !actor.b0 || !actor.W1 || !actor.b1 || (gauss && (!actor.W1b || !actor.b1b)))
        return RPO_ERR_ARG;
    if (actor.E != 128) return RPO_ERR_ARG;                      // the E = 256 instance of the tile spills (evaluate.hip)
    return 0;
}

// A projection without exploration, clock or statistics (RPO_NOISE_NONE), as the entry points here take it: what fill_env makes the
// env's ActArgs and Consts of.  obs / obs_stride: SpringPendulum's rows; consts_host / partial: CartSafe's table.
struct Projection {
    int n;
    const float* obs;
    int obs_stride;
    const float* ap_raw;
    float* action;
    int* iters;
    float box_lo, box_hi;
    int max_steps;
    float corr_lr, corr_eps, corr_momentum;
    const float* consts_host;
    int partial;
};

int fill_env(rpo_cart_dev::ActArgs& a, CartEnv::Consts& c, const Projection& q) {
    if (int e = rpo_cart_dev::load_consts(c, q.consts_host, q.partial)) return e;
    a = rpo_cart_dev::ActArgs{q.n, q.ap_raw, nullptr, q.action, q.iters, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f, q.box_lo, q.box_hi,
                              q.max_steps, q.corr_lr, q.corr_eps, q.corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    return 0;
}

int fill_env(rpo_pend_dev::ActArgs& a, PendEnv::Consts& c, const Projection& q) {
    c = PendEnv::Consts{0};
    a = rpo_pend_dev::ActArgs{q.n, q.obs, q.obs_stride, q.ap_raw, nullptr, q.action, q.iters, RPO_NOISE_NONE, 0.0f, 0.0f, 0.0f,
                              q.box_lo, q.box_hi, q.max_steps, q.corr_lr, q.corr_eps, q.corr_momentum, 0ull, 0u, nullptr, nullptr, 0};
    return 0;
}

// *_project_profile.  The env's constants are tested first, then the rows
template <class ENV>
int project_profile(const Projection& q, float* profile, void* stream) {
    typename ENV::ActArgs a;
    typename ENV::Consts c;
    if (int e = fill_env(a, c, q)) return e;
    if (a.n <= 0) return RPO_ERR_ARG;
    if (!a.ap_raw || !a.action) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(a.action) % 8) return RPO_ERR_ARG;
    if (int e = check_profile(profile, a.max_steps)) return e;
    return launch(project_profile_kernel<ENV>, dim3(rpo_grid_for(a.n)), RPO_BLOCK, 0, stream, a, c, q.obs, q.obs_stride,
                  ActProfile{profile, a.max_steps});
}

// What *_policy_act and *_policy_act_profile take alike (q: its obs rows are the policy's, its ap_raw and iters unused)
struct PolicyAct {
    const rpo_mlp* actor_host;
    int gauss;
    float scale, base;
    const float* obs;
    int obs_stride;
    float* proposal;
    int* iters;
    float *eq_resid, *ineq_resid;
    Projection q;
};

template <class ENV>
int fill_policy_act(PolicyActArgs<ENV>& args, typename ENV::Consts& c, const PolicyAct& p) {
    const int n = p.q.n;
    if (!p.actor_host) return RPO_ERR_NULL;
    if (n <= 0 || p.obs_stride < ENV::OBS || p.q.max_steps < 0) return RPO_ERR_ARG;
    if (!p.obs || !p.q.action) return RPO_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(p.q.action) % 8) return RPO_ERR_ARG;                   // 8-byte stores of the action rows
    if (std::is_same<ENV, CartEnv>::value && reinterpret_cast<uintptr_t>(p.ineq_resid) % 8) return RPO_ERR_ARG;   // ... and of g[0..5]
    args.actor = to_dev(p.actor_host);
    if (int e = check_act_actor(args.actor, ENV::OBS, p.gauss)) return e;
    args.scale = p.scale; args.base = p.base; args.gauss = p.gauss ? 1 : 0; args.n = n; args.obs = p.obs; args.obs_stride = p.obs_stride;
    args.proposal = p.proposal; args.iters = p.iters; args.eq = p.eq_resid; args.ineq = p.ineq_resid;
    return fill_env(args.act, c, p.q);
}

// The row tile of n rows: 64 rows per workgroup once that still fills the chip (launch_eval's tile rule)
template <class ENV, int PROFILE, class Prof>
int launch_tile(const PolicyActArgs<ENV>& args, const typename ENV::Consts& c, const Prof& prof, void* stream) {
    const int n = args.n;
    if (n >= 64 * 192) return launch(policy_act_kernel<ENV, 4, PROFILE>, dim3((n + 63) / 64), kFwdThreads, 0, stream, args, c, prof);
    return launch(policy_act_kernel<ENV, 1, PROFILE>, dim3((n + 15) / 16), kFwdThreads, 0, stream, args, c, prof);
}

// *_policy_act.  form: 0 by size (the rollout's rule: launch_stream in rollout_stream.hip), 1 row tile, 2 streaming G = 1, 3 streaming G = 4
template <class ENV>
int policy_act(const PolicyAct& p, int env, int form, void* stream) {
    PolicyActArgs<ENV> args{};
    typename ENV::Consts c;
    if (int e = fill_policy_act(args, c, p)) return e;
    const int n = args.n;
    if (form < 0 || form > 3) return RPO_ERR_ARG;
    if (form == 0 && n >= RPO_ROLLOUT_STREAM_FROM) {
        const int e = rpo_act_stream_launch(env, &args, &c, n >= 4 * kRows * 16 * rpo_cu_count(), stream);
        if (e >= 0) return e;                                    // (-1: the form does not apply: the row tile below)
    } else if (form >= 2) {
        const int e = rpo_act_stream_launch(env, &args, &c, form == 3, stream);
        return e < 0 ? RPO_ERR_ARG : e;
    }
    return launch_tile<ENV, 0>(args, c, ActNoProfile{}, stream);
}

// *_policy_act_profile: always the row tile (a profile instance of the streaming form does not exist)
template <class ENV>
int policy_act_profile(const PolicyAct& p, float* profile, void* stream) {
    PolicyActArgs<ENV> args{};
    typename ENV::Consts c;
    if (int e = fill_policy_act(args, c, p)) return e;
    if (int e = check_profile(profile, args.act.max_steps)) return e;
    return launch_tile<ENV, 1>(args, c, ActProfile{profile, args.act.max_steps}, stream);
}

}  // namespace

extern "C" {

int rpo_cartsafe_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs, int obs_stride,
                            float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid, float box_lo,
                            float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                            const float* consts_host, int partial, int form, void* stream) {
    return policy_act<CartEnv>({actor_host, gauss, scale, base, obs, obs_stride, proposal, iters, eq_resid, ineq_resid,
                                {n, nullptr, 0, nullptr, action, nullptr, box_lo, box_hi, max_steps, corr_lr, corr_eps, corr_momentum,
                                 consts_host, partial}}, 0, form, stream);
}

int rpo_pendulum_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs, int obs_stride,
                            float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid, float box_lo,
                            float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum, int form,
                            void* stream) {
    return policy_act<PendEnv>({actor_host, gauss, scale, base, obs, obs_stride, proposal, iters, eq_resid, ineq_resid,
                                {n, nullptr, 5, nullptr, action, nullptr, box_lo, box_hi, max_steps, corr_lr, corr_eps, corr_momentum,
                                 nullptr, 0}}, 1, form, stream);
}

int rpo_cartsafe_policy_act_profile(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                                    int obs_stride, float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid,
                                    float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                    const float* consts_host, int partial, float* profile, void* stream) {
    return policy_act_profile<CartEnv>({actor_host, gauss, scale, base, obs, obs_stride, proposal, iters, eq_resid, ineq_resid,
                                        {n, nullptr, 0, nullptr, action, nullptr, box_lo, box_hi, max_steps, corr_lr, corr_eps,
                                         corr_momentum, consts_host, partial}}, profile, stream);
}

int rpo_pendulum_policy_act_profile(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                                    int obs_stride, float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid,
                                    float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                    float* profile, void* stream) {
    return policy_act_profile<PendEnv>({actor_host, gauss, scale, base, obs, obs_stride, proposal, iters, eq_resid, ineq_resid,
                                        {n, nullptr, 5, nullptr, action, nullptr, box_lo, box_hi, max_steps, corr_lr, corr_eps,
                                         corr_momentum, nullptr, 0}}, profile, stream);
}

int rpo_cartsafe_project_profile(int n, const float* ap_raw, float* action, int* iters, int max_steps, float corr_lr, float corr_eps,
                                 float corr_momentum, const float* consts_host, int partial, float* profile, void* stream) {
    return project_profile<CartEnv>({n, nullptr, 0, ap_raw, action, iters, 0.0f, 0.0f, max_steps, corr_lr, corr_eps, corr_momentum,
                                     consts_host, partial}, profile, stream);
}

int rpo_pendulum_project_profile(int n, const float* obs, int obs_stride, const float* ap_raw, float* action, int* iters,
                                 int max_steps, float corr_lr, float corr_eps, float corr_momentum, float* profile, void* stream) {
    if (n > 0 && !obs) return RPO_ERR_NULL;                      // (SpringPendulum's rows: tested in front of n)
    if (obs_stride < 5) return RPO_ERR_ARG;
    return project_profile<PendEnv>({n, obs, obs_stride, ap_raw, action, iters, 0.0f, 0.0f, max_steps, corr_lr, corr_eps, corr_momentum,
                                     nullptr, 0}, profile, stream);
}

}  // extern "C"
