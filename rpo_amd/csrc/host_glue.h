// Host-side glue of the C-ABI entry points, shared by the translation units that take networks (fused.hip, nsplit.hip,
// evaluate.hip, act.hip, mlp.hip): the host structs -> the kernels' argument structs, the shape checks of the 128 / 256 -> 256
// networks with scalar heads, and the launch plumbing (the launch itself: launch.h).  Host code only: nothing here reaches a code
// object.
#pragma once
#include "launch.h"
#include "mlp_tile.h"

namespace rpo_host {

using rpo_mlp_dev::Mlp;
using rpo_mlp_dev::MlpGrad;

inline Mlp to_dev(const rpo_mlp* h) {
    return Mlp{h->Ws, h->bs, h->Wa, h->ba, h->W0, h->b0, h->W1, h->b1, h->W1b, h->b1b, h->S, h->A, h->E, h->H, h->n_out, h->cat, h->head_dim};
}

inline MlpGrad grad_dev(const rpo_mlp_grad* g) {
    if (!g) return MlpGrad{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return MlpGrad{g->Ws, g->bs, g->Wa, g->ba, g->W0, g->b0, g->W1, g->b1, g->W1b, g->b1b};
}

// An actor of the row-tile kernels: obs_dim -> E -> 256 -> one scalar head (gauss: mean and log-std).  E is the caller's to test.
inline int check_actor(const Mlp& actor, int obs_dim, int gauss) {
    if (actor.hd > 1 || actor.S != obs_dim || actor.A != 0 || actor.n_out != (gauss ? 2 : 1) || actor.cat || actor.H != 256 || !actor.Ws ||
        !actor.W0 || !actor.W1 || (gauss && !actor.W1b))
        return RPO_ERR_ARG;
    return 0;
}

// A critic of the row-tile kernels: (obs_dim, 2) -> E -> 256 -> Q.  E: the width it has to have; tiled: and that has to be one the
// row tiles are instantiated for; hd: whether head_dim is tested too.  The entry points differ in all three, and say so here.
inline int check_critic(const Mlp& q, int obs_dim, int E, bool tiled, bool hd) {
    if (q.S != obs_dim || q.A != 2 || q.cat || q.H != 256 || q.n_out != 1 || (hd && q.hd > 1)) return RPO_ERR_ARG;
    if (q.E != E || (tiled && E != 128 && E != 256)) return RPO_ERR_ARG;
    return 0;
}

// The step range of every *_evaluate* entry point (evaluate.hip, evopf_eval.hip)
inline int check_eval_range(int n, int t0, int steps, int max_episode_steps, int max_steps) {
    if (n <= 0 || t0 < 0 || steps <= 0 || max_episode_steps <= 0 || max_steps < 0) return RPO_ERR_ARG;
    if ((long long)t0 + steps > (1ll << 24)) return RPO_ERR_ARG;   // lengths and step indices stay exact in the f32 row
    return 0;
}

// The per-constraint report of the evaluation entry points that take one: 16-byte aligned for the float4 accesses.
inline int check_eval_con(const float* con) {
    if (!con) return RPO_ERR_NULL;
    return reinterpret_cast<uintptr_t>(con) % 16 ? RPO_ERR_ARG : 0;
}

// A stage's kernel: its CartSafe and its SpringPendulum instantiation
template <class C, class P> struct EnvKernels { C* cart; P* pend; };
template <class C, class P> constexpr EnvKernels<C, P> env_kernels(C* cart, P* pend) { return EnvKernels<C, P>{cart, pend}; }

// The env dispatch: the CartSafe (env 0) or the SpringPendulum instantiation of a stage's kernel
template <class C, class P, class... A>
int launch_env(const EnvKernels<C, P>& k, int env, dim3 grid, int threads, void* stream, const A&... args) {
    return env == 0 ? launch(k.cart, grid, threads, 0, stream, args...) : launch(k.pend, grid, threads, 0, stream, args...);
}

// A row-tile kernel: its E = 128 and its E = 256 instantiation
template <class K> struct EmbedKernels { K* e128; K* e256; };
template <class K> constexpr EmbedKernels<K> embed_kernels(K* e128, K* e256) { return EmbedKernels<K>{e128, e256}; }

// The embedding-width dispatch; any other width is refused here, behind the caller's other checks
template <class K, class... A>
int launch_embed(const EmbedKernels<K>& k, int E, dim3 grid, int threads, void* stream, const A&... args) {
    if (E == 128) return launch(k.e128, grid, threads, 0, stream, args...);
    if (E == 256) return launch(k.e256, grid, threads, 0, stream, args...);
    return RPO_ERR_ARG;
}

}  // namespace rpo_host
