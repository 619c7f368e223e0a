// The policy_act launch (act.hip, trainer.act()) in its STREAMING form: rollout_stream_kernel's structure (rollout_stream.hip) with
// the env step and everything carried between steps removed -- one pass over n rows.  One persistent workgroup per CU stages
// the actor's hidden matrix into LDS once (stream_stage), every WAVE owns whole 16-row tiles (stream_tile: both layers transposed
// on the matrix cores, the next tile's inputs requested under the current tile's MFMAs, no barrier after the staging), the tile's
// outputs stay in the wave's LDS slot, and after G tiles one thread per row runs head -> Complete -> GRG -> residuals -> stores
// (act_dev.h) OUT OF LINE with its parameters read from an LDS copy.  No Philox, no episode bookkeeping, no ring row, no
// statistics, no arrival counting, no ctrl.  A translation unit of its own because it is compiled with -fno-slp-vectorize like
// rollout_stream.hip (packed f32 VALU beside f32 MFMAs: see that file's header).
#include "act_dev.h"
#include "mlp_stream.h"

namespace {

using namespace rpo_mlp_dev;

struct ActStreamIn {                                             // what stream_inputs / stream_tile read (mlp.hip's FwdArgs)
    Mlp net;
    int n;
    const float* s; int s_stride;
    const float* a; int a_stride;
    float* out; float* x0_save; float* h1_save;
    int out_mode; float scale, base;
};
struct ActKeep {                                                 // EMIT of stream_tile: the outputs of row `row` -> the wave's slot
    float* slot;
    int row0;
    __device__ __forceinline__ void operator()(int row, float o0, float o1, bool two) const {
        slot[(row - row0) * 2] = o0;
        slot[(row - row0) * 2 + 1] = two ? o1 : 0.0f;
    }
};
constexpr int kActStreamWaves = 16;

// The per-row phase reads the launch parameters from a copy in LDS through a pointer the optimiser cannot see through (as
// kernel arguments they stay live across the MFMA loops: rollout_stream.hip).
template <class ENV>
struct ActStreamParams {
    PolicyActArgs<ENV> p;
    typename ENV::Consts c;
};

template <class ENV, int G>
__device__ __attribute__((noinline)) void act_stream_rows(const ActStreamParams<ENV>* par, const float* slot, int grow0, int lane) {
    const PolicyActArgs<ENV>& p = par->p;
    const int i = grow0 + lane;
    if (lane < kRows * G && i < p.n) {
        float obs[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) obs[q] = 0.0f;
        if (!std::is_same<ENV, CartEnv>::value) {                // (CartSafe's projection and residuals do not read the state)
#pragma unroll
            for (int q = 0; q < ENV::OBS; ++q) obs[q] = p.obs[(size_t)i * p.obs_stride + q];
        }
        policy_act_row<ENV>(p, par->c, obs, i, slot[lane * 2], slot[lane * 2 + 1]);
    }
}

template <class ENV, int G>
__global__ __launch_bounds__(kActStreamWaves * 64, kActStreamWaves / 4) void policy_act_stream_kernel(PolicyActArgs<ENV> p_in,
                                                                                                    typename ENV::Consts c_in) {
    constexpr int H = 256, NW = kActStreamWaves, kGroup = kRows * G;
    __shared__ StreamLds<H> lds;
    __shared__ float out_s[NW][kGroup * 2];
    __shared__ ActStreamParams<ENV> par_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = p_in.n;
    const ActStreamIn in{p_in.actor, n, p_in.obs, p_in.obs_stride, nullptr, 0, nullptr, nullptr, nullptr, p_in.gauss ? 0 : 1, p_in.scale, p_in.base};
    const bool gauss = p_in.gauss != 0;
    stream_stage<H, NW>(p_in.actor, lds, tid);
    if (tid == 0) { par_s.p = p_in; par_s.c = c_in; }
    __syncthreads();
    const float b1a = p_in.actor.b1[0], b1b = gauss ? p_in.actor.b1b[0] : 0.0f;
    const int tiles = (n + kRows - 1) / kRows, groups = (tiles + G - 1) / G;
    const int g0 = blockIdx.x * NW + wave, dg = gridDim.x * NW;
    float in3[3] = {0.0f, 0.0f, 0.0f};
    if (g0 < groups) stream_inputs(in, (long long)g0 * kGroup, lane, in3);
    for (int g = g0; g < groups; g += dg) {
        const int grow0 = g * kGroup;
        const ActKeep keep{&out_s[wave][0], grow0};
#pragma unroll 1
        for (int q = 0; q < G; ++q) {
            const int row0 = grow0 + q * kRows;
            // the next tile's inputs land under this tile's MFMAs (rows beyond n: a clamped row, never used)
            const long long nrow0 = q + 1 < G ? (long long)row0 + kRows : (g + dg < groups ? (long long)(g + dg) * kGroup : (long long)row0);
            float nxt[3];
            stream_inputs(in, nrow0, lane, nxt);
            if (row0 < n) {
                if (row0 + kRows <= n) {
                    if (gauss) stream_tile<H, true, 2, 0, 1>(in, lds, row0, lane, b1a, b1b, in3, keep);
                    else stream_tile<H, true, 2, 0, 0>(in, lds, row0, lane, b1a, b1b, in3, keep);
                } else {
                    stream_tile_any<H, 2>(in, lds, row0, lane, b1a, b1b, in3, keep);
                }
            }
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) in3[ks] = nxt[ks];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the slot is written and read by lanes of ONE wave)
        __builtin_amdgcn_wave_barrier();
        act_stream_rows<ENV, G>(&par_s, &out_s[wave][0], grow0, lane);
    }
}

template <class ENV>
int launch_act_stream(const void* args_v, const void* consts_v, int g4, void* stream) {
    const PolicyActArgs<ENV>& args = *static_cast<const PolicyActArgs<ENV>*>(args_v);
    const typename ENV::Consts& c = *static_cast<const typename ENV::Consts*>(consts_v);
    const Mlp& a = args.actor;
    if (!stream_shape_ok(a) || a.A != 0 || (reinterpret_cast<uintptr_t>(a.W0) & 15u) != 0) return -1;
    const int group = (g4 ? 4 : 1) * kRows;
    const int groups = (args.n + group - 1) / group;
    int gx = (groups + kActStreamWaves - 1) / kActStreamWaves;
    if (gx > rpo_cu_count()) gx = rpo_cu_count();
    if (g4) hipLaunchKernelGGL((policy_act_stream_kernel<ENV, 4>), dim3(gx), dim3(kActStreamWaves * 64), 0, (hipStream_t)stream, args, c);
    else hipLaunchKernelGGL((policy_act_stream_kernel<ENV, 1>), dim3(gx), dim3(kActStreamWaves * 64), 0, (hipStream_t)stream, args, c);
    RPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int rpo_act_stream_launch(int env, const void* args, const void* consts, int g4, void* stream) {
    return env == 0 ? launch_act_stream<CartEnv>(args, consts, g4, stream) : launch_act_stream<PendEnv>(args, consts, g4, stream);
}
