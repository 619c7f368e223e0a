// Single-step AC optimal power flow of EVOPF-v0 on the device (EVOPFEnv.opf / opt_solve, EvalTrajectory.opf_gap): the cheapest
// dispatch (pg, qg, vm, va) that meets the 28 power-balance equations and the 48 bounds on pg, qg, vm for a given demand and a
// given battery power pe -- the problem the reference hands to pypower's interior-point solver once per state on the CPU
// (evopf.py:729-759).  ONE WAVEFRONT PER STATE, four states per workgroup, float32 throughout (geometry and workspace of evopf.hip).
//
// Method: primal-dual interior point in the form of MATPOWER's MIPS (Wang, Murillo-Sanchez, Zimmerman, Thomas 2007; MATPOWER
// manual app. A) with slacks z on the bounds, multipliers mu, lambda and the barrier parameter gamma; the update formulas stand
// at their lines below.  The flat start (middle of every box, angles 0, z = max(-h, 1), mu = gamma / z, lambda = 0, gamma = 1),
// sigma = 0.1, xi = 0.99995 and the stop test (max(|g|_inf, max h), |L_x|_inf and z^T mu all below tol, unscaled) are those of
// tests/evopf_opf_f64.py, the float64 yardstick, which solves the full 65 x 65 system with LAPACK.
//
// The KKT system here: the ten generator variables enter g through a selection matrix and have a diagonal block D in M (2 c2 +
// Sigma for pg, Sigma for qg), so they are eliminated by hand -- [[H_vv, J_v^T], [J_v, -S D^-1 S^T]] of order 27 + 28 = 55, ONE
// ROW PER LANE: lanes 0..13 the vm rows, 14..26 the va rows of buses 1..13, 27..54 the equations.  A lane evaluates its own row
// (Hessian row from the textbook second derivatives of the polar power-flow equations; the Jacobian entries are evopf_dev.h's
// jac_entry, read by row in the equation lanes and by column in the variable lanes), keeps it in 56 registers and the wave
// eliminates it by Gauss-Jordan with a dynamic pivot per column (the matrix is symmetric indefinite and its (2, 2) block has
// zeros on the diagonal at the load buses): evopf_dev.h's gj_dynamic, the routine of the 28-row systems' fallback, with the
// pivot picker for rows in all 64 lanes (PickExact64) -- rows are not swapped, every lane remembers the unknown its row ended
// up solving.  The lane that owns a bounded variable (vm lanes; the equation lane of a generator bus owns
// that generator's pg or qg) keeps its two slacks and two multipliers in registers; x lives in w.a, lambda in w.dir, the
// solution passes through w.vec.  Nothing else is shared, and nothing outside the workspace is written but the two outputs --
// and, through rpo_evopf_opf_state, the iterate itself: state_in replaces the flat start, state_out receives the state at exit
// (two wave-uniform branches outside the loop), which is how tests/test_evopf_opf_f64_gpu.py holds the loop one iteration at a time.
//
// eq_resid is injection minus flow: with F = lambda_p^T P + lambda_q^T Q = sum_ik V_i V_k c_ik, the Hessian of lambda^T g is -F''.
//   th = va_i - va_k,  G_ik = Yr[k][i], B_ik = Yi[k][i] (flows() multiplies the voltage ROW vector into Ybus)
//   a = G cos th + B sin th,  b = G sin th - B cos th           (P_i = V_i sum_k V_k a_ik,  Q_i = V_i sum_k V_k b_ik)
//   c = lp_i a + lq_i b,      d = dc / dth = -lp_i b + lq_i a    (dd / dth = -c);   cs = c + c^T,  dd = d - d^T
//   F_VmVn = cs_mn;   F_thm,thn = V_m V_n cs_mn - [m == n] V_m sum_k cs_mk V_k;   F_thm,Vn = [m == n] sum_k dd_mk V_k + V_m dd_mn
// A state that does not converge leaves at max_iters: every loop has a compile-time or max_iters bound, overflowing quotients
// only produce infinities and NaNs (a NaN in a stop quantity means "not converged").
#include "evopf_dev.h"
#include "launch.h"

using namespace rpo_evopf_dev;
using rpo_host::launch;

namespace {

constexpr int kOpfWaves = 4;                 // states per workgroup, one wave each
constexpr int NV = 2 * NB - 1;               // voltage unknowns: vm[14], va at the 13 non-slack buses (bus 0 is the slack)
constexpr int NK = NV + NEQ;                 // order of the reduced KKT system
constexpr int NBOUND = 2 * (2 * NG + NB);    // 48 inequalities
constexpr int NBOUND_FREE = NBOUND + 2 * NE; // ... and the 10 battery bounds of the free-pe instance: 58
constexpr float kSigma = 0.1f, kXi = 0.99995f, kZ0 = 1.0f, kGamma0 = 1.0f;
static_assert(NK + NE <= RPO_WAVE, "one row of the reduced KKT system per lane, and a lane per battery behind them");

struct OpfArgs {
    int n;
    const float* obs;
    int obs_stride;
    const float* pe;          // [n, 5] or NULL (zeros); the free-pe instance: pe_cost [n, 5] or NULL ((kWe / kWg) * price of the row)
    float* action;            // [n, 43]
    float* info;              // [n, 4]: cost, largest stop quantity at exit, iterations, converged
    float tol;
    int max_iters;
    const float* consts;
    const float* state_in;    // [n, RPO_EVOPF_OPF_STATE] or NULL (the flat start)
    float* state_out;         // [n, RPO_EVOPF_OPF_STATE] or NULL
    // the nearest-feasible instance alone (behind everything else: the other instances' arguments stay where they were)
    const float* target;      // [n, >= 43] rows in the layout of an action; the 14 controlled components are read
    int target_stride;
    const float* weight;      // [14] (weight_stride 0), [n, 14] (weight_stride 14) or NULL (1 / half-width^2 of the variable's box)
    int weight_stride;
};
// a row of the state: action[43] | lambda[28] | z_u[24] | z_l[24] | mu_u[24] | mu_l[24] | gamma, the bounded variables in the
// order pg[5], qg[5], vm[14]
constexpr int kStLam = NY, kStZu = kStLam + NEQ, kStBnd = NBOUND / 2, kStGamma = kStZu + 4 * kStBnd;
static_assert(kStGamma + 1 == RPO_EVOPF_OPF_STATE, "layout of the state row");

// kSpv[j] for a lane-dependent j.  Selects on literals, not a read of kSpv: a second kind of use of that table in this module
// moves the compiler's choices in the fixed-pe instance too (its instructions are pinned, see below).
__device__ __forceinline__ int bus_of_battery(int j) {
    static_assert(NE == 5 && kSpv[0] == 0 && kSpv[1] == 1 && kSpv[2] == 2 && kSpv[3] == 5 && kSpv[4] == 7, "battery j sits at bus kSpv[j]");
    return j == 4 ? 7 : (j == 3 ? 5 : j);
}

// bus -> its generator, -1 at a load bus; literals for the same reason
__device__ __forceinline__ int gen_of_bus(int b) { return b == 7 ? 4 : (b == 5 ? 3 : (b <= 2 ? b : -1)); }

// FREE_PE: the battery power is a variable too (rpo_evopf_opf_free).  pe_j enters g like pg_j -- linearly, in the real-power
// equation of bus kSpv[j] alone, with d g / d pe = +1 (eq_resid adds pg + pe; NOT jac_entry's -1, the reference's eq_jac sign,
// DESIGN hazard E1) -- has no Hessian and a box, battery_bounds(soc) of the row's observation: it is eliminated by hand like the
// generator variables.  Lane NK + j owns pe_j (x, box, the four slack / multiplier registers every bounded lane has);
// L_x = pe_cost_j + lambda_e + (mu_u - mu_l), D = Sigma, N = L_x + barrier part.  The equation lane of that bus, which owns pg_j,
// reads 1 / D_pe and N_pe / D_pe from it (two lane reads) for kdiag = -(1 / D_pg + 1 / D_pe) and rhs = N_pg / D_pg + N_pe / D_pe
// - g_e; after the solve lane NK + j reads dlambda_e from w.vec and forms dpe = (-N_pe - dlambda_e) / D_pe.  58 inequalities.
// No state seam (state_in / state_out are not read).  The FREE_PE = false instance is the kernel as it stood, instruction for
// instruction: every addition below folds away on a compile-time false.
//
// NEAREST (with FREE_PE: its variables and its 58 bounds, unchanged): the safety filter, rpo_evopf_nearest.  The objective is
// 0.5 sum_k w_k (y_k - t_k)^2 over the 14 components the actor controls (pg of generators 1..4, vm at the five generator buses,
// pe[5]) in place of the generation cost -- every one of them a bounded variable a lane already owns.  pg and pe are eliminated by
// hand, so the objective enters through their c2 = w (D = w + Sigma) and L_x = w (x - t) + lambda_e + (mu_u - mu_l); a vm lane of
// a generator bus adds w to its diagonal entry and w (x - t) to its L_x.  w: the row of the weight table, or 1 / s^2 with s the
// half-width of the lane's own box (hi, lo above; per row for pe), 0 where s <= 1e-6.  A weight that is not a finite number > 0
// becomes a NaN, which ends its row "not converged" like a NaN in the target or the observation.  The start stays the flat one.
// info[0] is the objective at exit.  The other two instances fold every line of it away.
template <bool FREE_PE, bool NEAREST = false>
__global__ __launch_bounds__(RPO_WAVE * kOpfWaves) void evopf_opf_kernel(OpfArgs p) {
    __shared__ Ws wss[kOpfWaves];
    Ws& w = wss[threadIdx.x / RPO_WAVE];
    const int i = blockIdx.x * kOpfWaves + threadIdx.x / RPO_WAVE, tid = lane_id();
    if (i >= p.n) return;                                       // (whole waves: only wave-level hand-overs below)
    load_consts(w, p.consts);
    // pd, qd: all the fixed-pe problem reads of the observation; free pe: the whole row (state of charge, current price)
    load_row(w.s, p.obs + (size_t)i * p.obs_stride, FREE_PE ? NS : 2 * NB);
    if (tid <= NY) w.a[tid] = 0.0f;
    if (tid < NEQ) w.dir[tid] = 0.0f;                           // lambda
    sync();

    // ---- what the lane owns
    const bool is_var = tid < NV, is_vm = tid < NB, is_eq = tid >= NV && tid < NK;
    const int vbus = is_vm ? tid : (is_var ? tid - (NB - 1) : 0);          // bus of the lane's voltage unknown
    const int myvar = is_vm ? VM0 + vbus : VA0 + vbus;
    const bool is_pe = FREE_PE && tid >= NK && tid < NK + NE;               // free pe: lane NK + j owns pe_j ...
    const int bat = is_pe ? tid - NK : 0;
    // the lane's equation (a battery lane: the real-power equation of its bus)
    const int e = is_eq ? tid - NV : (FREE_PE ? (is_pe ? bus_of_battery(bat) : 0) : 0);
    const bool e_real = e < NB;
    const int ebus = e_real ? e : e - NB;
    int gen = -1;
#pragma unroll
    for (int j = 0; j < NG; ++j) gen = kSpv[j] == ebus ? j : gen;
    const bool has_u = is_eq && gen >= 0;                                   // the equation's generator variable: pg / qg
    const bool is_pg = has_u && e_real;
    const bool elim = has_u || is_pe;                                       // the lane owns a variable eliminated by hand
    const bool bounded = is_vm || elim;
    const int xidx = is_var ? myvar : (has_u ? (e_real ? PG0 + gen : QG0 + gen) : (is_pe ? PE0 + bat : NY));   // w.a component the lane updates (NY: none)
    float hi = 0.0f, lo = 0.0f;
    if (is_vm) { hi = w.c[RPO_EVOPF_C_VMAX + vbus]; lo = w.c[RPO_EVOPF_C_VMIN + vbus]; }
    else if (is_pg) { hi = w.c[RPO_EVOPF_C_PMAX + gen]; lo = w.c[RPO_EVOPF_C_PMIN + gen]; }
    else if (has_u) { hi = w.c[RPO_EVOPF_C_QMAX + gen]; lo = w.c[RPO_EVOPF_C_QMIN + gen]; }
    else if (is_pe) battery_bounds(w.s[2 * NB + bat], hi, lo);
    // nearest: the lane's place among the 14 controlled components (the env's partial_actions order), its target and weight
    float tk = 0.0f, wq = 0.0f;
    bool ctrl = false;
    if constexpr (NEAREST) {
        const int vgen = gen_of_bus(vbus);
        const int k = (is_pg && gen >= 1) ? gen - 1 : ((is_vm && vgen >= 0) ? NG - 1 + vgen : (is_pe ? 2 * NG - 1 + bat : -1));
        ctrl = k >= 0;
        if (ctrl) {
            tk = p.target[(size_t)i * p.target_stride + xidx];
            if (p.weight) {
                const float v = p.weight[(size_t)i * p.weight_stride + k];
                wq = (v > 0.0f && v < __builtin_inff()) ? v : __builtin_nanf("");
            } else {
                const float half = 0.5f * (hi - lo);
                wq = half > 1e-6f ? 1.0f / (half * half) : 0.0f;
            }
        }
    }
    const int bidx = is_vm ? 2 * NG + vbus : (is_pg ? gen : NG + gen);    // the lane's bounded variable in the state row's order
    const float c2 = NEAREST ? (elim ? wq : 0.0f) : (is_pg ? 2.0f * w.c[RPO_EVOPF_C_QUAD + gen] : 0.0f);
    // linear cost: pe_cost_j of the battery lanes, by default what the env's reward charges for a unit of pe in units of obj_fn
    const float c1 = NEAREST ? 0.0f : (is_pg ? w.c[RPO_EVOPF_C_LIN + gen]
                           : (is_pe ? (p.pe ? p.pe[(size_t)i * NE + bat] : (kWe / kWg) * w.s[2 * NB + NE]) : 0.0f));

    // ---- flat start
    {
        const float x0 = 0.5f * (hi + lo);                                  // (0 for the angles)
        if (xidx < NY) w.a[xidx] = x0;
        if (!FREE_PE && tid < NE) w.a[PE0 + tid] = p.pe ? p.pe[(size_t)i * NE + tid] : 0.0f;
        if (tid == 32) w.a[VA0] = w.c[RPO_EVOPF_C_VA_INIT];                 // slack_va (bus 0)
    }
    float zu = 1.0f, zl = 1.0f, mu_u = 0.0f, mu_l = 0.0f, gamma = kGamma0;
    if (bounded) {
        const float x0 = 0.5f * (hi + lo);
        zu = fmaxf(hi - x0, kZ0); zl = fmaxf(x0 - lo, kZ0);
        mu_u = gamma / zu; mu_l = gamma / zl;
    }
    if (!FREE_PE && p.state_in) {                               // a given state replaces the flat start entirely
        const float* st = p.state_in + (size_t)i * RPO_EVOPF_OPF_STATE;
        if (tid < NY) w.a[tid] = st[tid];
        if (tid < NEQ) w.dir[tid] = st[kStLam + tid];
        if (bounded) {
            zu = st[kStZu + bidx]; zl = st[kStZu + kStBnd + bidx];
            mu_u = st[kStZu + 2 * kStBnd + bidx]; mu_l = st[kStZu + 3 * kStBnd + bidx];
        }
        gamma = st[kStGamma];
    }
    sync();

    int it = 0;
    bool converged = false;
    float resid = 0.0f;
    for (;;) {
        flows(w);
        eq_resid(w);                                             // g in w.eq
        const float x = w.a[xidx];
        const float hu = bounded ? x - hi : -1.0f, hl = bounded ? lo - x : -1.0f;
        // bound terms: Sigma, the barrier part of N, mu_u - mu_l
        const float sig = bounded ? mu_u / zu + mu_l / zl : 0.0f;
        const float nbar = bounded ? (mu_u * hu + gamma) / zu - (mu_l * hl + gamma) / zl : 0.0f;
        const float dmu = mu_u - mu_l;
        // generator variable of an equation lane: L_x, D, N of that variable; its column is eliminated into the lane's diagonal
        const float lam_e = w.dir[e], g_e = is_eq ? w.eq[e] : 0.0f;
        const float lxu = elim ? (NEAREST ? c2 * (x - tk) : c2 * x + c1) + lam_e + dmu : 0.0f;   // (nearest: the difference first, it is small)
        const float du = elim ? c2 + sig : 1.0f;
        const float nu = lxu + nbar;
        const float kdiag = has_u ? -1.0f / du : 0.0f;

        // Hessian coefficients of the lane's bus m against every bus n
        float csn[NB], ddn[NB], vmag[NB], csv = 0.0f, dv = 0.0f;
        const float vm_m = w.a[VM0 + vbus];
        {
            const float lpm = w.dir[vbus], lqm = w.dir[NB + vbus], cm = w.cs[vbus], sm = w.sn[vbus];
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                const bool same = vbus == n;
                const float cn = w.cs[n], sn = w.sn[n];
                const float C = same ? 1.0f : cm * cn + sm * sn, S = same ? 0.0f : sm * cn - cm * sn;
                const float gmn = Yr(w, n, vbus), bmn = Yi(w, n, vbus), gnm = Yr(w, vbus, n), bnm = Yi(w, vbus, n);
                const float amn = gmn * C + bmn * S, bbmn = gmn * S - bmn * C;
                const float anm = gnm * C - bnm * S, bbnm = -gnm * S - bnm * C;
                const float lpn = w.dir[n], lqn = w.dir[NB + n];
                const float cmn = lpm * amn + lqm * bbmn, cnm = lpn * anm + lqn * bbnm;
                const float dmn = -lpm * bbmn + lqm * amn, dnm = -lpn * bbnm + lqn * anm;
                csn[n] = cmn + cnm;
                ddn[n] = dmn - dnm;
                vmag[n] = w.a[VM0 + n];
                csv = fmaf(csn[n], vmag[n], csv);
                dv = fmaf(ddn[n], vmag[n], dv);
            }
        }

        // ---- the lane's row of [[H_vv + Sigma, J_v^T], [J_v, -S D^-1 S^T]] | rhs
        float row[NK + 1];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const bool col_vm = c < NB;
            const int n = col_vm ? c : c - (NB - 1);
            const int var = col_vm ? VM0 + n : VA0 + n;
            float v = 0.0f;
            if (is_var) {                                        // minus the second derivatives of F
                const bool same = vbus == n;
                if (is_vm) v = col_vm ? -csn[n] : (same ? -dv : vmag[n] * ddn[n]);
                else v = col_vm ? -((same ? dv : 0.0f) + vm_m * ddn[n]) : (same ? vm_m * csv : 0.0f) - vm_m * vmag[n] * csn[n];
                if (is_vm && tid == c) v += NEAREST ? sig + wq : sig;
            } else if (is_eq) {
                v = jac_entry(w, e, var);
            }
            row[c] = v;
        }
        float jtl = 0.0f;                                        // (J^T lambda) of the lane's voltage unknown
#pragma unroll
        for (int c = NV; c < NK; ++c) {
            float v = 0.0f;
            if (is_var) {
                v = jac_entry(w, c - NV, myvar);
                jtl = fmaf(v, w.dir[c - NV], jtl);
            } else if (tid == c) {
                v = kdiag;
            }
            row[c] = v;
        }
        const float lxv = is_var ? jtl + (is_vm ? (NEAREST ? dmu + wq * (x - tk) : dmu) : 0.0f) : 0.0f;   // L_x of the voltage unknown
        const float nv = lxv + (is_vm ? nbar : 0.0f);
        row[NK] = is_var ? -nv : (is_eq ? (has_u ? nu / du - g_e : -g_e) : 0.0f);
        if constexpr (FREE_PE) {
            // the pg lane of bus kSpv[j] takes pe_j's share from lane NK + j (two lane reads): kdiag = -(1 / D_pg + 1 / D_pe),
            // rhs = N_pg / D_pg + N_pe / D_pe - g_e.  Here, after the rows are built, where fewer registers are live.
            const int src = (NK + (is_pg ? gen : 0)) << 2;
            const float inv_pe = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(1.0f / du)));
            const float n_pe = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(nu / du)));
#pragma unroll
            for (int j = 0; j < NE; ++j) row[NV + bus_of_battery(j)] -= (is_pg && gen == j) ? inv_pe : 0.0f;
            row[NK] += is_pg ? n_pe : 0.0f;
        }

        // ---- stop test: max(|g|_inf, max h), |L_x|_inf, z^T mu
        const float feas_l = fmaxf(fabsf(g_e), bounded ? fmaxf(hu, hl) : 0.0f);
        const float grad_l = is_var ? fabsf(lxv) : fabsf(lxu);
        const float comp_l = bounded ? zu * mu_u + zl * mu_l : 0.0f;
        const float comp = rpo_wave_sum_rows(comp_l);
        const bool nan_l = g_e != g_e || hu != hu || lxv != lxv || lxu != lxu || comp != comp;
        const bool any_nan = __builtin_amdgcn_ballot_w64(nan_l) != 0ull;
        resid = fmaxf(fmaxf(rpo_wave_max_nonneg(fmaxf(feas_l, 0.0f)), rpo_wave_max_nonneg(grad_l)), comp);
        if (any_nan) resid = __builtin_nanf("");
        converged = !any_nan && resid < p.tol;
        if (converged || it >= p.max_iters) break;

        // ---- (dv, dlambda), then the eliminated generator steps, slacks and multipliers
        // (the pivot of column k: the largest |entry| among the rows that own none yet, PickExact64; on return the lane's row
        //  solves unknown `mycol`)
        int mycol;
        const float mypiv = gj_dynamic<0, NK, 0, NK + 1, PickExact64>(row, mycol);
        if (tid < NK) w.vec[mycol] = row[NK] / mypiv;
        sync();
        const float delta = w.vec[tid < NK ? tid : (is_pe ? NV + e : 0)];
        const float dlam = (is_eq || is_pe) ? delta : 0.0f;
        const float dx = is_var ? delta : (elim ? (-nu - dlam) / du : 0.0f);
        const float dzu = -hu - zu - dx, dzl = -hl - zl + dx;                   // dz = -h - z - dh
        const float dmu_u = -mu_u + (gamma - mu_u * dzu) / zu, dmu_l = -mu_l + (gamma - mu_l * dzl) / zl;
        // step lengths to the boundary times xi, capped at 1: xi * min(z / -dz) = xi / max(-dz / z)
        const float qp = rpo_wave_max_nonneg(bounded ? fmaxf(fmaxf(-dzu / zu, -dzl / zl), 0.0f) : 0.0f);
        const float qd = rpo_wave_max_nonneg(bounded ? fmaxf(fmaxf(-dmu_u / mu_u, -dmu_l / mu_l), 0.0f) : 0.0f);
        const float alpha_p = qp > 0.0f ? fminf(kXi / qp, 1.0f) : 1.0f;
        const float alpha_d = qd > 0.0f ? fminf(kXi / qd, 1.0f) : 1.0f;
        if (xidx < NY) w.a[xidx] = x + alpha_p * dx;
        if (is_eq) w.dir[e] = lam_e + alpha_d * dlam;
        if (bounded) {
            zu += alpha_p * dzu; zl += alpha_p * dzl;
            mu_u += alpha_d * dmu_u; mu_l += alpha_d * dmu_l;
        }
        gamma = kSigma * rpo_wave_sum_rows(bounded ? zu * mu_u + zl * mu_l : 0.0f) / (float)(FREE_PE ? NBOUND_FREE : NBOUND);
        sync();
        ++it;
    }

    // ---- outputs: the full 43-vector (slack angle as given; pe as given, or the optimal one) and (cost, residual, iterations, converged)
    float part = 0.0f;
    if (tid < NG) {
        const float pg = w.a[PG0 + tid];
        part = w.c[RPO_EVOPF_C_QUAD + tid] * pg * pg + w.c[RPO_EVOPF_C_LIN + tid] * pg;
    }
    float cost = rpo_wave_sum_rows(part) + w.c[RPO_EVOPF_C_CONST];
    if constexpr (NEAREST) {
        const float d = w.a[xidx] - tk;
        cost = rpo_wave_sum_rows(ctrl ? 0.5f * wq * d * d : 0.0f);
    }
    if (tid < NY) p.action[(size_t)i * NY + tid] = w.a[tid];
    if (tid < 4) p.info[(size_t)i * 4 + tid] = tid == 0 ? cost : (tid == 1 ? resid : (tid == 2 ? (float)it : (converged ? 1.0f : 0.0f)));
    if (!FREE_PE && p.state_out) {                                     // the state the stop test was last evaluated on
        float* st = p.state_out + (size_t)i * RPO_EVOPF_OPF_STATE;
        if (tid < NY) st[tid] = w.a[tid];
        if (tid < NEQ) st[kStLam + tid] = w.dir[tid];
        if (bounded) {
            st[kStZu + bidx] = zu; st[kStZu + kStBnd + bidx] = zl;
            st[kStZu + 2 * kStBnd + bidx] = mu_u; st[kStZu + 3 * kStBnd + bidx] = mu_l;
        }
        if (tid == 0) st[kStGamma] = gamma;
    }
}

}  // namespace

extern "C" int rpo_evopf_opf(int n, const float* obs, int obs_stride, const float* pe, float* action_out, float* info_out, float tol,
                             int max_iters, const float* consts_dev, void* stream) {
    return rpo_evopf_opf_state(n, obs, obs_stride, pe, action_out, info_out, tol, max_iters, consts_dev, nullptr, nullptr, stream);
}

extern "C" int rpo_evopf_opf_state(int n, const float* obs, int obs_stride, const float* pe, float* action_out, float* info_out,
                                   float tol, int max_iters, const float* consts_dev, const float* state_in, float* state_out,
                                   void* stream) {
    if (n <= 0 || max_iters < 0 || !(tol > 0.0f) || obs_stride < 2 * NB || (state_in && pe)) return RPO_ERR_ARG;
    if (!obs || !action_out || !info_out || !consts_dev) return RPO_ERR_NULL;
    const OpfArgs args{n, obs, obs_stride, pe, action_out, info_out, tol, max_iters, consts_dev, state_in, state_out, nullptr, 0, nullptr, 0};
    return launch(evopf_opf_kernel<false>, dim3((n + kOpfWaves - 1) / kOpfWaves), RPO_WAVE * kOpfWaves, 0, stream, args);
}

extern "C" int rpo_evopf_opf_free(int n, const float* obs, int obs_stride, const float* pe_cost, float* action_out, float* info_out,
                                  float tol, int max_iters, const float* consts_dev, void* stream) {
    if (n <= 0 || max_iters < 0 || !(tol > 0.0f) || obs_stride < NS) return RPO_ERR_ARG;
    if (!obs || !action_out || !info_out || !consts_dev) return RPO_ERR_NULL;
    const OpfArgs args{n, obs, obs_stride, pe_cost, action_out, info_out, tol, max_iters, consts_dev, nullptr, nullptr, nullptr, 0, nullptr, 0};
    return launch(evopf_opf_kernel<true>, dim3((n + kOpfWaves - 1) / kOpfWaves), RPO_WAVE * kOpfWaves, 0, stream, args);
}

extern "C" int rpo_evopf_nearest(int n, const float* obs, int obs_stride, const float* target, int target_stride, const float* weight,
                                 int weight_stride, float* action_out, float* info_out, float tol, int max_iters,
                                 const float* consts_dev, void* stream) {
    if (n <= 0 || max_iters < 0 || !(tol > 0.0f) || obs_stride < NS || target_stride < NY || (weight_stride != 0 && weight_stride != NP))
        return RPO_ERR_ARG;
    if (!obs || !target || !action_out || !info_out || !consts_dev) return RPO_ERR_NULL;
    const OpfArgs args{n, obs, obs_stride, nullptr, action_out, info_out, tol, max_iters, consts_dev, nullptr, nullptr, target, target_stride,
                       weight, weight_stride};
    return launch(evopf_opf_kernel<true, true>, dim3((n + kOpfWaves - 1) / kOpfWaves), RPO_WAVE * kOpfWaves, 0, stream, args);
}
