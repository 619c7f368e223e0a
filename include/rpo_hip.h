/*
 * rpo_hip.h -- C ABI of librpo_hip.so: the MI355X (gfx950) kernels behind the RPO rollout-collection +
 * constrained-policy-update hot path.
 *
 * The reference (wadx2019/rpo) is pure Python and has NO native / FFI boundary: its seam is the
 * duck-typed Python interface between `rpo/algo` trainers and `rpo/env` constraint oracles.  This header is the
 * C boundary this build puts underneath that interface.  Every entry point names the reference code it replaces
 * (paths relative to the reference root); INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - the caller owns all memory (PyTorch tensors in the shipped host code); nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous and capturable in a hipGraph: all
 *     per-iteration varying quantities (vector-step counter, ring position, Adam step) live in device memory;
 *   - return value: 0 = ok, RPO_ERR_* (<0) = rejected arguments, >0 = hipError_t of the failed launch;
 *   - re-entrant per stream; no hidden global state.
 *
 * Layouts (all float32 unless stated)
 *   CartSafe-v0      state row  [6]  = (x, x_dot, xacc, theta, theta_dot, thetaacc)       cartpole.py:206
 *                    action row [2]  ; basic ("partial") action index = consts.partial     cartpole.py:117
 *                    transition row [24] = s[6] a[2] s'[6] r done eq_viol[1] ineq_viol[6] pad   (ReplayBuffer keys,
 *                                                                       rpo/algo/agent/ddpg_pa.py:70-71)
 *   SpringPendulum-v0 internal row [4] = (theta, theta_dot, l, l_dot)                      pendulum.py:126
 *                    obs row [5] = (cos theta, sin theta, theta_dot, l, l_dot)             pendulum.py:138-140
 *                    transition row [16] = obs[5] a[2] obs'[5] r done eq_viol[1] ineq_viol[1]
 *   replay ring      rows [cap_steps * n_envs, W]; vector step t writes rows (t % cap_steps) * n_envs + lane.
 *   ctrl             int64[RPO_CTRL_LEN]; ctrl[RPO_CTRL_T] = number of vector steps taken so far.  Written only by
 *                    the *_step kernels (last finishing workgroup), read by every kernel that needs t.
 *   stats            float[stats_cap, RPO_STATS_SUB, RPO_STATS_LEN] per-vector-step accumulators, row t % stats_cap;
 *                    the value of a statistic is the sum (max for the *_MAX slots) over the RPO_STATS_SUB sub-rows.
 */
#ifndef RPO_HIP_H
#define RPO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* 3: rpo_split_update gained proj_ws / proj_store_mode / debug (the struct grew); rpo_split_critic_pfront*,
 * rpo_pendulum_project_batchref_ws; rpo_evopf_complete_bwd takes grad_action_b / grad_action2, rpo_evopf_lagrangian takes overwrite;
 * rpo_min_q_bwd, rpo_hw_probe
 * 6: ctrl[RPO_CTRL_NONFINITE] (the step / rollout kernels' sticky failure word) */
#define RPO_ABI_VERSION 6

#define RPO_ERR_ARG (-1)
#define RPO_ERR_NULL (-2)

#define RPO_CART_STATE_DIM 6
#define RPO_CART_ACTION_DIM 2
#define RPO_CART_INEQ 6
#define RPO_CART_ROW 24
#define RPO_CART_RING 32 /* floats between consecutive rows of the REPLAY RING: a 96-byte transition per 128-byte line, so a random
                            row is one line (96-byte spacing: 1.5 lines on average -- gather traffic 1.58 x, round 3); the last
                            8 floats of a ring row are PADDING: the step kernel's full-tile path writes zeros there (whole
                            128-byte lines leave the CU), its partial-tile path leaves them alone, and no kernel reads them.
                            Gathered batches stay RPO_CART_ROW wide.  The stride is compiled into the step / rollout / rider /
                            fused-sampling kernels: a ring must be [rows, RPO_CART_RING] floats (rpo_amd/ops.py refuses others). */
#define RPO_CART_CONSTS_LEN 35 /* C[2] C_p C_o_inv b G[12] d[6] G_r[6] d_r[6], cartpole.py:124-136,397-400 */

#define RPO_PEND_INTERNAL_DIM 4
#define RPO_PEND_OBS_DIM 5
#define RPO_PEND_ACTION_DIM 2
#define RPO_PEND_ROW 16
#define RPO_PEND_RING 16 /* 64-byte rows: two per line, never straddling */

/* EVOPF-v0 (rpo/env/electrical_grid/evopf.py:333-337): observation = pd[14] qd[14] soc[5] price[24]; action = pg[5] qg[5]
 * vm[14] va[14] pe[5]; 14 basic actions = pg at the 4 PV generators, vm at the 5 generator buses, pe[5] (:292-294). */
#define RPO_EVOPF_STATE 57
#define RPO_EVOPF_ACTION 43
#define RPO_EVOPF_PARTIAL 14
#define RPO_EVOPF_EQ 28
#define RPO_EVOPF_INEQ 58
#define RPO_EVOPF_ROW 248 /* state 57 | action 43 | next_state 57 | reward | done | eq_viol 28 | ineq_viol 58 | pad 3 */
/* Constants buffer (device, float32) the host fills from its case tables (rpo_amd/env/electrical_grid/case14.py):
 * Ybus real / imaginary parts row-major (evopf.py:263-266), generator and voltage limits per unit (:251-256), Newton
 * start values (:299-300), cost coefficients already divided by mean(genbase)^2 and multiplied by genbase^(2|1)
 * (obj_fn :509-518), the regularised load curve per hour in per unit of baseMVA (demand.py:48-49), (1 - rho) * nominal
 * load shares and sign(Qd) per bus (demand.py:54-62), the regularised price curve / genbase (price.py:32, evopf.py:57). */
#define RPO_EVOPF_C_YR 0
#define RPO_EVOPF_C_YI 196
#define RPO_EVOPF_C_PMAX 392
#define RPO_EVOPF_C_PMIN 397
#define RPO_EVOPF_C_QMAX 402
#define RPO_EVOPF_C_QMIN 407
#define RPO_EVOPF_C_VMAX 412
#define RPO_EVOPF_C_VMIN 426
#define RPO_EVOPF_C_VM_INIT 440
#define RPO_EVOPF_C_VA_INIT 454
#define RPO_EVOPF_C_QUAD 468
#define RPO_EVOPF_C_LIN 473
#define RPO_EVOPF_C_CONST 478
#define RPO_EVOPF_C_FLAGS 479 /* 1.0f (RPO_EVOPF_STATIC_OK): eliminate in the compiled-in static order of the case14 network (sparse;
                                 falls back to partial pivoting per solve when a pivot is < 2^-6 of the largest one) -- set ONLY by a
                                 host that has checked that every non-zero Ybus entry lies inside case14's branch pattern
                                 (rpo_amd/ops.py EvopfKernels; a skipped non-zero column gives a wrong answer, not a small pivot).
                                 Anything else -- in particular the 0 a table built by other code carries there -- = always
                                 partial pivoting: the safe choice is the default (ABI 5; the meaning was inverted in ABI 4). */
#define RPO_EVOPF_STATIC_OK 1.0f
#define RPO_EVOPF_C_PS 480
#define RPO_EVOPF_C_SHARE 504
#define RPO_EVOPF_C_QSIGN 518
#define RPO_EVOPF_C_PRICE 532
#define RPO_EVOPF_CONSTS_LEN 560
#define RPO_EVOPF_SCEN_DAY 720 /* floats per day of a scenario table: price[48] | 24 x (pd[14] qd[14]); 2880 bytes */

#define RPO_CTRL_LEN 288
#define RPO_CTRL_T 0        /* vector steps completed */
#define RPO_CTRL_ARRIVE 1   /* top-level arrival counter of the running *_step launch (always 0 between launches) */
#define RPO_CTRL_UPDATES 2  /* updates done within the current vector step (host-maintained, 0 unless several updates
                               per step are requested): 4th Philox counter word of the sampling / update-noise draws */
#define RPO_CTRL_NONFINITE 3 /* failure detection (the reference asserts on a NaN action: cartpole.py:170-174,
                               pendulum.py:85-89): 0, or 1 + the vector step at which a lane FIRST stepped with a NaN action or
                               reached a non-finite next state / reward.  Sticky: set once by the *_step / *_rollout / riding
                               kernels (one compare-and-swap per offending lane, nothing on the clean path), cleared only by the
                               host; the transitions of that step ARE in the ring -- the host must stop, not train on. */
#define RPO_CTRL_SUB0 16    /* 16 sub-counters, one per 128-byte line: ctrl[RPO_CTRL_SUB0 + RPO_CTRL_SUB_STRIDE * j] */
#define RPO_CTRL_SUB_STRIDE 16

#define RPO_GRADMAX_SLOTS 16   /* `gradmax` buffers (inf-norm of a gradient slice, clip_grad_norm_) are float[RPO_GRADMAX_LEN]: */
#define RPO_GRADMAX_LEN 512    /* 16 slots 128 bytes apart (slot j at [32 j]), a producing workgroup maxes into slot
                                  (block index) % 16 and the norm is the maximum over the slots -- several hundred atomics on
                                  ONE cache line are served one after the other (2.9 us behind a 448-workgroup backward);
                                  rpo_absmax_slots spreads likewise (rpo_absmax writes word 0); rpo_adam_step* read all slots and zero them (reset_gradmax) */
#define RPO_ADAM_STATE_LEN 544 /* int32 words of an optimiser state buffer (`step_dev` of rpo_adam_step*) */
#define RPO_STATS_SUB 16    /* sub-rows per statistics row: workgroup b adds into sub-row b % 16; the reader sums them */
#define RPO_STATS_LEN 16
#define RPO_STAT_REWARD_SUM 0    /* sum over envs of this step's reward                   rpo_ddpg.py:132 */
#define RPO_STAT_EPISODES 1      /* episodes that ended at this step                       rpo_ddpg.py:134 */
#define RPO_STAT_RETURN_SUM 2    /* sum of their returns                                   rpo_ddpg.py:134 */
#define RPO_STAT_LENGTH_SUM 3    /* sum of their lengths                                                   */
#define RPO_STAT_MAX_INEQ_SUM 4  /* sum over envs of max_i ineq_viol_i                     rpo_ddpg.py:121 */
#define RPO_STAT_MAX_EQ_SUM 5    /* sum over envs of max_i |eq_viol_i|                     rpo_ddpg.py:120 */
#define RPO_STAT_VIOL_COUNT 6    /* envs with max(max_ineq, max_eq) > viol_thresh          cartpole.py:326 */
#define RPO_STAT_MAX_INEQ_MAX 7  /* max over envs                                                          */
#define RPO_STAT_MAX_EQ_MAX 8
#define RPO_STAT_PROJ_ITERS 9    /* sum over envs of GRG iterations taken by the rollout projection       */
#define RPO_STAT_TERMINATED 10   /* episodes ended by the env's own termination test (not the TimeLimit)   */

/* Per-episode accumulators of a policy evaluation (rpo_<env>_evaluate, rpo_eval_accumulate): float[n, RPO_EVAL_LEN], one
 * row per episode, written by the launch at step 0 (nothing needs clearing).  Slots 0..6 are floats; slot 7 holds the int32
 * word RPO_EVAL_ALIVE | RPO_EVAL_NONFINITE | length << RPO_EVAL_LEN_SHIFT. */
#define RPO_EVAL_LEN 8
#define RPO_EVAL_RET 0           /* sum of the rewards of the episode's steps */
#define RPO_EVAL_MEAN_INEQ 1     /* running mean m + (x - m) / (i + 1) of the step's max inequality violation */
#define RPO_EVAL_MEAN_EQ 2       /* the same of the step's max |equality residual| */
#define RPO_EVAL_MAX_INEQ 3      /* maxima over the episode's steps (NaN-propagating like torch.maximum) */
#define RPO_EVAL_MAX_EQ 4
#define RPO_EVAL_VIOL_STEPS 5    /* steps whose max inequality violation exceeds viol_thresh */
#define RPO_EVAL_PROJ_ITERS 6    /* GRG iterations summed over the episode */
#define RPO_EVAL_WORD 7
#define RPO_EVAL_ALIVE 1         /* the episode has not ended: the next step updates the row */
#define RPO_EVAL_NONFINITE 2     /* a live step produced a non-finite reward or violation */
#define RPO_EVAL_LEN_SHIFT 2     /* steps taken (the step that ended the episode included) */
#define RPO_EVAL_LANE_STEPS 4194304  /* lane-steps per evaluate launch the host aims at: steps = clamp(this / n, 1, horizon) */
/* The same for rpo_evopf_evaluate, where a lane-step is a power-flow solve and not a row of a tile.  The kernel's geometry (one
 * wave per lane, one wave per SIMD) runs 4 waves x 256 CUs = 1024 lanes at once, so L lane-steps take about L / 1024 lane-step
 * times.  A lane-step is Newton + the GRG iterations of the evaluation budget: ~48 us at 10 iterations, ~3.4 us
 * per further iteration, so ~190 us at the scripts' eval_steps = 50 -- measured 195 us with the actor.
 * 12 rounds of the chip = 12 * 1024 = 12288 lane-steps ~ 2.3 ms per launch at that budget (0.6 ms at 10 iterations): a
 * 24-step day in one launch up to 512 lanes, two launches at 1024, one step per launch from 12288 lanes on. */
#define RPO_EVOPF_EVAL_LANE_STEPS 12288

/* Per-step record of a policy evaluation (rpo_<env>_evaluate_record, rpo_eval_record): float[T, R, W], step-major -- row
 * (s, i) is env step s of episode i < R, so the lanes of a workgroup write neighbouring rows.  With O / P / A the widths of
 * the observation, the proposal (the partial action handed to the projection) and the action, a row is
 *   head [HEAD = (O + P + A + 1) rounded up to RPO_TRACE_ALIGN]: obs[O] | proposal[P] | action[A] | GRG iterations | zeros
 *   tail [RPO_TRACE_TAIL], at HEAD: the RPO_TRACE_* slots below
 * and W = HEAD + RPO_TRACE_TAIL (CartSafe-v0 and SpringPendulum-v0: 16).  The head is known before the env step and the tail
 * after it; both are whole 16-byte stores.  Only live lanes write (a lane is live at step 0, and afterwards while
 * RPO_EVAL_ALIVE is set in its accumulator word), so the caller hands in a zeroed buffer and the rows of the steps after
 * an episode's end stay zero; the kernels never clear it. */
#define RPO_TRACE_ALIGN 4        /* floats: W and HEAD are multiples of it, the buffer is 16-byte aligned */
#define RPO_TRACE_TAIL 4
#define RPO_TRACE_REWARD 0       /* tail slots: the step's reward */
#define RPO_TRACE_DONE 1         /* its done flag (termination or TimeLimit) */
#define RPO_TRACE_INEQ 2         /* max inequality violation, as rpo_eval_lane_update received it */
#define RPO_TRACE_EQ 3           /* max |equality residual|, likewise */
#define RPO_TRACE_MAX_BYTES 1073741824  /* the host refuses a larger trace buffer */

/* Per-constraint report of a policy evaluation (rpo_<env>_evaluate_constraints, rpo_eval_constraints): float[n, W], one row
 * per episode, W = (2 * ineq_num + eq_num) rounded up to RPO_CON_ALIGN:
 *   ineq_max[ineq_num] | ineq_steps[ineq_num] | eq_max[eq_num] | zeros
 * ineq_max[j]: maximum over the episode's live steps of ineq_viol[j] of the step's transition row (clamped at 0 there),
 * NaN-propagating and started at 0 like RPO_EVAL_MAX_INEQ; ineq_steps[j]: the live steps with ineq_viol[j] > viol_thresh (a
 * count kept as a float: exact below 2^24, the bound on the step index); eq_max[j]: the maximum of |eq_viol[j]|.  A step is
 * live for the report exactly when it is for the accumulator row (step 0, and afterwards while RPO_EVAL_ALIVE is set BEFORE
 * the step's accumulator update).  Step 0 writes the whole row, padding included: nothing needs clearing.  CartSafe-v0: W = 16
 * (6 + 6 + 1); SpringPendulum-v0: W = 4; EVOPF-v0: W = 144 (58 + 58 + 28). */
#define RPO_CON_ALIGN 4          /* floats: W is a multiple of it, the buffer is 16-byte aligned */

/* One row of an evaluation curve (rpo_eval_summarize): double[RPO_CURVE_LEN], the accumulator rows of one evaluation
 * reduced over its episodes.  Means and population standard deviations (numpy's x.mean(), x.std()) of the float32
 * accumulators widened to float64, in eval()'s order. */
#define RPO_CURVE_LEN 16
#define RPO_CURVE_STEP 0         /* ctrl[RPO_CTRL_T] of the training env when the row was written */
#define RPO_CURVE_EPISODES 1
#define RPO_CURVE_STATS 2        /* (mean, std) of RPO_EVAL_RET, _MEAN_INEQ, _MEAN_EQ, _MAX_INEQ, _MAX_EQ: slots 2 .. 11 */
#define RPO_CURVE_LENGTH 12      /* sum of the episode lengths */
#define RPO_CURVE_VIOL_STEPS 13  /* sum of RPO_EVAL_VIOL_STEPS */
#define RPO_CURVE_NONFINITE 14   /* episodes with RPO_EVAL_NONFINITE set */
#define RPO_CURVE_WS 4096        /* doubles of workspace rpo_eval_summarize needs (per-workgroup partials in fixed slots) */
#define RPO_CURVE_MAX_EPISODES 1048576

/* noise_mode of the *_act_project entry points (agent/ddpg_pa.py:101-112, rpo_ddpg.py:98-106) */
#define RPO_NOISE_NONE 0      /* deterministic: ap used as is, not clipped          (take_action(deterministic=True)) */
#define RPO_NOISE_EXPLICIT 1  /* ap += eps * noise[i], then clip to the box         (tests: noise injected)           */
#define RPO_NOISE_PHILOX 2    /* ap += eps * N(0,1) from Philox(seed; env, t), clip (rollout)                         */
#define RPO_NOISE_UNIFORM 3   /* ap  = U(box) from Philox, ignores ap_raw           (warm-up, BoxConstraint.sample)   */
#define RPO_NOISE_CLIP_ONLY 4 /* ap clipped to the box, no noise                    (SAC: noise lives in rsample)     */

/* Philox stream tags (counter word 2) */
#define RPO_STREAM_RESET 1
#define RPO_STREAM_ACT 2
#define RPO_STREAM_SAMPLE 3
#define RPO_STREAM_POLICY 4
#define RPO_STREAM_EVOPF_DEMAND 5 /* episode load profile: Dirichlet + power factors (data/demand.py:53-62) */
#define RPO_STREAM_EVOPF_PRICE 6  /* episode price profile: magnitude + hourly noise   (data/price.py:41-43)  */
#define RPO_STREAM_EVAL_OBS 7     /* evaluate(obs_noise=): counter (episode, step, this + 0x100 * column, 0), words 0 and 1 */
#define RPO_STREAM_EVOPF_DAY 8    /* scenario bank, deal "uniform": counter (env, episode, this, 0), word 0 -> the day of the episode */

int rpo_abi_version(void);

/* Kernel-variant switches: process-wide integers the launch code reads on every call (the library reads NO environment
 * variable).  They select between kernels that compute the same values (bit-equal, or to summation round-off where a test
 * says so) and exist for A/B tests and measurements; the defaults are what is shipped and measured.
 * rpo_tuning(key, value): sets `key` to `value` and returns the previous value; value < 0 only queries; RPO_ERR_ARG for an
 * unknown key.  Not thread-safe against concurrent launches (one host thread per device, as everywhere in this ABI). */
#define RPO_TUNE_FWD_STREAM 0       /* 1: large-n forward (n >= 12288, 128 -> 256 scalar heads) through the weights-in-LDS
                                       streaming kernel (mlp_stream.h); 0: the 64-row tile kernel of rounds 3-4 */
#define RPO_TUNE_FWD_STREAM_WAVES 1 /* waves per workgroup of that kernel: 16 (default, <= 128 registers: 528 us at 2^20 rows) or 12
                                       (<= 168 registers: 576 us) */
#define RPO_TUNE_BWD_ONEPASS 2      /* 1: large-batch backward in one pass over the activations; 0: rows pass + split-K weights pass */
#define RPO_TUNE_GEMM_KSPLIT 3      /* 1: K >= 256 layer launches split k over the four waves of a workgroup; 0: one chain */
#define RPO_TUNE_MLP_GEMM 4         /* 1: 256-wide networks layer by layer (mlp_gemm.h); 0: row-tile kernels */
#define RPO_TUNE_ROLLOUT_WIDE 5     /* fused rollout: 0 16-lane tiles, 1 64-lane tiles, 3 the streaming form (weights stationary in LDS,
                                      rollout_stream.hip; 4: the same with 64-lane groups forced, its form from 2^18 lanes), 2 (default) by lane count: 16-lane tiles below 12 288 lanes,
                                      64-lane tiles below RPO_ROLLOUT_STREAM_FROM, streaming from there */
#define RPO_ROLLOUT_STREAM_FROM 65536
#define RPO_TUNE_BWD_STREAM 6       /* 1: large-batch backward as the two streaming launches of mlp_bwd_stream.h (rows kernel with W0
                                       in LDS + weights kernel); 0: the one-pass / two-pass kernels of round 3 */
#define RPO_TUNE_L1_MFMA 7         /* 1: first layer of the 128-wide row-tile forward as three matrix-core steps (S <= 6, A <= 4);
                                       0: the vector form -- the same fmaf chain, the same bits (rpo_mlp_forward / _multi only) */
#define RPO_TUNE_EVOPF_PLACE 8    /* EXPERIMENT (round 6; default 0 = off): 1: rpo_evopf_act_project places a batch
                                      projection (<= 512 rows) on XCDs 0-1 and a rollout projection on XCDs 2-7 (block b runs on XCD b % 8:
                                      the grid is padded and the other XCDs' workgroups leave at once), so that the two launches that
                                      overlap in the training windows never share a SIMD.  Measured: DESIGN.md 4b */
#define RPO_TUNE_FWD_BF16X3 9      /* EXPERIMENT (default 0 = off): 1: the streaming forward (where RPO_TUNE_FWD_STREAM
                                      applies, nowhere else) runs its hidden layer as a 3 x bf16 split of both operands on
                                      v_mfma_f32_16x16x32_bf16 (mlp_stream_bf16x3.h): f32-accurate, NOT bit-equal to the exact form */
#define RPO_TUNE_COUNT 10          /* the keys above: [0, RPO_TUNE_COUNT).  The value is pinned (callers of ABI 6 probe rpo_tuning(RPO_TUNE_COUNT, ..)
                                      for RPO_ERR_ARG), so index 10 stays no key and later keys follow behind it: */
#define RPO_TUNE_WGRAD_STAGED 11   /* 1: the hidden-vector blocks (db0, dW1 [, dW1b], db1) of rpo_split_critic_bwd_b /
                                      rpo_split_policy_e stage their operands in LDS, requested by all four waves in one round trip,
                                      and pol_e's Lagrangian fold requests its partials up front; 0: one wave fetches them with scalar
                                      loads -- the same chains, the same bits (rpo_split_critic_bwd_b_ride, bound by its lane blocks,
                                      always has the one-wave form) */
int rpo_tuning(int key, int value);

/* ---------------------------------------------------------------------------------------------------------------
 * Philox4x32-10 (Salmon et al., SC'11), the build's counter-based RNG: key = seed, counter = (id, index, stream, sub);
 * sub = 0 except for the replay-sampling and update-noise draws, where it is ctrl[RPO_CTRL_UPDATES].
 * Fills out[n,4] (uint32) with the raw words for id = id_base + i.  Test hook for bit-exact comparison with
 * oracle/philox.py.  The reference uses global numpy/torch generators instead (scripts/cart_exp.py:9-10), whose
 * streams cannot be reproduced on a GPU; parity tests inject the draws explicitly (SURVEY.md §7 hard part iv).
 * ------------------------------------------------------------------------------------------------------------- */
int rpo_philox_fill(int n, unsigned* out, unsigned long long seed, unsigned id_base, unsigned index,
                    unsigned stream_tag, void* stream);

/* out[i] = N(0,1) (Box-Muller, float32) from Philox(seed; id_base + i, t + salt, stream_tag), t = ctrl[RPO_CTRL_T]
 * (ctrl may be NULL: t = 0).  Replaces the global-generator draws of the update step -- torch.randn_like in
 * PDDDPG_PA.take_action (agent/ddpg_pa.py:109) and Normal.rsample in GaussianSharedPolicy (model/policy.py:59) --
 * with a stream that is reproducible, capturable in a hipGraph and independent of the rank layout. */
int rpo_philox_normal(int n, float* out, unsigned long long seed, unsigned id_base, unsigned salt,
                      unsigned stream_tag, const long long* ctrl, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * CartSafe-v0
 * ------------------------------------------------------------------------------------------------------------- */

/* CartSafeEnv.reset() for every lane (cartpole.py:231-239): state = U(-0.05, 0.05)^6 from
 * Philox(seed; env_id_base + lane, ep_count[lane], RPO_STREAM_RESET); zeroes ep_len / ep_ret. ep_count is kept. */
int rpo_cartsafe_reset(int n_envs, float* state, int* ep_len, float* ep_ret, const unsigned* ep_count,
                       unsigned long long seed, unsigned env_id_base, void* stream);

/* One vectorised env step + TimeLimit + violation bookkeeping + replay scatter + auto-reset, fused.
 * Replaces, per lane: CartSafeEnv.step (cartpole.py:166-229) incl. ineq_dist_np/eq_resid_np of the PRE-step state
 * and UN-clipped action (:229, :410-422), gym TimeLimit(200) (classic_control/__init__.py:9),
 * ReplayBuffer.add (rpo/utils/buffer.py:22-29), the per-step statistics of RPODDPG.run (rpo_ddpg.py:120-145) and
 * the env.reset() that follows a done (:142).
 *   state      [n,6]  in: pre-step state; out: post-step state, or a fresh reset state where done (auto_reset != 0)
 *   action     [n,2]  un-clipped action (clipped to +-10 for the dynamics only)
 *   ep_len/ep_ret/ep_count [n] per-lane episode bookkeeping (updated)
 *   rows       replay ring (may be NULL: no scatter); ring row = (t % cap_steps) * n_envs + lane, t = ctrl[RPO_CTRL_T]
 *   stats      [stats_cap, RPO_STATS_SUB, RPO_STATS_LEN] (may be NULL)
 *   ctrl       int64[RPO_CTRL_LEN]; ctrl[RPO_CTRL_T] is incremented when the launch finishes
 * Pinned by tests/test_envs_f64_gpu.py (float64 restatement: tests/envs_f64.py):
 *   done       is the reference's float64 test of the STORED float32 next state: x > 2.4, theta > 12 deg (cartpole.py:208-213).
 *              2.4f and 0.20943952f lie above those thresholds; the kernel compares with the largest floats not above them, so a
 *              next x of exactly 2.4f (or theta of 0.20943952f) terminates, as it does in the reference.
 *   np.sign    (cartpole.py:184) is taken of the FLOAT32 product n_c * x_dot: x_dot = +-0 gives sign 0 (both friction terms
 *              vanish), and so does a product that underflows to 0 -- |n_c x_dot| < 2^-150, e.g. the smallest denormal x_dot
 *              under |n_c| < 1/2 -- where the float64 product keeps its sign.  Denormals are not flushed otherwise.
 *   non-finite a NaN action or a non-finite next state sets ctrl[RPO_CTRL_NONFINITE] = t + 1 once (sticky; nothing is written
 *              with ctrl = NULL); the row's outputs are non-finite where float64 gives that, every other row keeps its bits.
 *   alignment  state / rows that are 8- but not 16-byte aligned take a per-lane path with the same bits; the 8 padding floats of
 *              a ring row are written as zeros by whole-tile launches and left untouched otherwise.
 */
int rpo_cartsafe_step(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count,
                      float* rows, long long cap_steps, float* stats, int stats_cap, long long* ctrl,
                      const float* consts_host, int partial, int max_episode_steps, int auto_reset,
                      float viol_thresh, unsigned long long seed, unsigned env_id_base, void* stream);

/* Exploration noise + box clip + equation solver + GRG projection, fused; one lane per sample, per-lane stop test.
 * Replaces PDDDPG_PA.take_action's noise/clip tail (agent/ddpg_pa.py:108-110) or BoxConstraint.sample (warm-up,
 * model/utils.py:53-62), CartSafeEnv.complete_partial (cartpole.py:369-373) and RPODDPG.grad_steps
 * (rpo_ddpg.py:266-305, corr_mode 0) with CartSafeEnv.eq_resid / ineq_dist / ineq_partial_grad (cartpole.py:375-408).
 *   ap_raw   [n]     actor output (basic action) -- ignored for RPO_NOISE_UNIFORM
 *   noise    [n]     only for RPO_NOISE_EXPLICIT
 *   action   [n,2]   out: completed + projected action
 *   iters    [n]     out (may be NULL): GRG iterations taken by the lane
 *   eps_t = max(eps_end, eps_start - eps_decay * t) (PDDDPG_PA.eps_decay, ddpg_pa.py:118-119), t = ctrl[RPO_CTRL_T]
 *   (ctrl may be NULL: t = 0).  stats may be NULL.
 * Pinned by tests/test_envs_f64_gpu.py: the other component is completed from the NOISED and clipped basic action; the masks
 * are strict (a_p G_r[i] - d_r[i] > 0: a basic action ON the box, 10 * 1 - 10 = 0, does not select its row); the first iteration
 * is unconditional and the loop then stops as soon as neither |eq_resid| nor max ineq_resid exceeds corr_eps.  A NaN basic action
 * passes through the clip and the loop as NaN and stops after ONE iteration (iters = 1 for max_steps >= 1): NaN compares false
 * with corr_eps, in torch.max(...) > corr_eps of the reference's loop as well.
 */
int rpo_cartsafe_act_project(int n, const float* ap_raw, const float* noise, float* action, int* iters,
                             int noise_mode, float eps_start, float eps_end, float eps_decay, float box_lo,
                             float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                             const float* consts_host, int partial, unsigned long long seed, unsigned env_id_base,
                             const long long* ctrl, float* stats, int stats_cap, void* stream);

/* Backward of complete_partial for the actor loss (rpo_ddpg.py:310; autograd through cartpole.py:369-373):
 * grad_ap[i] = grad_action[i,p] - grad_action[i,o] * C_p * C_o_inv. */
int rpo_cartsafe_complete_bwd(int n, const float* grad_action, float* grad_ap, const float* consts_host,
                              int partial, void* stream);

/* Constraint residuals of a batch of full actions: eq_resid [n,1] (cartpole.py:375-376), ineq_resid [n,6] (:378-379).
 * Either output may be NULL.  ineq_dist = max(ineq_resid, 0). */
int rpo_cartsafe_resid(int n, const float* action, float* eq_resid, float* ineq_resid, const float* consts_host,
                       int partial, void* stream);

/* ineq_partial_grad (cartpole.py:396-408) -> step [n,2]. */
int rpo_cartsafe_ineq_partial_grad(int n, const float* action, float* step, const float* consts_host, int partial,
                                   void* stream);

/* Lagrangian term of the actor loss, forward + backward fused (rpo_ddpg.py:312,319,322; Dual.forward dual.py:63-65):
 *   loss_out[0] += scale * sum_b sum_i nu_i * max(0, g_i(a_b));   grad_action[b,:] = scale * sum_i nu_i 1[g_i>0] G_i;
 *   grad_nu[i] += scale * sum_b max(0, g_i(a_b)).   loss_out / grad_nu must be zeroed by the caller. */
int rpo_cartsafe_lagrangian(int n, const float* action, const float* nu, float scale, float* loss_out,
                            float* grad_action, float* grad_nu, const float* consts_host, int partial, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * SpringPendulum-v0 (same roles; the equality is state dependent, pendulum.py:264-288)
 * ------------------------------------------------------------------------------------------------------------- */
int rpo_pendulum_reset(int n_envs, float* internal, float* obs, int* ep_len, float* ep_ret, const unsigned* ep_count,
                       unsigned long long seed, unsigned env_id_base, void* stream);

/* pendulum.py:80-128 + TimeLimit + scatter + auto-reset.  internal [n,4] in/out; obs [n,5] out (may be NULL): the
 * next observation, or the reset observation where done.  The pre-step observation stored in the transition row is
 * recomputed from `internal` (it is bit-identical to what a previous launch wrote to `obs`).
 * Pinned by tests/test_envs_f64_gpu.py (tests/envs_f64.py): done is the reference's float64 test of the STORED next state
 * (l <= 0.5, l >= 1.5, |theta| >= pi / 12: pi/12f lies above pi / 12 and the tests are >= / <=, so the float32 comparison IS that
 * test; equality terminates); theta is stepped with the UN-clipped next theta_dot and the speed clip at +-8 follows; the reward's
 * |angle_normalize(theta)| is |theta| exactly for -pi < theta < pi and ((theta + pi) mod 2 pi) - pi outside; the violations are
 * those of the un-clipped action; the Lagrangian's mask g > 0 is strict (g = 0 gives gradient 0 exactly); non-finite rows as in
 * rpo_cartsafe_step; a NaN basic action in rpo_pendulum_act_project as in rpo_cartsafe_act_project. */
int rpo_pendulum_step(int n_envs, float* internal, float* obs, const float* action, int* ep_len, float* ep_ret,
                      unsigned* ep_count, float* rows, long long cap_steps, float* stats, int stats_cap,
                      long long* ctrl, int max_episode_steps, int auto_reset, float viol_thresh,
                      unsigned long long seed, unsigned env_id_base, void* stream);

/* noise/clip + complete_partial (pendulum.py:256-262) + grad_steps with the ROW-WISE ineq_partial_grad
 * (pendulum.py:331-343 as evaluated for B = 1; the reference's batched call couples samples).
 * obs rows are read with a row stride of obs_stride floats (>= 5): they may be columns of a gathered batch. */
int rpo_pendulum_act_project(int n, const float* obs, int obs_stride, const float* ap_raw, const float* noise,
                             float* action, int* iters, int noise_mode, float eps_start, float eps_end,
                             float eps_decay, float box_lo, float box_hi, int max_steps, float corr_lr,
                             float corr_eps, float corr_momentum, unsigned long long seed, unsigned env_id_base,
                             const long long* ctrl, float* stats, int stats_cap, void* stream);

#define RPO_PROJ_WS_WORDS 5408
#define RPO_PROJ_WS_GAVE_UP 529
/* complete_partial + the reference's LITERAL batched grad_steps on a training batch (n <= 1024): batch-global stop
 * test (rpo_ddpg.py:271-272) and the sample-coupled ineq_partial_grad of pendulum.py:337-339, grad_i = sum_j
 * 1[a_x,i * dgp_j - bgp_i > 0] * dgp_j.  Used for the TD-target projection of critic_loss
 * (rpo_ddpg.py:330) so that the update step matches the reference; iters_out (int32[1], may be NULL) = iterations. */
int rpo_pendulum_project_batchref(int n, const float* obs, int obs_stride, const float* ap, float* action,
                                  int* iters_out, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                  void* stream);
/* The same on one workgroup per 16 rows (n <= 256, max_steps <= 30): the batch's dgp values are all-gathered
 * once per GRG iteration through tagged 8-byte granules in `ws` (RPO_PROJ_WS_WORDS 64-bit words, 128-byte aligned, zero before
 * the first launch; see rpo_split_update.proj_ws for store_mode and the gave-up word).  Same bits as the call above. */
int rpo_pendulum_project_batchref_ws(int n, const float* obs, int obs_stride, const float* ap, float* action, int* iters_out,
                                     int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                     unsigned long long* ws, int store_mode, void* stream);

/* grad_ap[i] = grad_action[i,0] - grad_action[i,1] * sin/cos (autograd through pendulum.py:256-262). */
int rpo_pendulum_complete_bwd(int n, const float* obs, int obs_stride, const float* grad_action, float* grad_ap,
                              void* stream);

/* eq_resid [n] (pendulum.py:298-300), ineq_resid [n] (:302-303); either output may be NULL. */
int rpo_pendulum_resid(int n, const float* obs, int obs_stride, const float* action, float* eq_resid,
                       float* ineq_resid, void* stream);

int rpo_pendulum_ineq_partial_grad(int n, const float* obs, int obs_stride, const float* action, float* step,
                                   void* stream);

/* g(a) = |a|^2 - 32: loss += scale * nu * sum_b max(0,g); grad_action = scale * nu * 1[g>0] * 2a; grad_nu likewise. */
int rpo_pendulum_lagrangian(int n, const float* action, const float* nu, float scale, float* loss_out,
                            float* grad_action, float* grad_nu, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Replay ring (rpo/utils/buffer.py:3-47)
 * ------------------------------------------------------------------------------------------------------------- */

/* ReplayBuffer.sample (buffer.py:31-34): uniform with replacement over the valid rows
 * n_valid = min(t, cap_steps) * n_envs (t = ctrl[RPO_CTRL_T]); index b = mulhi64(Philox(seed; b, t + sample_salt,
 * RPO_STREAM_SAMPLE).xy, n_valid); copies the row into batch[b, :].  idx_out (int64 [B], may be NULL) receives the
 * drawn indices.  ring_floats = floats between consecutive ring rows (RPO_*_RING; >= row_floats), row_floats = floats of a
 * transition = width of the gathered batch. */
int rpo_replay_sample_gather(const float* rows, int ring_floats, int row_floats, long long cap_steps, int n_envs, int batch,
                             float* batch_out, long long* idx_out, unsigned long long seed, unsigned sample_salt,
                             const long long* ctrl, void* stream);

/* Same gather with caller-provided indices (int64 [B]) -- parity tests inject the reference's np.random.randint. */
int rpo_replay_gather(const float* rows, int ring_floats, int row_floats, int batch, const long long* idx, float* batch_out,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused TD target + Huber loss, forward + backward (RPODDPG.critic_loss rpo_ddpg.py:327-337,
 * RPOSAC.critic_loss rpo_sac.py:342-353; F.smooth_l1_loss beta = 1, mean reduction)
 *   y_b = r_b + gamma * (1 - done_b) * (min(qn1_b, qn2_b) - alpha * logp_b)        (qn2 / logp NULL: DDPG form)
 *   loss_out[0] += (1/n) sum_b huber(q1_b - y_b) [+ huber(q2_b - y_b)];  grad_q*[b] = clamp(q*_b - y_b, -1, 1) / n
 *   reward / done are read with an element stride (they are columns of the gathered batch).
 * ------------------------------------------------------------------------------------------------------------- */
int rpo_td_huber(int n, const float* q1, const float* q2, const float* qn1, const float* qn2, const float* logp,
                 float alpha, const float* reward, int reward_stride, const float* done, int done_stride, float gamma,
                 float* loss_out, float* grad_q1, float* grad_q2, float* target_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Optimiser plumbing of RPODDPG.train (rpo_ddpg.py:178-205) on flat float32 parameter buffers
 * ------------------------------------------------------------------------------------------------------------- */

/* d(-min(q1, q2))/dq scaled (the actor loss of RPOSAC, rpo_sac.py:335): the smaller one takes the gradient, ties are split like
 * torch.min's backward: w = [q1 < q2] + 0.5 [q1 == q2]; dq1 = w * scale, dq2 = (1 - w) * scale (exact: w is 0, 0.5 or 1;
 * +0.0 == -0.0 and inf == inf are ties).  A NaN on either side, or both, makes both comparisons false: dq1 = 0, dq2 = scale.
 * That deviates from torch: torch.minimum's backward hands BOTH inputs the full gradient there, dq1 = dq2 = scale. */
int rpo_min_q_bwd(int n, const float* q1, const float* q2, float scale, float* dq1, float* dq2, void* stream);

/* max_out[0] = max(max_out[0], max_i |x_i|) -- the "inf" norm of clip_grad_norm_ (rpo_ddpg.py:180,193).
 * max_out must hold a non-negative float (0 before the first call of an update).  x must be 16-byte aligned.
 * NaN: fmaxf drops a NaN operand, so the norm is the maximum over the elements that are NOT NaN (torch's norm would be NaN and
 * poison every element through the clip coefficient).  rpo_adam_step* then turns exactly the NaN element's exp_avg, exp_avg_sq
 * and parameter into NaN and steps every other element with the norm of the finite ones. */
int rpo_absmax(long long n, const float* x, float* max_out, void* stream);
/* The same into a gradmax buffer [RPO_GRADMAX_LEN]: workgroup b maxes into slot b % 16 (the norm is the maximum over the
 * slots, as rpo_adam_step* read it) -- a wide launch does not queue its atomics on one word. */
int rpo_absmax_slots(long long n, const float* x, float* gradmax, void* stream);

/* clip_grad_norm_(inf) + torch.optim.Adam step (+ optional DualAdam clamp, model/dual.py:37-45) (+ optional Polyak
 * target update, agent/ddpg_pa.py:77-86), one pass over the flat buffer:
 *   coef = min(1, clip_thres / (max over the slots of gradmax [RPO_GRADMAX_LEN] + 1e-6)) when clip_thres > 0 (gradmax from
 *   rpo_absmax or left by a backward launch); g = coef * grad
 *   (written back, as clip_grad_norm_ does); maximize: g = -g; weight decay; Adam with bias correction at step
 *   step_dev[0] + 1 (the counter is advanced by the launch); clamp_min0: p = max(p, 0); target != NULL:
 *   target = (1 - tau) * target + tau * p.   gradmax is reset to 0 by the launch when reset_gradmax != 0.
 *   zero_grad != 0: instead of the clipped value, 0 is written back -- the gradient is consumed, so that the next
 *   backward pass (which accumulates) needs no separate fill launch (optimizer.zero_grad() folded into the step).
 *   step_dev points at int32[RPO_ADAM_STATE_LEN] (128-byte aligned): {step, the step the cached corrections belong to,
 *   8-byte arrival word (0 between launches),
 *   two doubles: the bias corrections 1 - beta1^(step+1), sqrt(1 - beta2^(step+1)) cached by the previous launch (0.0 = not
 *   cached: they are then computed by every thread; zero-initialise the buffer, and zero the cache when betas change)},
 *   then from word 32 on 16 sub-counters 128 bytes apart (0 between launches): the launch finds its last workgroup
 *   through a two-level arrival tree -- 135 returning atomics on ONE word are served one after the other (3.3 us of a
 *   5.8 us launch, 4.7 us with 270 workgroups); 9 per sub-counter + 16 on the top word are not.
 *   prepared = 1: the caller's previous launch did the bookkeeping (rpo_split_update.prep_step: step_dev[0] already holds
 *   THIS step, the cache its corrections) -- the launch is then purely elementwise: it neither counts its workgroups in
 *   nor touches step_dev, gradmax (reset by the next rpo_split_critic_fwd_a, gradmax_reset) or `clock`.
 *   Words of step_dev a launch may write: 0-7 (step, cached step, arrival word, the two doubles) and 32 k + 32, 32 k + 33 for
 *   k < 16 (the sub-counters); no other word of the 544 is read or written.  Of gradmax only the 16 words [32 j] are.
 *   Scalars: lr, betas, eps, weight_decay, tau arrive as float.  1 - beta and 1 - tau are formed in float32 FROM the float, and
 *   the bias corrections in double from the float32 betas.  torch.optim.Adam hands its float32 ops float32(1 - beta) and takes
 *   the corrections from the double betas: for beta2 = 0.999 the two 1 - beta2 differ by 1.3e-5 relative, which one step does not
 *   show (0.11 eps32 of g^2 in exp_avg_sq) and thousands of steps build up to 1.3e-5 of exp_avg_sq (108 eps32; 6e-6 of the
 *   denominator); sqrt(1 - beta2^t) differs by up to 6.4e-6 (t = 1; 3.7e-6 at t = 1000, nothing once beta2^t is gone).  Harmless
 *   for learning; the cure is double scalars through this ABI (tests/optim_f64.py).
 *   clamp_min0 is fmaxf(p, 0): a NaN parameter comes out as 0 (torch's clamp_ keeps NaN) while its exp_avg / exp_avg_sq stay NaN. */
int rpo_adam_step(long long n, float* param, float* grad, float* exp_avg, float* exp_avg_sq, int* step_dev,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int maximize, float clip_thres,
                  float* gradmax, int reset_gradmax, int zero_grad, int clamp_min0, float* target, float tau,
                  long long* clock, int prepared, void* stream);
/*   clock (may be NULL): a device counter advanced by one when the launch has finished.  The trainers use it as the
 *   UPDATE clock: the update kernels read their step index from it instead of ctrl[RPO_CTRL_T], so that the next
 *   rollout -- which advances ctrl[RPO_CTRL_T] -- may run concurrently with the update (another stream of the same
 *   hipGraph) without the update seeing the counter move. */

/* Up to four independent optimiser slices in ONE launch (gridDim.y = slice): the tail of a policy step is
 * actor Adam + multiplier DualAdam + the Polyak update of the critic target (rpo_ddpg.py:197-205), three launches of a
 * few microseconds each otherwise.  Every field as in rpo_adam_step; additionally
 *   target2 / n2: a second Polyak target for the first n2 elements of the slice (with a shared state embedding the
 *                 actor's step also moves the critic's copy of it: critic_target[shared] follows in the same pass);
 *   polyak_only:  no optimiser step for this slice, only target = (1 - tau) target + tau param (grad etc. unused).
 * The slices must not overlap. */
typedef struct {
    long long n;
    float *param, *grad, *exp_avg, *exp_avg_sq;
    int* step_dev;
    float lr, beta1, beta2, eps, weight_decay;
    int maximize;
    float clip_thres;
    float* gradmax;
    int reset_gradmax, zero_grad, clamp_min0;
    float* target;
    float tau;
    float* target2;
    long long n2;
    int polyak_only;
    int prepared;                /* as in rpo_adam_step (per slice; with every stepped slice prepared the launch counts no
                                    workgroups in and `clock` is ignored) */
} rpo_adam_seg;
int rpo_adam_step_multi(int count, const rpo_adam_seg* segs, long long* clock, void* stream);

/* soft_update alone (agent/ddpg_pa.py:77-86, sac_pa.py:87-91): target = (1 - tau) * target + tau * param. */
int rpo_polyak(long long n, const float* param, float* target, float tau, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Actor / critic MLPs, exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32 == an fmaf chain).
 * One descriptor covers every network of the reference's agents with hidden_layer = 1 (model/embedding.py:21-29,
 * model/policy.py:24-33,48-57, model/value.py:51-59,125-140):
 *     x0 = s Ws^T + bs (+ a Wa^T + ba; `cat`: [s-part | a-part] concatenated, model/value.py:22-31)
 *     h1 = relu(x0) W0^T + b0 ;  out_k = relu(h1) W1_k^T + b1_k   (k < n_out; second head = SAC's log-std head)
 * Weights are device pointers in torch's nn.Linear layout [out][in]; W0 must be 16-byte aligned.
 * Supported sizes: H = 256 and Ein (= E, or 2E when cat) in {128, 256, 512}; S <= 64, A <= 48 (rpo_mlp_supported).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *Ws, *bs, *Wa, *ba, *W0, *b0, *W1, *b1, *W1b, *b1b;
    int S, A, E, H, n_out, cat;
    int head_dim; /* outputs per head: 0 / 1 = scalar heads (out [n, n_out]); 2..16 = W1_k is [head_dim, H], b1_k
                   * [head_dim], out [n, n_out * head_dim] head-major, raw (out_mode must be 0): the 14 basic actions of
                   * EVOPF-v0, whose state-dependent tanh box is applied by rpo_evopf_act_project (ap_is_raw) */
} rpo_mlp;
typedef struct {
    float *Ws, *bs, *Wa, *ba, *W0, *b0, *W1, *b1, *W1b, *b1b;
    /* Large batches (n >= RPO_SPLITK_FROM rows): NULL, or a scratch buffer of splitk_floats floats.  The weights pass of the
     * backward kernels then splits the batch over up to 256 slices -- every slice accumulates its share of every parameter
     * gradient into its own copy of the network's gradient span inside this buffer (one owner per element, fixed order) and a
     * second launch adds the slices in order: the batch reductions use the width of the chip instead of ~50 workgroups
     * (36 ms -> ~2 ms at 2^20 rows), still bitwise reproducible.  Needs >= 2 x (the span of the gradient tensors, in floats).
     * Must be 16-byte aligned (it is zeroed with float4 stores): rpo_mlp_backward / _pair (whenever param_grads is set) and
     * rpo_ddpg_actor_backward / rpo_sac_actor_backward (the actor's scratch) refuse another address with RPO_ERR_ARG before
     * any launch. */
    float* splitk_scratch; long long splitk_floats;
} rpo_mlp_grad;
#define RPO_SPLITK_FROM 16384

/* TD target + Huber loss as a prologue of the critic's backward pass (rpo_ddpg.py:331-335, rpo_sac.py:346-353): with
 * td != NULL rpo_mlp_backward ignores `dout` and computes, per row i,
 *   y = reward + gamma (1 - done) (min(qn1, qn2) - alpha logp),  dq_out[i] = clamp(q[i] - y, -1, 1) / n  (its dout),
 * and loss_partial[i / 16] = that row tile's share of the mean smooth-L1 loss (n_out must be 1).  qn2 / logp may be
 * NULL (RPODDPG).  This is what lets the critic-forward pipelines run Q, Q_targ (and the twin critics) in separate
 * workgroups: the values meet at the kernel boundary instead of inside one workgroup. */
typedef struct {
    const float *q, *qn1, *qn2, *logp;
    const float* reward; int reward_stride;
    const float* done; int done_stride;
    float alpha, gamma;
    float* dq_out;
    float* loss_partial;
} rpo_td;

int rpo_mlp_supported(int E, int H, int cat);

/* Forward of n rows.  s [n, >=S] / a [n, >=A] are read with row strides (columns of a gathered batch are fine).
 * out [n, n_out]; x0_save [n, Ein] / h1_save [n, H] (pre-activations, for rpo_mlp_backward) may be NULL.
 * out_mode 1 applies BoxConstraint's tanh map to output 0: scale * tanh(o) + base (model/utils.py:40-51).
 * Non-finite values: relu(x) is x for x > 0 AND for a NaN of either sign, 0 otherwise -- a NaN pre-activation stays NaN.  A NaN
 * in row r of s / a therefore makes x0[r] (the part that read it), every entry of h1[r] and every output of row r NaN; +-inf does
 * the same wherever inf * 0 or inf - inf arises (a zero weight is enough).  Rows are independent: no other row changes a bit.
 * This holds for rpo_mlp_forward in every form (row tile, first layer on either unit, x0 / h1 saved or not, layer by layer),
 * rpo_mlp_forward_multi and rpo_mlp_forward_split + rpo_mlp_split_head, which agree on such rows as on all others; the failure
 * flag (RPO_CTRL_NONFINITE) relies on it.  The streaming forms (n >= 12288 rows here; the streaming rollout and policy_act, which
 * share that forward) keep a NaN of either sign like every other form: tests/test_nonfinite_gpu.py pins the launches that train,
 * act and evaluate.  One exception, stated: the opt-in 3 x bf16 hidden layer (RPO_TUNE_FWD_BF16X3) still takes its relu as an
 * integer maximum and keeps a NaN only when its sign bit is clear. */
int rpo_mlp_forward(const rpo_mlp* net_host, int n, const float* s, int s_stride, const float* a, int a_stride,
                    float* out, float* x0_save, float* h1_save, int out_mode, float scale, float base, void* stream);

/* rpo_mlp_forward (out_mode 0) of 1..4 same-shaped scalar-head networks, each on its own inputs, in ONE launch
 * (gridDim.y = network): Q_targ(s', a') and Q(s, a) of a critic update, and RPOSAC's twins (model/value.py:125-140), do
 * not depend on each other.  All arguments are arrays of `count` entries; x0_save[k] / h1_save[k] may be NULL. */
int rpo_mlp_forward_multi(int count, const rpo_mlp* const* nets, int n, const float* const* s, const int* s_stride,
                          const float* const* a, const int* a_stride, float* const* out, float* const* x0_save,
                          float* const* h1_save, void* stream);

/* Column-split forward (rpo_amd/csrc/nsplit_dev.h): the hidden layer of 1..4 same-shaped scalar-head networks (E = 128,
 * H = 256, "add" critics / actors, S <= 6, A <= 4: the first layer is three matrix-core steps) on 16 row tiles x 8 column groups of workgroups each.  Leaves the head
 * partials of the column groups in part_k [8, n, 2]; rpo_mlp_split_head (or the prologue of any consumer kernel) adds
 * them in the order of rpo_mlp_forward's wave loop, so the outputs are bitwise those of rpo_mlp_forward.  This is how
 * the batch-256 update kernels use the width of the chip: one network evaluation is 128 workgroups with a 16 KB weight
 * slice and a 32-instruction MFMA chain each, instead of 16 workgroups with 128 KB and 128 instructions per SIMD. */
int rpo_mlp_split_supported(const rpo_mlp* net_host);
int rpo_mlp_forward_split(int count, const rpo_mlp* const* nets, int n, const float* const* s, const int* s_stride,
                          const float* const* a, const int* a_stride, float* const* part, float* const* x0_save,
                          float* const* h1_save, void* stream);
int rpo_mlp_split_head(const rpo_mlp* net_host, int n, const float* part, float* out, int out_mode, float scale,
                       float base, void* stream);

/* ---- Column-split update of RPODDPG / RPOSAC on CartSafe-v0 / SpringPendulum-v0 (rpo_amd/csrc/nsplit.hip) -------------
 * The batch-256 constrained policy update (rpo_ddpg.py:163-205, rpo_sac.py:167-219) as a chain of SHORT launches that
 * each use the width of the chip (>= 128 workgroups), cut where a value needs every hidden column or every sample:
 *
 *   critic update   fwd_a   ReplayBuffer.sample -> {pi_targ / pi hidden slabs on s' | Q1 (, Q2) hidden slabs on (s, a)}
 *                   fwd_b   head of pi -> (rsample, log pi) -> Complete + Proj -> Q_targ (x2) hidden slabs on (s', a')
 *                           (SpringPendulum: head + the batch-coupled projection are one single-workgroup launch,
 *                           rpo_split_pend_head_project, followed by fwd_b on the projected actions)
 *                   bwd_a   TD target + Huber (from the slab partials) -> {dx0 column groups | dW0 tiles | hidden vectors}
 *                   bwd_b   first-layer gradients (batch reduction of dx0), inf-norm of everything written
 *                   then rpo_adam_step.
 *   policy step     pol_a   pi hidden slabs on s (saved)
 *                   pol_b   head -> noise / rsample + clip -> Complete -> Lagrangian row terms -> Q (x2) slabs on (s, a_pi)
 *                   pol_c   d(-Q or -min Q)/dQ -> critic dx0 column groups -> per-group partials of d/d action
 *                   pol_d   d/d action -> Complete -> head backward -> {actor dx0 column groups | dW0 tiles | vectors}
 *                   pol_e   actor first-layer gradients (+ the critics' dx0 under a shared embedding), multiplier terms
 *                   then rpo_adam_step_multi.
 * Every network is E = 128, H = 256, "add" critic / scalar-head actor (rpo_mlp_split_supported).  All values are
 * bitwise those of the row-tile pipelines (rpo_cartsafe_*_critic_forward + rpo_mlp_backward) for the critic update;
 * the policy step sums d/d action over column groups (agrees to 1e-7 relative).  One struct carries the arguments
 * of all stages; a stage reads only the fields it needs.  part_* are [8, batch, 2] float buffers. */
typedef struct {
    const rpo_mlp *actor, *actor_target, *critic1, *critic2, *critic_target1, *critic_target2;
    const rpo_mlp_grad *critic1_grad, *critic2_grad, *actor_grad;
    int env;                     /* 0 CartSafe-v0 (consts_host / partial), 1 SpringPendulum-v0 */
    int twin;                    /* 0 RPODDPG (actor_target, critic1, critic_target1), 1 RPOSAC (actor, twins) */
    int batch;
    /* ReplayBuffer.sample */
    const float* rows; long long cap_steps; int n_envs;
    float* batch_out; long long* idx_out; const long long* idx_in;
    unsigned long long sample_seed; unsigned sample_salt;
    /* policy draws: rsample of a' (critic update) / take_action noise (policy step); eps_in / noise_in replace Philox */
    const float* eps_in; unsigned long long noise_seed; unsigned noise_id_base, noise_salt;
    const long long* ctrl;
    float scale, base, box_lo, box_hi;
    int max_steps; float corr_lr, corr_eps, corr_momentum;
    const float* consts_host; int partial;
    float alpha, gamma;
    float eps_start, eps_end, eps_decay;          /* exploration schedule of take_action in the actor loss (RPODDPG) */
    /* slab partials and saved pre-activations */
    float *part_pi, *part_q1, *part_q2, *part_qn1, *part_qn2;
    float *x0_1, *h1_1, *x0_2, *h1_2, *x0_a, *h1_a;
    float *logp;                 /* [batch] log pi(a'|s') (critic update) / log pi(a|s) (policy step) */
    float *next_actions;         /* [batch, 2] SpringPendulum: projected a' */
    int *proj_iters;             /* NULL or [1] */
    /* backward */
    float *dq1, *dq2;            /* [batch] dLoss/dQ_k */
    float *loss_partial;         /* [2, ceil(batch / 16)] */
    float *dx0_1, *dx0_2, *dx0_a;
    float *gradmax;              /* NULL or [RPO_GRADMAX_LEN] */
    /* policy step */
    const float* nu; float* nu_grad;
    float *ap_det, *noise_out, *raw, *actions, *g_act, *lag_partial, *lag_out, *da_part, *dout;
    int shared_embedding;
    /* fwd_a: NULL, or the clock / statistics of a rollout launched with defer_clock = 1 right before this update:
     * fwd_a advances rollout_ctrl[RPO_CTRL_T] and clears the next statistics row on its behalf */
    long long* rollout_ctrl; float* rollout_stats; int rollout_stats_cap;
    /* bwd_b: bookkeeping for the rpo_adam_step(prepared = 1) launch of the critic that follows it.  prep_step: NULL, or that
     * optimiser's state buffer -- one thread of bwd_b advances step_dev[0] and leaves the bias corrections of the new step
     * (prep_beta1 / prep_beta2 = the optimiser's betas).  clock_out: NULL, or the update clock, advanced by one (set it
     * when the critic step is the iteration's last optimiser launch).  gradmax_reset (fwd_a): NULL, or the gradmax buffer a
     * prepared Adam launch of the PREVIOUS update consumed: fwd_a zeroes its slots before this update's backward fills them. */
    int* prep_step; float prep_beta1, prep_beta2; long long* clock_out; float* gradmax_reset;
    /* pol_e: the same bookkeeping for up to three slices of the rpo_adam_step_multi launch behind the policy step (actor,
     * multipliers, log alpha); clock_out is advanced by pol_e when set for that stage.  gradmax_reset2 (fwd_a): the actor's. */
    int* prep2_step[3]; float prep2_beta1[3], prep2_beta2[3]; float* gradmax_reset2;
    /* bwd_b / pol_e: NULL, or the update's ctrl buffer: ctrl[RPO_CTRL_UPDATES] += 1 when the stage is the last one of the
     * update that reads it (several updates per vector step: the next update draws with the next sub-index) */
    long long* updates_out;
    /* policy step: head partials of pi(s) between pol_a and pol_b, [8, batch, 2]; NULL: part_pi is used.  A buffer of its
     * own lets pol_a run INSIDE fwd_b's launch (rpo_split_critic_fwd_b_pol) while fwd_b still reads part_pi. */
    float* part_pol;
    /* rpo_split_critic_front: [(3 * ceil(batch / 16) + 1) * 32] words (one 128-byte line per arrival word), 128-byte
     * aligned, zero before the first launch (every launch leaves them zero); word [3 * ceil(batch / 16) * 32] is set to 1 if a
     * workgroup ever gave up waiting for its tile's producers (never, on a healthy device). */
    unsigned* tile_sync;
    /* rpo_split_pend_head_project: NULL (one workgroup), or RPO_PROJ_WS_WORDS 64-bit words, 128-byte aligned, zero before the
     * first launch: the batch-coupled projection then runs on one workgroup per row tile; they all-gather the batch's dgp values once
     * per GRG iteration through tagged 8-byte granules in this buffer (batch <= 256, max_steps <= 30; same bits).  Word
     * RPO_PROJ_WS_GAVE_UP is set to 1 if a workgroup ever gave up waiting for another one's granules (never, on a healthy
     * device).  proj_store_mode: 0 = agent-scope granule stores; 1 = plain stores when the workgroups find themselves on
     * one XCD (checked inside every launch; the polling loads are served by that XCD's L2), agent-scope otherwise. */
    unsigned long long* proj_ws; int proj_store_mode;
    /* tests only (0 in production): bit 0 -- in the fused front launches the policy workgroup of row tile 0, column group 0
     * withholds its hand-over (arrival / granules), so that its consumers run into their bounded wait and raise the gave-up
     * word: the failure path must be loud and must leave the device usable. */
    int debug;
} rpo_split_update;


int rpo_split_critic_fwd_a(const rpo_split_update* u, void* stream);
int rpo_split_critic_fwd_b(const rpo_split_update* u, void* stream);
/* CartSafe-v0 only: rpo_split_critic_fwd_a + rpo_split_critic_fwd_b + rpo_split_critic_bwd_a as ONE launch -- the later
 * stages' workgroups are extra planes of the grid that wait (tile_sync) for the workgroups of their own row tile instead of
 * for a launch boundary (the three stages hand over row-tile-local data only; bwd_b needs every row and stays a launch).  Same
 * values bit for bit (rpo_ddpg.py:163-185 / rpo_sac.py:167-196 up to the TD target's inputs).  Requires that the
 * dispatcher places all workgroups of a row tile on one XCD (rpo_xcc_probe). */
int rpo_split_critic_front(const rpo_split_update* u, void* stream);
/* ... + rpo_split_policy_a as one more plane (policy iteration without a shared embedding, like rpo_split_critic_fwd_b_pol:
 * the caller then skips rpo_split_policy_a; requires part_pol) */
int rpo_split_critic_front_pol(const rpo_split_update* u, void* stream);
/* SpringPendulum-v0: rpo_split_critic_fwd_b + rpo_split_critic_bwd_a as ONE launch in the same way (the batch-coupled
 * projection, rpo_split_pend_head_project, needs every row and keeps fwd_a a launch of its own); _pol: + rpo_split_policy_a. */
int rpo_split_critic_mid(const rpo_split_update* u, void* stream);
int rpo_split_critic_mid_pol(const rpo_split_update* u, void* stream);
/* SpringPendulum-v0: rpo_split_critic_fwd_a + rpo_split_pend_head_project + rpo_split_critic_fwd_b + rpo_split_critic_bwd_a as ONE
 * launch (requires proj_ws, batch <= 256, max_steps <= 30).  The projection is one workgroup per row tile (all on one XCD); what
 * crosses XCDs -- the policy's head partials into it, the projected actions and log pi out of it -- travels as tagged 8-byte
 * granules in proj_ws with agent-scope stores and loads (nothing depends on placement); the row-tile-local hand-overs use
 * tile_sync like rpo_split_critic_front.  Same values bit for bit.  _pol: + rpo_split_policy_a as one more plane. */
int rpo_split_critic_pfront(const rpo_split_update* u, void* stream);
int rpo_split_critic_pfront_pol(const rpo_split_update* u, void* stream);
/* out[x + gx * (y + gy * z)] = the XCD (XCC_ID) workgroup (x, y, z) of a (gx, gy, gz) grid of `threads`-thread workgroups ran
 * on.  rpo_split_critic_front hands data from workgroup to workgroup through ONE XCD's L2; its caller checks with this probe
 * (same grid: 8, ceil(batch / 16), 1 + 3 K; 256 threads) that all workgroups of a row tile share an XCD. */
int rpo_xcc_probe(int gx, int gy, int gz, int threads, int* out, void* stream);
/* Diagnostic (tools/hw_probe.py): out[...] = (XCC_ID << 16) | HW_ID[15:0] (wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13) of
 * the first wave of every workgroup of a grid whose workgroups hold lds_bytes of LDS and stay resident for `spin` sleep rounds:
 * how many workgroups the dispatcher stacks on one CU / SIMD while others are empty. */
int rpo_hw_probe(int gx, int gy, int gz, int threads, int lds_bytes, int spin, int* out, void* stream);
/* fwd_b + pol_a in one launch (policy iterations, no shared state embedding: the policy slabs on the batch states need
 * nothing the critic update produces); the caller then skips rpo_split_policy_a.  Requires part_pol. */
int rpo_split_critic_fwd_b_pol(const rpo_split_update* u, void* stream);
int rpo_split_pend_head_project(const rpo_split_update* u, void* stream);
int rpo_split_critic_bwd_a(const rpo_split_update* u, void* stream);
int rpo_split_critic_bwd_b(const rpo_split_update* u, void* stream);
int rpo_split_policy_a(const rpo_split_update* u, void* stream);
int rpo_split_policy_b(const rpo_split_update* u, void* stream);
int rpo_split_policy_c(const rpo_split_update* u, void* stream);
int rpo_split_policy_d(const rpo_split_update* u, void* stream);
int rpo_split_policy_e(const rpo_split_update* u, void* stream);
/* rpo_split_policy_a + _b + _c + _d as ONE launch, like rpo_split_critic_front (tile_sync; both envs: the actor loss completes the
 * action without projection steps, rpo_ddpg.py:307-312, so nothing couples the rows); _bc: pol_a already ran inside the
 * critic update's launch (rpo_split_critic_front_pol / _fwd_b_pol / _mid_pol).  Same values bit for bit. */
int rpo_split_policy_front(const rpo_split_update* u, void* stream);
int rpo_split_policy_front_bc(const rpo_split_update* u, void* stream);

/* ---- Rollout stages riding on the critic update's launches ---------------------------------------------------------------
 * Vector step t+1 of the loop (rpo_ddpg.py:93-145) reads nothing the critic update of step t writes when the policy and
 * the critics share no parameters and no policy step lies in between; the update stages above read their own clock
 * (`ctrl` of rpo_split_update), so the two can run side by side.  Instead of a second stream (on one MI355X the fork /
 * join of a hipGraph branch costs more than the 16 us rollout it hides) the rollout's work is handed to workgroups the
 * update launches leave idle:
 *   rpo_split_critic_fwd_a_ride, rpo_split_critic_fwd_b_ride
 *       = the stage + the actor's hidden slabs on the observations of lanes [lane_begin, lane_end) (8 column groups x
 *         lanes / 16 workgroups of 128 threads; partials to `part`).  The forward touches neither the ring nor anything
 *         the update writes, so it may ride anywhere; split over two launches it stays in their shadow.
 *   rpo_split_critic_bwd_b_ride
 *       = the stage + head -> exploration noise / rsample -> box clip -> equation solver -> GRG projection -> env step ->
 *         replay scatter -> statistics -> auto-reset of ALL lanes (one thread per lane, 256 lanes per workgroup);
 *         advances r->ctrl[RPO_CTRL_T].  Must follow rpo_split_critic_fwd_a(_ride) of the same update, which gathers
 *         the batch out of the ring this stage writes into, and forward stages covering every lane.
 * Together they compute exactly what rpo_cartsafe_rollout / rpo_pendulum_rollout compute (same bits: the slab forward is
 * bitwise the row-tile forward and the lane functions are the same code).  u->actor is the rollout policy; u must not
 * have a shared state embedding.  Fields as in rpo_*_rollout. */
typedef struct {
    int n_envs;
    int gauss;                   /* 0: tanh box + exploration noise (RPODDPG), 1: squashed-Gaussian sample (RPOSAC) */
    float scale, base;
    float* state;                /* CartSafe-v0: state [n_envs, 6]; SpringPendulum-v0: internal state [n_envs, 4] */
    float* obs;                  /* SpringPendulum-v0: observation out [n_envs, 5] or NULL; CartSafe-v0: NULL */
    float* action;               /* [n_envs, 2] */
    int* ep_len; float* ep_ret; unsigned* ep_count;
    float* rows; long long cap_steps;             /* replay ring (may be NULL) */
    float* stats; int stats_cap;
    int noise_mode;
    long long* ctrl;             /* the ROLLOUT clock (ctrl[RPO_CTRL_T] = vector steps taken) */
    float eps_start, eps_end, eps_decay, box_lo, box_hi;
    int max_steps; float corr_lr, corr_eps, corr_momentum;
    int max_episode_steps, auto_reset;
    float viol_thresh;
    unsigned env_id_base;
    unsigned long long seed;
    float* part;                 /* [8, n_envs, 2] head partials of the actor between the forward stages and the step */
    int lane_begin, lane_end;    /* forward stages: the lanes of this launch (multiples of 16; lane_end may be n_envs) */
    int defer_clock;             /* step stage: as in rpo_*_rollout -- 1: ctrl[RPO_CTRL_T] is advanced by the next fwd_a */
} rpo_rollout_rider;

int rpo_split_critic_fwd_a_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);
int rpo_split_critic_fwd_b_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);
int rpo_split_critic_bwd_b_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);
/* CartSafe-v0: rpo_split_critic_front with the actor forward of lanes [lane_begin, lane_end) riding in the planes behind its
 * own (replaces fwd_a_ride + fwd_b_ride + bwd_a; bwd_b_ride follows with the lanes' step). */
int rpo_split_critic_front_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);
/* SpringPendulum-v0: rpo_split_critic_mid with riding planes (replaces fwd_b_ride + bwd_a). */
int rpo_split_critic_mid_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);
/* SpringPendulum-v0: rpo_split_critic_pfront with riding planes (replaces fwd_a_ride + pend_head_project + mid_ride). */
int rpo_split_critic_pfront_ride(const rpo_split_update* u, const rpo_rollout_rider* r, void* stream);

/* Backward of the same rows given dout [n, n_out] (two launches).  Parameter gradients are ACCUMULATED (+=) into
 * grad_host's buffers (the shared state embedding of shared_param=True receives contributions from two networks,
 * agent/ddpg_pa.py:34-36).  dh [n, H] and dx0 [n, Ein] are caller-provided scratch; da [n, A] (may be NULL) receives
 * the gradient w.r.t. the action input (actor loss: -Q(s, a) back to the policy, rpo_ddpg.py:317).
 * param_grads = 0: only dx0 / da; first_layer_state_only = 1: of the parameters only Ws / bs are accumulated.
 * dh / dx0 are SCRATCH of the two-pass kernels: from RPO_SPLITK_FROM rows the streaming kernels (mlp_bwd_stream.h) keep both in
 * registers and leave the buffers untouched -- a caller must not read them back.
 * gradmax (may be NULL; [RPO_GRADMAX_LEN]): its slots receive max(slot, max |gradient element written by this call|) -- when the buffers were
 * zero before the call this is clip_grad_norm_'s inf-norm of the network (rpo_ddpg.py:180), without the rpo_absmax pass. */
int rpo_mlp_backward(const rpo_mlp* net_host, const rpo_mlp_grad* grad_host, int n, const float* s, int s_stride,
                     const float* a, int a_stride, const float* x0, const float* h1, const float* dout, float* dh,
                     float* dx0, float* da, int param_grads, int first_layer_state_only, float* gradmax,
                     const rpo_td* td, void* stream);

/* rpo_mlp_backward of two networks of the same shape on the same inputs in one pair of launches (SAC's twin critics,
 * model/value.py:125-140): gridDim.y = 2 selects the network.  Results are those of two rpo_mlp_backward calls. */
int rpo_mlp_backward_pair(const rpo_mlp* net1_host, const rpo_mlp_grad* grad1_host, const rpo_mlp* net2_host,
                          const rpo_mlp_grad* grad2_host, int n, const float* s, int s_stride, const float* a,
                          int a_stride, const float* x0_1, const float* h1_1, const float* dout_1, float* dh_1,
                          float* dx0_1, float* da_1, const float* x0_2, const float* h1_2, const float* dout_2, float* dh_2,
                          float* dx0_2, float* da_2, int param_grads, int first_layer_state_only, float* gradmax,
                          const rpo_td* td1, const rpo_td* td2, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * EVOPF-v0 (rpo_amd/csrc/evopf.hip): one wavefront per env lane / batch row; the lane's 22x22 Newton system and the
 * 28x28 block of the equality Jacobian are eliminated in registers, one matrix row per thread (evopf_dev.h).  state [n,57], action [n,43], basic actions [n,14];
 * consts_dev = the RPO_EVOPF_C_* buffer in device memory; state_stride = floats between consecutive state rows (57 for a
 * dense matrix, RPO_EVOPF_ROW when the states are columns of gathered replay rows).  The IEEE-14 bus classification is compiled in, like the
 * reference hard-wires case14 (evopf.py:211,336-337).
 * ------------------------------------------------------------------------------------------------------------- */

/* EVOPFEnv.reset (evopf.py:369-380): hour 0 of episode ep_count[i] (NULL: 0) of lane env_id_base + i; the loaders'
 * random draws (demand.py:53-62, price.py:41-43) come from Philox(seed; env, episode, RPO_STREAM_EVOPF_*). */
int rpo_evopf_reset(int n_envs, float* state, int* ep_len, float* ep_ret, const unsigned* ep_count,
                    const float* consts_dev, unsigned long long seed, unsigned env_id_base, void* stream);

/* EVOPFEnv.step (evopf.py:348-366) + Battery.step (:74-102) + run-loop bookkeeping (rpo_ddpg.py:120-145); same contract
 * as rpo_cartsafe_step: transition rows [RPO_EVOPF_ROW] scattered into the ring, statistics, ctrl[T] advanced by the
 * last workgroup, auto-reset.  An episode ends when the loaders run out of data after 24 hours (demand.py:71). */
int rpo_evopf_step(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count,
                   float* rows, long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps,
                   int auto_reset, float viol_thresh, const float* consts_dev, unsigned long long seed,
                   unsigned env_id_base, void* stream);

/* Scenarios: a caller's days instead of the Philox draws (an evaluation seam; additive, RPO_ABI_VERSION stays 6).  A scenario
 * table is float [days, RPO_EVOPF_SCEN_DAY]: floats [0, 48) of a day = the price of hours 0..47 in the observation's units
 * (24..47: the look-ahead past midnight), floats [48 + 28 t, 48 + 28 t + 28) = (pd[14], qd[14]) of hour t per unit; day [n]
 * (int) = the table row lane i plays.  Hour t < 24 of the observation: [0, 28) = demand[t], [33 + k] = price[t + k]; t >= 24:
 * zero.  A day[i] outside [0, days) never indexes the table: the lane's observation becomes NaN (ctrl[RPO_CTRL_NONFINITE]).
 * Refused before any launch: n <= 0, days <= 0 (RPO_ERR_ARG), a NULL among the required pointers (RPO_ERR_NULL), and what
 * rpo_evopf_step refuses. */

/* The day lane env_id_base + i is dealt in episode ep_count[i] (NULL: 0) under `seed`, written in the table layout by the device
 * function rpo_evopf_reset / rpo_evopf_step draw with (the same bits); price hours 24..47 are zero.  table_out [n, 720]. */
int rpo_evopf_scenario_table(int n, float* table_out, const unsigned* ep_count, const float* consts_dev, unsigned long long seed,
                             unsigned env_id_base, void* stream);

/* rpo_evopf_reset with hour 0 of table row day[i]; state of charge as there. */
int rpo_evopf_reset_scenario(int n_envs, float* state, int* ep_len, float* ep_ret, const float* table, int days, const int* day,
                             const float* consts_dev, void* stream);

/* rpo_evopf_step with the next hour read from table row day[i]; never auto-resets (ep_count is left as it is).  Everything else
 * is that step: violations, reward, battery, transition row, statistics, failure flag. */
int rpo_evopf_step_scenario(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count,
                            float* rows, long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps,
                            float viol_thresh, const float* consts_dev, const float* table, int days, const int* day, void* stream);

/* Scenario bank: TRAINING on a caller's days (additive, RPO_ABI_VERSION stays 6).  `table` is a scenario table as above, used as
 * a bank: lane env_id_base + i plays in episode e the row
 *   deal RPO_EVOPF_DEAL_UNIFORM: umulhi(word 0 of Philox(seed; env id, e, RPO_STREAM_EVOPF_DAY, 0), days)
 *   deal RPO_EVOPF_DEAL_CYCLE:   (env id + (64-bit) e * stride) mod days, stride = the run's total lane count
 * -- a pure function of (seed, env id, episode): no per-lane day array exists, ep_count is the whole state.  Refused before any
 * launch: n <= 0, days < 1, a deal other than these two, stride < 1 with the cycle (RPO_ERR_ARG), a NULL among the required
 * pointers (RPO_ERR_NULL; ep_count may be NULL where rpo_evopf_reset allows it: episode 0), and what rpo_evopf_step refuses. */
#define RPO_EVOPF_DEAL_UNIFORM 0
#define RPO_EVOPF_DEAL_CYCLE 1

/* rpo_evopf_reset with hour 0 of the day dealt for episode ep_count[i]; state of charge as there. */
int rpo_evopf_reset_bank(int n_envs, float* state, int* ep_len, float* ep_ret, const unsigned* ep_count, const float* table, int days,
                         int deal, int stride, unsigned long long seed, unsigned env_id_base, void* stream);

/* rpo_evopf_step (its whole argument list, auto_reset included) with the episode data read from the bank: the next hour from the
 * day of episode ep_count[i], and at done && auto_reset hour 0 of the day of episode ep_count[i] + 1. */
int rpo_evopf_step_bank(int n_envs, float* state, const float* action, int* ep_len, float* ep_ret, unsigned* ep_count, float* rows,
                        long long cap_steps, float* stats, int stats_cap, long long* ctrl, int max_episode_steps, int auto_reset,
                        float viol_thresh, const float* consts_dev, unsigned long long seed, unsigned env_id_base, const float* table,
                        int days, int deal, int stride, void* stream);

/* day_out[i] (int [n]) = the bank row lane env_id_base + i plays in episode ep_count[i] (NULL: 0): what the two kernels above
 * compute, for the host to ask which day a lane is on. */
int rpo_evopf_bank_days(int n, const unsigned* ep_count, int days, int deal, int stride, unsigned long long seed, unsigned env_id_base,
                        int* day_out, void* stream);

/* take_action's noise + clip to the state-dependent box (agent/ddpg_pa.py:101-112; EVOPFEnv.update evopf.py:769-783)
 * -> complete_partial = Newton power flow (PFFunction.forward, evopf.py:789-855; newton_tol 1e-5, newton_max_iters 50)
 * -> grad_steps (rpo_ddpg.py:266-305, corr_mode 0).  Every row carries its own Newton and GRG stop tests (== the
 * reference's B = 1 rollout calls; on a batch the reference tests the batch maximum, which adds iterations only to
 * rows that had already met the test).  iters [n] (may be NULL) = GRG iterations.  Noise draw of basic action j:
 * Philox(seed; env, ctrl[T], RPO_STREAM_ACT, j / 2) normals (x,y) | (z,w); RPO_NOISE_UNIFORM: word j % 4 of block j / 4.
 * ap_is_raw = 1: ap_raw holds the actor's pre-activation outputs and the kernel applies BoxConstraint's map
 * scale(s) * tanh(.) + base(s) with the lane's own box first (model/utils.py:40-51,75-88). */
int rpo_evopf_act_project(int n, const float* state, int state_stride, const float* ap_raw, const float* noise, float* action, int* iters,
                          int noise_mode, int ap_is_raw, float eps_start, float eps_end, float eps_decay, int max_steps,
                          float corr_lr, float corr_eps, float corr_momentum, float newton_tol, int newton_max_iters,
                          const float* consts_dev, unsigned long long seed, unsigned env_id_base, const long long* ctrl,
                          float* stats, int stats_cap, void* stream);

/* The projection profile of RPOTrainerBase.act(profile=True) on EVOPF-v0 (schedule profile_evopf=1): rpo_evopf_act_project under
 * RPO_NOISE_NONE (its arguments without the noise, the generator, ctrl and stats; ap_raw [n,14] is required) that also writes
 * every budget 0..K of the projection, K = max_steps >= 0, in ONE launch.  profile [K + 1, n, 4], 16-byte aligned: plane b, row
 * i = (a[0], a[1], eq*, ineq*) of the row's iterate after min(b, iters[i]) GRG iterations, one non-temporal 16-byte store per row
 * and plane, with the residuals of rpo_evopf_resid (its bits): ineq* = the largest of the 58 inequality residuals (a NaN among
 * them is returned, as torch.max does); eq* = the equality residual of largest magnitude with its sign, the lowest index among
 * equal magnitudes, the first NaN if there is one.  Every plane of every row is written (a row whose stop test has fired
 * repeats its final entry): the buffer needs no zeroing.  action [n,43] and iters [n] (may be NULL) are those of the budget K.
 * == for b = 0..K: rpo_evopf_act_project(RPO_NOISE_NONE, max_steps = b) + rpo_evopf_resid, bit for bit.
 * Refused before any HIP call: n <= 0, max_steps < 0, newton_max_iters <= 0, state_stride < RPO_EVOPF_STATE (RPO_ERR_ARG); a NULL
 * state, ap_raw, action, consts_dev or profile (RPO_ERR_NULL); a profile that is not 16-byte aligned, or of more than
 * RPO_TRACE_MAX_BYTES = 16 (K + 1) n bytes (RPO_ERR_ARG). */
int rpo_evopf_project_profile(int n, const float* state, int state_stride, const float* ap_raw, int ap_is_raw,
                              float* action, int* iters, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                              float newton_tol, int newton_max_iters, const float* consts_dev, float* profile, void* stream);

/* Backward of the actor's output map for EVOPF: ap = clip(scale(s) * tanh(raw) + base(s) + eps_t * noise, lo(s), hi(s))
 * (model/policy.py:24-33 with the state-dependent box, then ddpg_pa.py:108-110); dout [n,14] = dap * d ap / d raw.
 * noise NULL: no noise and no clip. */
int rpo_evopf_tanh_box_bwd(int n, const float* state, int state_stride, const float* raw, const float* noise,
                           float eps_start, float eps_end, float eps_decay, const long long* ctrl, const float* dap,
                           float* dout, const float* consts_dev, void* stream);

/* RPOSAC's policy head on EVOPF: squashed Gaussian with the state-dependent box (model/policy.py:53-66 with
 * BoxConstraint.update_box; the clip of agent/sac_pa.py:111).  raw [n,28] = (mean heads [14] | log-std heads [14]) from
 * rpo_mlp_forward (head_dim 14, n_out 2), eps [n,14]; ap_out [n,14], logp_out [n] (sum over the 14 dimensions, may be
 * NULL); the backward writes draw [n,28] given dap [n,14] and dlogp = coefficient of log pi in the loss. */
int rpo_evopf_gauss_head(int n, const float* state, int state_stride, const float* raw, const float* eps, int deterministic,
                         float* ap_out, float* logp_out, const float* consts_dev, void* stream);
int rpo_evopf_gauss_head_bwd(int n, const float* state, int state_stride, const float* raw, const float* eps,
                             const float* dap, float dlogp, float* draw, const float* consts_dev, void* stream);

/* PFFunction.backward (evopf.py:857-910): grad_ap [n,14] = dL/dz given grad_action [n,43] = dL/dy and the completed
 * action; the Jacobians are re-evaluated at that action (the reference keeps those of the last Newton point). */
int rpo_evopf_complete_bwd(int n, const float* action, const float* grad_action, const float* grad_action_b, const float* grad_action2,
                           float* grad_ap, const float* consts_dev, void* stream);
/*   dL/dy = (grad_action [+ grad_action_b]) [+ grad_action2]: grad_action_b (NULL, or the second twin critic's [n,43] term) and
 *   grad_action2 (NULL, or the Lagrangian's) are added inside the kernel, in that order. */

/* eq_resid [n,28] (evopf.py:520-546) and ineq_resid [n,58] (signed, :548-563); either output may be NULL. */
int rpo_evopf_resid(int n, const float* state, int state_stride, const float* action, float* eq_out, float* ineq_out,
                    const float* consts_dev, void* stream);

/* ineq_partial_grad [n,43] (evopf.py:596-612): reduced gradient of the number of violated inequalities. */
int rpo_evopf_ineq_partial_grad(int n, const float* state, int state_stride, const float* action, float* step_out, const float* consts_dev,
                                void* stream);

/* grad_action [n,43] = J_eq(action)^T grad_eq [n,28] with the entries of eq_jac (evopf.py:614-661): the backward of
 * eq_resid in the Lagrangian baselines' actor loss (ddpg_lag.py:257-263).  autograd_sign != 0 gives the battery columns
 * the sign torch autograd derives from the residual's +pe (evopf.py:532) instead of eq_jac's -I (:639-640). */
int rpo_evopf_eq_vjp(int n, const float* action, const float* grad_eq, float* grad_action, int autograd_sign,
                     const float* consts_dev, void* stream);

/* scale * sum_b sum_j nu_j relu(g_j(s_b, a_b)) accumulated into loss_out, d/d action into grad_action [n,43] (written),
 * d/d nu accumulated into grad_nu [58] (rpo_ddpg.py:312-319, dual.py:63-65). */
int rpo_evopf_lagrangian(int n, const float* state, int state_stride, const float* action, const float* nu, float scale, float* loss_out,
                         float* grad_action, float* grad_nu, const float* consts_dev, int overwrite, void* stream);
/* (overwrite != 0: loss_out is written instead of accumulated -- one launch instead of a fill + this one; grad_nu accumulates) */

/* Policy evaluation on EVOPF-v0 (RPOTrainerBase.evaluate under schedule fused_eval_evopf=1; csrc/evopf_eval.hip): env steps
 * [t0, t0 + steps) of n_envs independent episodes in one launch that loops over the steps inside each workgroup (4 waves = 4
 * episodes): the 57 -> 256 -> 256 -> 14 actor layer by layer on the workgroup's four observation rows, with the ordered MFMA
 * chains and the summation order of rpo_mlp_forward's layer-by-layer launches -> tanh box (gauss = 0: one head) | mean head
 * (gauss = 1: two heads) in the state-dependent box -> complete_partial -> grad_steps (max_steps iterations, no noise) -> env
 * step + violations + TimeLimit (no auto-reset, no replay row, no statistics row) -> acc [n_envs, RPO_EVAL_LEN] (t0 == 0
 * writes a row from scratch) and, with con != NULL, the per-constraint report con [n_envs, 144] (layout RPO_CON_*; 16-byte
 * aligned).  A lane whose episode has ended is not stepped again; a workgroup whose lanes have all ended returns.  The host
 * enqueues the launches back to back, t0 = 0, steps, 2 * steps, ...; the split changes no bit.
 * == per step: rpo_mlp_forward (n <= 16384, RPO_TUNE_MLP_GEMM and RPO_TUNE_GEMM_KSPLIT at their defaults)
 *    [+ rpo_evopf_gauss_head(deterministic)] + rpo_evopf_act_project(RPO_NOISE_NONE, ap_is_raw = !gauss, iters) +
 *    rpo_evopf_step(auto_reset 0, cap_steps 1) [+ rpo_eval_constraints] + rpo_eval_accumulate, bit for bit.
 * Refused before any HIP call: a NULL actor_host (RPO_ERR_NULL); n_envs <= 0, steps <= 0, t0 < 0, max_episode_steps <= 0,
 * max_steps < 0, newton_max_iters <= 0 (RPO_ERR_ARG); a NULL state, action, ep_len, ep_ret, ep_count, acc or consts_dev
 * (RPO_ERR_NULL); a con that is not 16-byte aligned (RPO_ERR_ARG); an actor that is not S = 57, E = H = 256 with 14 outputs per
 * head, one head (gauss = 0) or two (RPO_ERR_ARG).  ctrl (may be NULL) receives ctrl[RPO_CTRL_NONFINITE] like rpo_evopf_step;
 * ctrl[RPO_CTRL_T] is neither read nor advanced. */
int rpo_evopf_evaluate(const rpo_mlp* actor_host, int gauss, int n_envs, float* state, float* action, int* ep_len, float* ep_ret,
                       unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, int max_steps, float corr_lr,
                       float corr_eps, float corr_momentum, float newton_tol, int newton_max_iters, const float* consts_dev,
                       int max_episode_steps, float viol_thresh, unsigned long long seed, unsigned env_id_base, float* con,
                       void* stream);

/* Single-step AC optimal power flow on EVOPF-v0 (EVOPFEnv.opf / opt_solve, EvalTrajectory.opf_gap; csrc/evopf_opf.hip): for
 * each of n states the cheapest (pg, qg, vm, va) that meets eq_resid = 0 and the bounds on pg, qg, vm, for the demand in the
 * first 28 floats of the row of obs (obs_stride >= 28 floats between rows: [n,57] observations, [n,28] demands or a column
 * slice of something wider) and the battery power pe [n,5] (NULL: zeros), which is data of the problem and not a variable.  What
 * the reference asks of pypower (evopf.py:729-759), as a MIPS-style primal-dual interior point method from the flat start, one
 * wavefront per state, float32; the reduced KKT system of order 55 is eliminated in registers, one row per lane.
 * action_out [n,43]: the full action vector (va at the slack bus = slack_va, pe as given), so eq_resid / ineq_resid / obj_fn
 * apply to it; info_out [n,4] = (cost, the largest of the three stop quantities at exit, iterations, converged 0 / 1).  The stop
 * test: max(|g|_inf, max h), |L_x|_inf and z^T mu all below tol; a row that does not meet it leaves after max_iters iterations
 * with converged = 0 (max_iters = 0: the flat start).  A row's output does not depend on the other rows of the launch.  Reads obs,
 * pe and consts_dev, writes the two outputs, nothing else.
 * Refused before any HIP call, sizes before pointers: n <= 0, max_iters < 0, tol <= 0 (or NaN), obs_stride < 28 (RPO_ERR_ARG); a
 * NULL obs, action_out, info_out or consts_dev (RPO_ERR_NULL). */
int rpo_evopf_opf(int n, const float* obs, int obs_stride, const float* pe, float* action_out, float* info_out, float tol,
                  int max_iters, const float* consts_dev, void* stream);

/* The same kernel with its iterate visible: rpo_evopf_opf plus state_in / state_out [n, RPO_EVOPF_OPF_STATE] floats, either may
 * be NULL (both NULL: rpo_evopf_opf).  A row is
 *     action[43] | lambda[28] | z_u[24] | z_l[24] | mu_u[24] | mu_l[24] | gamma[1]
 * with the bounded variables in the order pg[5], qg[5], vm[14].  With state_in the row replaces the flat start entirely (x with pe
 * and the slack angle, lambda, slacks, multipliers, gamma) and iterations count from it; pe must then be NULL (RPO_ERR_ARG, before
 * any HIP call, like the other refusals).  state_out receives the state at exit, the one the stop test was last evaluated on
 * (state_out[:, :43] = action_out).  For holding the solver one iteration at a time (tests/test_evopf_opf_f64_gpu.py). */
#define RPO_EVOPF_OPF_STATE 168
int rpo_evopf_opf_state(int n, const float* obs, int obs_stride, const float* pe, float* action_out, float* info_out, float tol,
                        int max_iters, const float* consts_dev, const float* state_in, float* state_out, void* stream);

/* The single-step AC-OPF with the battery power a VARIABLE (EVOPFEnv.opf(pe="free"), evaluate_opf; the free-pe instance of the
 * same kernel): for each of n observations (obs_stride >= 57 floats between rows: the demand, the five states of charge and the
 * current price of the row are read) minimise obj_fn(pg) + sum_j pe_cost[j] pe[j] over (pg, qg, vm, va, pe[5]) subject to
 * eq_resid = 0, the 48 bounds on pg, qg, vm and the 10 battery bounds battery_bounds(soc) that ineq_resid uses.  pe_cost [n,5], or
 * NULL: (we / wg) * price of the row in every component, with which the optimum maximises the env's one-step reward.  pe enters
 * the real-power equation of its generator bus with derivative +1, as eq_resid adds it (not eq_jac's -1).  Same method, flat
 * start (pe at the middle of its box), stop test and outputs as rpo_evopf_opf with 58 inequalities; action_out [n,43] carries
 * the optimal pe in columns 38..42, info_out [n,4] column 0 stays obj_fn of the returned point.  An empty battery box (a state of
 * charge far outside its band) ends as not converged at max_iters.  No state seam.  A row's output does not depend on the other
 * rows of the launch.  Reads obs, pe_cost and consts_dev, writes the two outputs, nothing else.
 * Refused before any HIP call, sizes before pointers: n <= 0, max_iters < 0, tol <= 0 (or NaN), obs_stride < 57 (RPO_ERR_ARG); a
 * NULL obs, action_out, info_out or consts_dev (RPO_ERR_NULL). */
int rpo_evopf_opf_free(int n, const float* obs, int obs_stride, const float* pe_cost, float* action_out, float* info_out, float tol,
                       int max_iters, const float* consts_dev, void* stream);

/* The safety filter of EVOPF-v0 (EVOPFEnv.nearest_feasible, evaluate_filtered; a third instance of the same kernel; additive,
 * RPO_ABI_VERSION stays 6): for each of n observations the dispatch NEAREST to a given action that meets eq_resid = 0 and all 58
 * bounds of ineq_resid -- minimise 0.5 sum_k w_k (y_k - t_k)^2 over (pg, qg, vm, va, pe[5]) with the constraint set of
 * rpo_evopf_opf_free, k over the 14 components the actor controls in the env's partial_actions order: pg of generators 1..4, vm at
 * the five generator buses, pe[5].  target [n, >= 43] rows in the layout of an action (target_stride floats between rows); only
 * those 14 components are read.  weight NULL: w_k = 1 / s_k^2 with s_k the half-width of the variable's own box in this problem (per
 * row for pe), 0 where s_k <= 1e-6 -- the distance in box units; else a table of 14 floats per row in that order, weight_stride 0
 * (one row for all) or 14, every value a finite number > 0 (anything else, like a NaN in the row's target or observation, ends
 * that row as not converged at max_iters and touches no other row).  Same method, flat start (the target is NOT the start), stop
 * test and signs as rpo_evopf_opf_free; action_out [n,43] the full action vector, info_out [n,4] = (the objective at exit, the
 * largest of the three stop quantities at exit, iterations, converged 0 / 1).  A row's output does not depend on the other rows of
 * the launch.  Reads obs, target, weight and consts_dev, writes the two outputs, nothing else.
 * Refused before any HIP call, sizes before pointers: n <= 0, max_iters < 0, tol <= 0 (or NaN), obs_stride < 57, target_stride <
 * 43, weight_stride neither 0 nor 14 (RPO_ERR_ARG); a NULL obs, target, action_out, info_out or consts_dev (RPO_ERR_NULL). */
int rpo_evopf_nearest(int n, const float* obs, int obs_stride, const float* target, int target_stride, const float* weight,
                      int weight_stride, float* action_out, float* info_out, float tol, int max_iters, const float* consts_dev,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused pipelines of one RPO iteration (rpo_amd/csrc/fused.hip): the row-local stages chained
 * inside one workgroup of 16 rows, because at 4096 lanes / batch 256 every launch is dominated by dispatch + cold-start
 * latency.  Bitwise identical to the sequences of single-stage launches they replace.
 * ------------------------------------------------------------------------------------------------------------- */

/* Rollout of one vector step (rpo_ddpg.py:93-145, rpo_sac.py:95-150): actor MLP -> policy head -> complete_partial ->
 * grad_steps -> env step + violations + TimeLimit -> replay scatter -> statistics -> auto-reset.
 * gauss = 0 (RPODDPG, agent/ddpg_pa.py:108-110): the actor's tanh-box output + noise_mode's exploration noise + clip;
 *   == rpo_mlp_forward(actor, out_mode 1) + rpo_<env>_act_project(noise_mode) + rpo_<env>_step (same arguments).
 * gauss = 1 (RPOSAC, agent/sac_pa.py:105-115): actor has the two heads (mean, log-std); the rsample draw of lane i is
 *   normal(philox(seed, env_id_base + i, ctrl[T], RPO_STREAM_POLICY, ctrl[UPDATES])), i.e. rpo_philox_normal(salt 0);
 *   == rpo_philox_normal + rpo_mlp_forward(actor) + rpo_gauss_head + rpo_<env>_act_project(RPO_NOISE_NONE) + step.
 * CartSafe-v0: state [n,6] is the observation.  SpringPendulum-v0: internal [n,4], obs [n,5] (may be NULL: the
 * pipeline itself derives observations from the internal state).
 * defer_clock = 1: the launch does NOT advance ctrl[RPO_CTRL_T] / clear the next statistics row (two dependent atomic
 *   round trips behind its last workgroup, ~1.5 us); the caller's NEXT launch on the stream does it instead --
 *   rpo_split_critic_fwd_a with `rollout_ctrl` set (one plain store, no arrival counting: a later launch starts after
 *   every workgroup of this one has finished). */
int rpo_cartsafe_rollout(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                         float* action, int* ep_len, float* ep_ret, unsigned* ep_count, float* rows, long long cap_steps,
                         float* stats, int stats_cap, long long* ctrl, int noise_mode, float eps_start, float eps_end,
                         float eps_decay, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                         float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                         int auto_reset, float viol_thresh, unsigned long long seed, unsigned env_id_base, int defer_clock,
                         void* stream);
int rpo_pendulum_rollout(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                         float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, float* rows,
                         long long cap_steps, float* stats, int stats_cap, long long* ctrl, int noise_mode,
                         float eps_start, float eps_end, float eps_decay, float box_lo, float box_hi, int max_steps,
                         float corr_lr, float corr_eps, float corr_momentum, int max_episode_steps, int auto_reset,
                         float viol_thresh, unsigned long long seed, unsigned env_id_base, int defer_clock, void* stream);

/* Policy evaluation (RPOTrainerBase.evaluate, rpo_amd/algo/evaluation.py): env steps [t0, t0 + steps) of n_envs independent
 * episodes with eval()'s policy (rpo_ddpg.py:224-226, rpo_sac.py:238-240), in one launch that loops over the steps inside
 * each workgroup: actor MLP -> tanh box (gauss = 0) | mean head clip(scale * tanh(mean) + base, box_lo, box_hi) (gauss = 1)
 * -> complete_partial -> grad_steps (max_steps iterations, no noise) -> env step + violations + TimeLimit (no auto-reset, no
 * replay row, no statistics row) -> the lane's accumulator row acc [n_envs, RPO_EVAL_LEN] (t0 == 0 writes it from scratch).
 * A lane whose episode has ended is not stepped again; a workgroup whose lanes have all ended returns.  The host enqueues
 * the launches back to back, t0 = 0, steps, 2 * steps, ...
 * == per step: rpo_mlp_forward (+ rpo_gauss_head(deterministic)) + rpo_<env>_act_project(RPO_NOISE_NONE, iters) +
 *    rpo_<env>_step(auto_reset 0, cap_steps 1) + rpo_eval_accumulate, bit for bit.
 * The actor: embed width E = 128, hidden 256 (RPO_ERR_ARG otherwise).
 * CartSafe-v0: state [n,6] is the observation.  SpringPendulum-v0: internal [n,4] and obs [n,5] (the observations the
 * actor and the projection read; rewritten by every step).  ctrl (may be NULL): receives ctrl[RPO_CTRL_NONFINITE] like the
 * step kernels'; ctrl[RPO_CTRL_T] is neither read nor advanced. */
int rpo_cartsafe_evaluate(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                          float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc, int t0,
                          int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                          float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                          float viol_thresh, void* stream);
int rpo_pendulum_evaluate(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                          float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                          float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                          float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, void* stream);

/* The same launches with a per-step record (layout RPO_TRACE_*, O = 6 | 5, P = 1, A = 2: W = 16): a live lane
 * i < trace_rows writes row (s, i) of trace [trace_steps, trace_rows, 16] at every step s of [t0, t0 + steps) -- the head
 * (the observation the actor and the projection read, the proposal, the projected action, the iteration count) before the env
 * step, the tail after it, as non-temporal 16-byte stores.  The accumulators, the env state and the actions are those of
 * rpo_<env>_evaluate, bit for bit; launches with t0 > 0 continue the same buffer.  trace: zeroed by the caller, 16-byte
 * aligned; 1 <= trace_rows <= n_envs and t0 + steps <= trace_steps (RPO_ERR_ARG otherwise). */
int rpo_cartsafe_evaluate_record(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                 float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                 int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                 float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                 float viol_thresh, float* trace, int trace_rows, int trace_steps, void* stream);
int rpo_pendulum_evaluate_record(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                 float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                 float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                 float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                 int trace_rows, int trace_steps, void* stream);

/* The same launches with the per-constraint report con [n_envs, W] (layout RPO_CON_*; W = 16 | 4; 16-byte aligned, RPO_ERR_NULL
 * / RPO_ERR_ARG otherwise): after the env step a live lane folds the step's ineq_viol / eq_viol -- the values of the
 * transition row rpo_<env>_step writes, bit for bit -- into its row with 16-byte loads and stores; launches with t0 > 0
 * continue the rows.  trace == NULL: no per-step record (trace_rows, trace_steps unused); otherwise the arguments and the
 * record of rpo_<env>_evaluate_record.  Accumulators, env state, actions and trace are those of the calls without con.
 * == per step: ... + rpo_eval_constraints in front of rpo_eval_accumulate, bit for bit. */
int rpo_cartsafe_evaluate_constraints(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                      float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                      float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                      float corr_eps, float corr_momentum, const float* consts_host, int partial,
                                      int max_episode_steps, float viol_thresh, float* trace, int trace_rows, int trace_steps,
                                      float* con, void* stream);
int rpo_pendulum_evaluate_constraints(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs,
                                      float* internal, float* obs, float* action, int* ep_len, float* ep_ret,
                                      unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, float box_lo,
                                      float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                      int max_episode_steps, float viol_thresh, float* trace, int trace_rows, int trace_steps,
                                      float* con, void* stream);

/* The same launches with observation noise (RPOTrainerBase.evaluate(obs_noise=)): at every step s the actor and the projection
 * of episode i read o~[q] = o[q] + sigma[q] * z(i, s, q) -- an f32 multiply, then an f32 add, not fused -- with z the Box-Muller
 * normal of words 0 and 1 of Philox(noise_seed; i, s, RPO_STREAM_EVAL_OBS + 0x100 * q, 0), keyed by the ABSOLUTE step: the
 * split of the horizon over launches changes nothing.  A column with sigma[q] == 0 is not drawn and keeps its bits.  The env
 * steps the TRUE state: rewards, violations, accumulators, the tail of the record and the report are those of the true state
 * under the action chosen from the noisy observation, and nothing of the noise reaches the env's state or observation rows;
 * the head of the record holds o~, what the policy read.  sigma_host: sigma_len = 6 | 5 host floats >= 0, copied into the
 * launch (NULL: RPO_ERR_NULL; another length, a negative or a non-finite entry: RPO_ERR_ARG, before any HIP call).  trace
 * and con may each be NULL (no record / no report); otherwise the arguments of rpo_<env>_evaluate_constraints.
 * == per step: rpo_eval_obs_noise(step s) in front of the launches of rpo_<env>_evaluate_constraints' sequence, the actor and
 *    the projection reading its output, bit for bit. */
int rpo_cartsafe_evaluate_noisy(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                float viol_thresh, float* trace, int trace_rows, int trace_steps, float* con,
                                const float* sigma_host, int sigma_len, unsigned long long noise_seed, void* stream);
int rpo_pendulum_evaluate_noisy(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                int trace_rows, int trace_steps, float* con, const float* sigma_host, int sigma_len,
                                unsigned long long noise_seed, void* stream);

/* The same launches with a projection budget PER LANE (RPOTrainerBase.evaluate_budgets): a live lane i projects with at most
 * lane_steps[i] GRG iterations at step size lane_lr[i] in place of max_steps / corr_lr, which are validated and otherwise
 * unused; corr_eps, corr_momentum and everything else stay launch-uniform.  lane_steps (int), lane_lr (float): DEVICE arrays
 * [n_envs], 4-byte aligned (NULL: RPO_ERR_NULL; misaligned: RPO_ERR_ARG, before any HIP call).  The arguments are those of
 * rpo_<env>_evaluate_constraints with con optional (NULL: no report); there is no record and no noise with it: trace must be
 * NULL (RPO_ERR_ARG otherwise; trace_rows, trace_steps unused).  With B budgets tiled group-major over n_envs = B * episodes
 * lanes that share their initial states, lane g * episodes + e is episode e under budget g: lanes never read one another, so
 * == rpo_<env>_evaluate[_constraints] of the episodes-lane env with max_steps = lane_steps[g], corr_lr = lane_lr[g], bit for
 *    bit, for every g. */
int rpo_cartsafe_evaluate_budgets(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                  float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                  int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                  float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                  float viol_thresh, float* trace, int trace_rows, int trace_steps, float* con,
                                  const int* lane_steps, const float* lane_lr, void* stream);
int rpo_pendulum_evaluate_budgets(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                  float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                  float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                  float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* trace,
                                  int trace_rows, int trace_steps, float* con, const int* lane_steps, const float* lane_lr,
                                  void* stream);

/* The same launches with an actor PER GROUP of lanes (RPOTrainerBase.evaluate_policies): P policies on the same initial
 * states in one launch sequence.  The n_envs lanes are P groups of group_lanes lanes, group-major; group g evaluates the
 * actor whose parameters lie g * policy_stride floats behind those of actor_host -- every non-NULL pointer of the descriptor
 * is advanced by that much, so actor_host describes policy 0 of a DEVICE bank [P, policy_stride] in which every policy has the
 * layout of policy 0.  Of every group the first `episodes` lanes are live; the others are padding: they are never stepped,
 * never keep a workgroup alive, and their rows of acc, con, action and of the env arrays are neither read into a result nor
 * written.  policy_stride: > 0 and a multiple of 4 (W0 of every policy stays 16-byte aligned); group_lanes: > 0 and a multiple
 * of 64 (no workgroup's lanes belong to two policies); 1 <= episodes <= group_lanes; n_envs a whole multiple of group_lanes
 * (RPO_ERR_ARG otherwise, before any HIP call).  The arguments are those of rpo_<env>_evaluate_constraints without a trace
 * and with con optional (NULL: no report); no record, no noise, one budget.  acc, con, action and the env arrays have
 * n_envs rows.  Lanes never read one another, so rows [g * group_lanes, g * group_lanes + episodes) are
 * == rpo_<env>_evaluate[_constraints] of the episodes-lane env with the g-th actor, bit for bit, for every g. */
int rpo_cartsafe_evaluate_policies(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                   float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl, float* acc,
                                   int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                   float corr_momentum, const float* consts_host, int partial, int max_episode_steps,
                                   float viol_thresh, float* con, int policy_stride, int group_lanes, int episodes,
                                   void* stream);
int rpo_pendulum_evaluate_policies(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* internal,
                                   float* obs, float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                   float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                   float corr_eps, float corr_momentum, int max_episode_steps, float viol_thresh, float* con,
                                   int policy_stride, int group_lanes, int episodes, void* stream);

/* The noisy launches with a sigma PER GROUP of lanes (RPOTrainerBase.evaluate_noise): S noise levels on the same episodes AND
 * the same draws in one launch sequence.  The n_envs lanes are S groups of group_lanes lanes, group-major; lane
 * g * group_lanes + e is episode e under level g: its actor and projection read o[q] + sigma_table[8 g + q] * z(e, s, q) with
 * the z of rpo_<env>_evaluate_noisy keyed by the EPISODE e within the group, not by the lane -- every level sees the draw that
 * rpo_<env>_evaluate_noisy on an episodes-lane env hands its lane e (common random numbers).  sigma_table: a DEVICE table
 * [S, 8] of floats >= 0, zero beyond the env's 6 | 5 observation columns, 4-byte aligned; a zero entry is not drawn and keeps
 * the column's bits, so an all-zero row is the clean evaluation (NULL: RPO_ERR_NULL; misaligned: RPO_ERR_ARG; the values are on
 * the device and are the caller's to check).  Of every group the first `episodes` lanes are live; the others are padding:
 * they are never stepped, never drawn for, never keep a workgroup alive, and their rows of acc, con, action and of the env
 * arrays are neither read into a result nor written.  group_lanes: > 0 and a multiple of 64 (no workgroup's lanes belong to
 * two levels); 1 <= episodes <= group_lanes; n_envs a whole multiple of group_lanes (RPO_ERR_ARG otherwise, before any HIP
 * call).  The arguments are those of rpo_<env>_evaluate_constraints without a trace and with con optional (NULL: no report);
 * no record, one budget, one actor.  The env steps the TRUE state, as in rpo_<env>_evaluate_noisy.  Lanes never read one
 * another, so rows [g * group_lanes, g * group_lanes + episodes) are
 * == rpo_<env>_evaluate_noisy of the episodes-lane env with sigma = sigma_table[8 g ..] and the same noise_seed (an all-zero
 *    row: rpo_<env>_evaluate[_constraints]), bit for bit, for every g. */
int rpo_cartsafe_evaluate_noise_sweep(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs, float* state,
                                      float* action, int* ep_len, float* ep_ret, unsigned* ep_count, long long* ctrl,
                                      float* acc, int t0, int steps, float box_lo, float box_hi, int max_steps, float corr_lr,
                                      float corr_eps, float corr_momentum, const float* consts_host, int partial,
                                      int max_episode_steps, float viol_thresh, float* con, const float* sigma_table,
                                      unsigned long long noise_seed, int group_lanes, int episodes, void* stream);
int rpo_pendulum_evaluate_noise_sweep(const rpo_mlp* actor_host, int gauss, float scale, float base, int n_envs,
                                      float* internal, float* obs, float* action, int* ep_len, float* ep_ret,
                                      unsigned* ep_count, long long* ctrl, float* acc, int t0, int steps, float box_lo,
                                      float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                                      int max_episode_steps, float viol_thresh, float* con, const float* sigma_table,
                                      unsigned long long noise_seed, int group_lanes, int episodes, void* stream);

/* The stepwise form of the noise (any env): out[i, q] = obs[i, q] + sigma[q] * z(i, step, q) for i < n, q < obs_dim, with the
 * draw and the arithmetic above (== per column q with sigma[q] != 0: rpo_philox_normal(n, ., seed, 0, step,
 * RPO_STREAM_EVAL_OBS + 0x100 * q, NULL), then the unfused multiply and add); a column with sigma[q] == 0 is copied.  obs
 * [n, obs_stride], out [n, out_stride] (strides >= obs_dim; columns beyond obs_dim are not touched), sigma: obs_dim DEVICE
 * floats.  out is a buffer of its own, never obs (RPO_ERR_ARG): CartSafe-v0's observation rows are the env's state.
 * 1 <= obs_dim <= 4096, 0 <= step < 2^24.  One thread per element, grid-stride. */
int rpo_eval_obs_noise(int n, const float* obs, int obs_stride, int obs_dim, const float* sigma, unsigned long long seed,
                       int step, float* out, int out_stride, void* stream);

/* Projected actions for caller-supplied observations (RPOTrainerBase.act, rpo_amd/algo/acting.py): n rows obs [n, obs_stride]
 * (obs_stride >= 6 | 5 floats) -> action [n, 2] (8-byte aligned), and where the pointer is not NULL: proposal [n] (what the
 * policy handed to the projection), iters [n] (GRG iterations of the row), eq_resid [n] and ineq_resid [n, 6 | 1] (signed,
 * at the returned action; CartSafe-v0: 8-byte aligned).  One launch, rows independent (per-row stop test), no env state, no
 * control word, no generator; the outputs leave as non-temporal stores.
 * == the sequence of launches rpo_mlp_forward (+ rpo_gauss_head(deterministic)) + rpo_<env>_act_project(RPO_NOISE_NONE,
 *    iters) + rpo_<env>_resid on the same rows, bit for bit.
 * form: 0 = chosen by n (row tile below RPO_ROLLOUT_STREAM_FROM rows, streaming from there, 64-row groups once every wave
 *   of the chip gets one), 1 = row tile (16 rows per workgroup, 64 from 12 288 rows), 2 = streaming with 16-row groups,
 *   3 = streaming with 64-row groups; RPO_ERR_ARG where the asked form does not apply.
 * The actor: embed width E = 128, hidden 256 (RPO_ERR_ARG otherwise); n > 0, max_steps >= 0 (0: complete_partial only). */
int rpo_cartsafe_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                            int obs_stride, float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid,
                            float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                            const float* consts_host, int partial, int form, void* stream);
int rpo_pendulum_policy_act(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                            int obs_stride, float* action, float* proposal, int* iters, float* eq_resid, float* ineq_resid,
                            float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps, float corr_momentum,
                            int form, void* stream);

/* Projection profiles (RPOTrainerBase.act(profile=True)): the same rows with every budget 0..K of the projection written down
 * in ONE launch, K = max_steps >= 0.  profile [K + 1, n, 4] (16-byte aligned; RPO_ERR_ARG when NULL or misaligned): plane b,
 * row i = (a0, a1, eq_resid, max_j ineq_resid_j) of the row's iterate after min(b, iters[i]) GRG steps, signed residuals with
 * the bits of rpo_<env>_resid, one non-temporal 16-byte store per row and plane.  Every plane of every row is written (a row
 * whose stop test has fired repeats its final iterate): the buffer needs no zeroing.  The other outputs are those of the call
 * without the profile, for the budget K.  Row-tile form only (16 rows per workgroup, 64 from 12 288 rows).
 * == for b = 0..K: rpo_<env>_policy_act(max_steps = b, form 1), plane b = (action, eq_resid, max_j ineq_resid), bit for bit. */
int rpo_cartsafe_policy_act_profile(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                                    int obs_stride, float* action, float* proposal, int* iters, float* eq_resid,
                                    float* ineq_resid, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                    float corr_momentum, const float* consts_host, int partial, float* profile, void* stream);
int rpo_pendulum_policy_act_profile(const rpo_mlp* actor_host, int gauss, float scale, float base, int n, const float* obs,
                                    int obs_stride, float* action, float* proposal, int* iters, float* eq_resid,
                                    float* ineq_resid, float box_lo, float box_hi, int max_steps, float corr_lr, float corr_eps,
                                    float corr_momentum, float* profile, void* stream);
/* The projection alone, behind the caller's proposal launches: rpo_<env>_act_project under RPO_NOISE_NONE (its arguments
 * without the noise, the box, the generator, ctrl and stats) with the profile of the budgets 0..K, K = max_steps >= 0; one
 * thread per row.  action [n, 2] (8-byte aligned), iters [n] (may be NULL), profile as above.
 * == for b = 0..K: rpo_<env>_act_project(RPO_NOISE_NONE, max_steps = b) + rpo_<env>_resid, plane b = (action, eq_resid,
 *    max_j ineq_resid), bit for bit. */
int rpo_cartsafe_project_profile(int n, const float* ap_raw, float* action, int* iters, int max_steps, float corr_lr,
                                 float corr_eps, float corr_momentum, const float* consts_host, int partial, float* profile,
                                 void* stream);
int rpo_pendulum_project_profile(int n, const float* obs, int obs_stride, const float* ap_raw, float* action, int* iters,
                                 int max_steps, float corr_lr, float corr_eps, float corr_momentum, float* profile,
                                 void* stream);

/* The stepwise form of the record (any env): row (step, i), i < trace_rows, of trace [trace_steps, trace_rows, W] from the
 * transition rows rpo_<env>_step wrote (reward, done and the violations, reduced as in rpo_eval_accumulate), the
 * observation obs [n, obs_stride] the policy read BEFORE that step (the caller keeps a copy: the step overwrites it), the
 * proposal [n, partial_dim], the stepped action [n, action_dim] and iters [n] (may be NULL: 0).  W follows from obs_dim,
 * partial_dim and action_dim (RPO_TRACE_*).  Liveness is read from acc [n, RPO_EVAL_LEN], so the call goes BEFORE
 * rpo_eval_accumulate of the same step; at step 0 every lane is live.  trace: zeroed by the caller, 16-byte aligned. */
int rpo_eval_record(int n, const float* rows, int row_stride, int reward_col, int done_col, int eq_col, int eq_num,
                    int ineq_col, int ineq_num, const float* obs, int obs_stride, int obs_dim, const float* proposal,
                    int partial_dim, const float* action, int action_dim, const int* iters, int step, const float* acc,
                    float* trace, int trace_rows, int trace_steps, void* stream);

/* The stepwise form of the per-constraint report (any env): step `step` of n episodes from the transition rows
 * rpo_<env>_step wrote into con [n, W] (layout RPO_CON_*, W from ineq_num and eq_num).  One thread per (episode, cell) -- a
 * wave reads neighbouring columns of a row and stores neighbouring cells; every cell has one owner, nothing is reduced across
 * threads.  Liveness is read from acc [n, RPO_EVAL_LEN], so the call goes BEFORE rpo_eval_accumulate of the same step; at step
 * 0 every lane is live and every cell is written. */
int rpo_eval_constraints(int n, const float* rows, int row_stride, int eq_col, int eq_num, int ineq_col, int ineq_num, int step,
                         float viol_thresh, const float* acc, float* con, void* stream);

/* The stepwise form of the same statistics (any env): step `step` of n episodes from the transition rows rpo_<env>_step
 * wrote (rows [n, row_stride], the column layout of the env's replay rows: reward, done, eq_viol [eq_num], ineq_viol
 * [ineq_num] at the given columns) and the projection's iteration counts iters [n] (may be NULL: 0) into acc
 * [n, RPO_EVAL_LEN]; step == 0 writes the rows from scratch. */
int rpo_eval_accumulate(int n, const float* rows, int row_stride, int reward_col, int done_col, int eq_col, int eq_num,
                        int ineq_col, int ineq_num, const int* iters, int step, float viol_thresh, float* acc, void* stream);

/* The accumulator rows acc [n, RPO_EVAL_LEN] of one finished evaluation -> one curve row row_out [RPO_CURVE_LEN] (doubles,
 * layout RPO_CURVE_*); ctrl: the TRAINING env's control words, ctrl[RPO_CTRL_T] becomes RPO_CURVE_STEP (read on the device);
 * ws [RPO_CURVE_WS] doubles of scratch (owned by the caller, one evaluation at a time).  1 <= n <= RPO_CURVE_MAX_EPISODES.
 * No floating-point atomics: a workgroup sums its own contiguous chunk of rows (wave64 butterfly, then the four waves in
 * order) into its own slot of ws, and the slots are combined in slot order -- the summation order depends on n alone, so the
 * row is the same bits from run to run and for any placement of the workgroups.  Standard deviations come from the
 * deviations about the mean (a second pass over the rows).  n <= 1024: one workgroup, one launch; otherwise three launches
 * (chunk sums | chunk sums of squared deviations | combine). */
int rpo_eval_summarize(int n, const float* acc, const long long* ctrl, double* row_out, double* ws, void* stream);

/* Keep the best policy of a curve-mode run (trainer argument keep_best): the curve row `row` [RPO_CURVE_LEN] that
 * rpo_eval_summarize has just written for evaluation point `point` (>= 0) is compared ON THE DEVICE with the incumbent's row
 * best_row [RPO_CURVE_LEN]; best_point[0] is the point held, -1 for none.  With rate = row[VIOL_STEPS] / row[LENGTH] (+inf when
 * LENGTH == 0) and ret = row[RPO_CURVE_STATS]: a candidate with row[NONFINITE] > 0 or a NaN ret is never taken; a point is safe
 * when rate <= max_violation_rate (>= 0, RPO_ERR_ARG otherwise); a candidate wins when there is no incumbent, when it is safe
 * and the incumbent is not, when both are safe and its ret is strictly higher, or when both are unsafe and its rate is
 * strictly lower or equal with a strictly higher ret (rpo_eval_dev::keep_best_wins).  Ties keep the earlier point.
 * Two launches on `stream`, kernels only, nothing read on the host: one wave decides and, if the candidate wins, writes
 * best_row = row and best_point[0] = point; then every thread of the copy reads best_point[0] and, where it equals `point`,
 * copies its share of src [n_params] (the actor's span of the flat parameter buffer, or its snapshot) into best [n_params] --
 * 16-byte accesses where src and best sit at the same offset from a 16-byte boundary (scalar head and tail), scalar accesses
 * otherwise; neither needs more than float alignment (RPO_ERR_ARG below that).  A losing candidate leaves best untouched. */
int rpo_eval_keep_best(long long n_params, const float* src, float* best, const double* row, double* best_row,
                       long long* best_point, long long point, double max_violation_rate, void* stream);

/* Forward half of the critic update (rpo_ddpg.py:165-174, 327-337): ReplayBuffer.sample (Philox draw, or idx_in when
 * given) -> batch_out [B,24]; pi_targ(s') -> Complete + Proj -> Q_targ(s', a') = qn_out; Q(s, a) = q_out with the
 * critic's pre-activations saved (x0_save [B,E], h1_save [B,H]) for rpo_mlp_backward.  Two workgroups per 16-row tile
 * (gridDim.y: target chain | critic) that never talk to each other; the TD target / Huber loss is the prologue of
 * rpo_mlp_backward (rpo_td), where their results meet.
 * == rpo_replay_sample_gather + 3 x rpo_mlp_forward + rpo_cartsafe_act_project. */
int rpo_cartsafe_ddpg_critic_forward(const rpo_mlp* actor_target_host, const rpo_mlp* critic_target_host,
                                     const rpo_mlp* critic_host, float scale, float base, const float* rows,
                                     long long cap_steps, int n_envs, int batch, float* batch_out, long long* idx_out,
                                     const long long* idx_in, unsigned long long seed, unsigned sample_salt,
                                     const long long* ctrl, int max_steps, float corr_lr, float corr_eps,
                                     float corr_momentum, float box_lo, float box_hi, const float* consts_host,
                                     int partial, float* q_out, float* qn_out, float* x0_save, float* h1_save,
                                     void* stream);

/* The policy step of RPODDPG (rpo_ddpg.py:186-205, 307-324) as forward + backward pipelines, env = 0 CartSafe-v0 /
 * 1 SpringPendulum-v0 (E = 128; the actor loss completes the action but does not project it):
 *   forward:  pi(s) with pre-activations saved -> ap = clip(ap_det + eps_t * N(0,1)) (noise_in[b], or the Philox draw of
 *             rpo_philox_normal(noise_id_base, noise_salt, RPO_STREAM_POLICY)) -> Complete -> Q(s, a) saved ->
 *             Lagrangian term: g_act [B,2] = d/d action / B, partial_out [ceil(B/16), 8] = per-workgroup sums of
 *             (nu . relu(g), relu(g_0..5), Q); dq_out = -1/B.
 *   backward: critic rows with da, da += g_act, autograd through Complete and the tanh box / clip, actor rows, the
 *             actor's weights pass (with a shared state embedding the critic's dx0 is added to the actor's first, so one
 *             first-layer reduction yields the embedding's gradient); lag_out = (mean Lagrangian term, mean Q),
 *             nu_grad [6] += mean relu(g); gradmax as in rpo_mlp_backward (actor slice).
 * == rpo_mlp_forward x 2, rpo_philox_normal, rpo_cartsafe_act_project, rpo_cartsafe_lagrangian, rpo_mlp_backward x 2,
 *    rpo_cartsafe_complete_bwd, rpo_tanh_box_bwd and three elementwise launches. */
int rpo_ddpg_actor_forward(int env, const rpo_mlp* actor_host, const rpo_mlp* critic_host, float scale, float base,
                                    float box_lo, float box_hi, float eps_start, float eps_end, float eps_decay,
                                    const float* batch, int batch_size, const float* noise_in, unsigned long long seed,
                                    unsigned noise_id_base, unsigned noise_salt, const long long* ctrl, const float* nu,
                                    const float* consts_host, int partial, float* ap_det, float* noise_out,
                                    float* actions, float* q_out, float* dq_out, float* g_act, float* partial_out,
                                    float* actor_x0, float* actor_h1, float* critic_x0, float* critic_h1, void* stream);
int rpo_ddpg_actor_backward(int env, const rpo_mlp* actor_host, const rpo_mlp_grad* actor_grad_host,
                                     const rpo_mlp* critic_host, int shared_embedding, const float* batch,
                                     int batch_size, const float* actions, const float* g_act, const float* ap_det,
                                     const float* noise, const float* dq, float eps_start, float eps_end,
                                     float eps_decay, float box_lo, float box_hi, float scale, float base,
                                     const long long* ctrl, const float* consts_host, int partial,
                                     const float* actor_x0, const float* actor_h1, const float* critic_x0,
                                     const float* critic_h1, float* actor_dh, float* actor_dx0, float* critic_dh,
                                     float* critic_dx0, float* da, float* dout, const float* partial_in, float* lag_out,
                                     float* nu_grad, float* gradmax, void* stream);

/* The policy step of RPOSAC (rpo_sac.py:191-219, 321-339) as forward + backward pipelines, env = 0 CartSafe-v0 /
 * 1 SpringPendulum-v0 (E = 128; the actor loss completes the action but does not project it, so nothing couples rows):
 *   forward:  two independent workgroups per 16-row tile (gridDim.y = critic): pi(s) heads -> rsample (noise_in[b] or the
 *             Philox draw) + box clip, logp [B] -> Complete -> Q_k(s, a) saved, left in dq_k [B] (a Q value at this point);
 *             role 0 also writes raw [B,2], noise_out, logp, actions, the Lagrangian term's g_act and partial_out
 *             [ceil(B/16), 8] columns 0..6 = sums of (nu . relu(g), relu(g_0..5));
 *   backward: prologue per tile: dq_k <- d(-min(Q1, Q2))/dQ_k / B in place (ties split like torch.min's backward) and
 *             partial[tile][7] = sum(alpha log pi - min Q); then both critics' rows (da_k), da = da1 + da2 + g_act, Complete,
 *             Gaussian head with dlogp = alpha / B, actor rows, the actor's weights pass; lag_out[0] = mean Lagrangian
 *             term, nu_grad +=.  (mean(alpha log pi - min Q) = sum of partial[:, 7] / B, summed by whoever reads the loss.) */
int rpo_sac_actor_forward(int env, const rpo_mlp* actor_host, const rpo_mlp* critic1_host, const rpo_mlp* critic2_host,
                          float scale, float base, float box_lo, float box_hi, float alpha, const float* batch,
                          int batch_size, const float* noise_in, unsigned long long seed, unsigned noise_id_base,
                          unsigned noise_salt, const long long* ctrl, const float* nu, const float* consts_host,
                          int partial, float* raw, float* noise_out, float* logp, float* actions, float* dq1, float* dq2,
                          float* g_act, float* partial_out, float* actor_x0, float* actor_h1, float* critic1_x0,
                          float* critic1_h1, float* critic2_x0, float* critic2_h1, void* stream);
int rpo_sac_actor_backward(int env, const rpo_mlp* actor_host, const rpo_mlp_grad* actor_grad_host,
                           const rpo_mlp* critic1_host, const rpo_mlp* critic2_host, int shared_embedding,
                           const float* batch, int batch_size, const float* actions, const float* g_act, const float* raw,
                           const float* noise, const float* logp, float* dq1, float* dq2, float dlogp, float box_lo,
                           float box_hi, float scale, float base, const float* consts_host, int partial,
                           const float* actor_x0, const float* actor_h1, const float* critic1_x0, const float* critic1_h1,
                           const float* critic2_x0, const float* critic2_h1, float* actor_dh, float* actor_dx0,
                           float* critic1_dh, float* critic1_dx0, float* critic2_dh, float* critic2_dx0, float* da1,
                           float* da2, float* dout, float* partial_in, float* lag_out, float* nu_grad,
                           float* gradmax, void* stream);

/* The same for RPOSAC.critic_loss (rpo_sac.py:342-353): sample -> a' ~ pi(s') with the ONLINE actor (mean / log-std
 * heads, rsample, box clip; the N(0,1) draw of row b is normal(philox(noise_seed, noise_id_base + b, ctrl[T] +
 * noise_salt, RPO_STREAM_POLICY, ctrl[UPDATES])), i.e. rpo_philox_normal, or eps_in[b] when given) -> Complete + Proj ->
 * qn_k = Qk_targ(s', a'), logp_out = log pi(a'|s'); q_k = Qk(s, a) with the pre-activations saved.  Four independent
 * workgroups per 16-row tile (gridDim.y: Q1_targ chain | Q2_targ chain | Q1 | Q2); the TD target
 * y = r + gamma (1 - done) (min(qn1, qn2) - alpha logp) and both Huber terms are the prologue of rpo_mlp_backward_pair
 * (rpo_td).
 * == rpo_replay_sample_gather + rpo_philox_normal + 5 x rpo_mlp_forward + rpo_gauss_head + rpo_cartsafe_act_project. */
int rpo_cartsafe_sac_critic_forward(const rpo_mlp* actor_host, const rpo_mlp* critic_target1_host,
                                    const rpo_mlp* critic_target2_host, const rpo_mlp* critic1_host,
                                    const rpo_mlp* critic2_host, float scale, float base, const float* rows,
                                    long long cap_steps, int n_envs, int batch, float* batch_out, long long* idx_out,
                                    const long long* idx_in, const float* eps_in, unsigned long long sample_seed,
                                    unsigned sample_salt, unsigned long long noise_seed, unsigned noise_id_base,
                                    unsigned noise_salt, const long long* ctrl, int max_steps, float corr_lr,
                                    float corr_eps, float corr_momentum, float box_lo, float box_hi,
                                    const float* consts_host, int partial, float* q1_out, float* q2_out,
                                    float* qn1_out, float* qn2_out, float* logp_out, float* x0_save1, float* h1_save1,
                                    float* x0_save2, float* h1_save2, void* stream);

/* SpringPendulum-v0: the reference's batched projection couples the samples of a batch (pendulum.py:337-339), so the
 * RPOSAC critic-forward chain is cut there into two launches around rpo_pendulum_project_batchref:
 *   front: sample -> batch_out [B,16] -> a' ~ pi(s') -> ap_out [B] (clipped basic action), logp_out [B];
 *   back:  four independent workgroups per tile: qn_k = Qk_targ(s', next_actions [B,2]) | q_k = Qk(s, a) of batch_rows
 *          (pre-activations saved); TD / Huber: rpo_td prologue of rpo_mlp_backward_pair. */
int rpo_pendulum_sac_critic_front(const rpo_mlp* actor_host, float scale, float base, float box_lo, float box_hi,
                                  const float* rows, long long cap_steps, int n_envs, int batch, float* batch_out,
                                  long long* idx_out, const long long* idx_in, const float* eps_in,
                                  unsigned long long sample_seed, unsigned sample_salt, unsigned long long noise_seed,
                                  unsigned noise_id_base, unsigned noise_salt, const long long* ctrl, float* ap_out,
                                  float* logp_out, void* stream);
int rpo_pendulum_sac_critic_back(const rpo_mlp* critic_target1_host, const rpo_mlp* critic_target2_host,
                                 const rpo_mlp* critic1_host, const rpo_mlp* critic2_host, int batch, float* batch_rows,
                                 const float* next_actions, float* q1_out, float* q2_out, float* qn1_out, float* qn2_out,
                                 float* x0_save1, float* h1_save1, float* x0_save2, float* h1_save2, void* stream);

/* The RPODDPG form of the cut pipeline for SpringPendulum-v0 (rpo_ddpg.py:327-337):
 *   front: sample -> batch_out [B,16] -> ap_out [B] = pi_targ(s') (tanh box);
 *   back:  two independent workgroups per tile: qn = Q_targ(s', next_actions) | q = Q(s, a) of batch_rows
 *          (pre-activations saved); TD / Huber: rpo_td prologue of rpo_mlp_backward. */
int rpo_pendulum_ddpg_critic_front(const rpo_mlp* actor_target_host, float scale, float base, const float* rows,
                                   long long cap_steps, int n_envs, int batch, float* batch_out, long long* idx_out,
                                   const long long* idx_in, unsigned long long sample_seed, unsigned sample_salt,
                                   const long long* ctrl, float* ap_out, void* stream);
int rpo_pendulum_ddpg_critic_back(const rpo_mlp* critic_target_host, const rpo_mlp* critic_host, int batch,
                                  float* batch_rows, const float* next_actions, float* q_out, float* qn_out,
                                  float* x0_save, float* h1_save, void* stream);

/* Policy heads around the MLP kernels.
 * DDPG (model/policy.py:30-31, agent/ddpg_pa.py:108-110): ap = clip(ap_det + eps_t * noise), ap_det = scale*tanh(o)+base.
 *   dout[i] = dap[i] * 1[lo <= ap_det + eps_t*noise <= hi] * scale * (1 - tanh(o)^2); noise NULL: no noise, no clip. */
int rpo_tanh_box_bwd(int n, const float* dap, const float* ap_det, const float* noise, float eps_start, float eps_end,
                     float eps_decay, const long long* ctrl, float lo, float hi, float scale, float base, float* dout,
                     void* stream);

/* SAC (GaussianSharedPolicy.forward, model/policy.py:53-66; PDSAC_PA.take_action, agent/sac_pa.py:105-115):
 * raw [n,2] = (mean, log-std head) from rpo_mlp_forward, eps [n] the N(0,1) draw of rsample.
 *   log_std = clamp(raw1 - 3, -23, -2); x = mean + eps * exp(log_std); y = tanh(x);
 *   ap = clip(scale*y + base)  (deterministic: clip(scale*tanh(mean)+base));
 *   log_prob = -eps^2/2 - log_std - log(sqrt(2 pi)) - log(scale*(1 - y^2) + 1e-6). */
int rpo_gauss_head(int n, const float* raw, const float* eps, float scale, float base, float lo, float hi,
                   int deterministic, float* ap_out, float* logp_out, void* stream);

/* Backward of the above: draw [n,2] given dap [n] and a uniform d/d(log_prob) = dlogp (alpha / B in rpo_sac.py:331). */
int rpo_gauss_head_bwd(int n, const float* raw, const float* eps, const float* dap, float dlogp, float scale,
                       float base, float lo, float hi, float* draw, void* stream);

/* Behaviour-cloning head (trainer.pretrain, rpo_amd/algo/pretrain.py; csrc/bc.hip): the loss of the actor's tanh-box output
 * against a demonstrated basic action, in box-normalised coordinates, and its gradient w.r.t. the RAW actor output.
 * raw [n, heads * P] from rpo_mlp_forward without a box (heads = 1: RPODDPG; heads = 2: RPOSAC's (mean | log-std), the mean half is
 * read), target [n, P] with rows target_stride >= P floats apart (columns of a gathered batch), P <= 16.  Per row i, component j:
 *   scale = (hi - lo) / 2, base = lo + scale;  u = clamp((target - base) / scale, -clip, clip), 0 < clip <= 1;  y = tanh(raw)
 *   L = 1 / (n P) sum_ij w_j (y - u)^2;        draw_ij = 2 w_j / (n P) (y - u) (1 - y^2)
 * A term with scale <= 1e-6 (an empty box) contributes 0 to both; the denominator stays n P.  draw [n, heads * P] is written in
 * full: for heads = 2 the log-std half receives exactly 0.  loss_parts [(n + 15) / 16]: loss_parts[g] is the share of rows
 * [16 g, 16 g + 16) in L, summing them in index order gives L.  The bits of draw and loss_parts depend on neither the grid size
 * nor any arrival order (one writer per word, fixed summation order, no atomics).  NaN: as in the heads above, a NaN in raw
 * reaches draw and the loss (in a term of an empty box it is dropped with the term); the clamp of u keeps a NaN target.
 * lo_host / hi_host / weights_host: HOST pointers to P floats, copied into the launch's arguments (weights_host NULL: all 1;
 * a negative or NaN weight is RPO_ERR_ARG). */
int rpo_bc_head(int n, int P, int heads, const float* raw, const float* target, int target_stride, const float* lo_host,
                const float* hi_host, const float* weights_host, float clip, float* draw, float* loss_parts, void* stream);

/* The same for EVOPF-v0 (P = RPO_EVOPF_PARTIAL): the box of (i, j) is the state-dependent one of row i's observation
 * (state [n, >= RPO_EVOPF_STATE] with rows state_stride floats apart; EVOPFEnv.update, what rpo_evopf_tanh_box_bwd and the
 * projection use), so a battery whose state of charge is out of band has an empty box and its term is 0. */
int rpo_evopf_bc_head(int n, int heads, const float* state, int state_stride, const float* raw, const float* target,
                      int target_stride, const float* weights_host, float clip, float* draw, float* loss_parts,
                      const float* consts_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RPO_HIP_H */
