/*
 * hpc_rll_hip.h -- C ABI of libhpc_rll_hip.so, the MI355X (gfx950) operator library behind the
 * hpc_rll.rl_utils / hpc_rll.torch_utils Python API.
 *
 * This is the drop-in boundary: plain pointers + sizes + a HIP stream, no torch types, no
 * allocation, no host synchronisation, never throws.  Every entry point returns 0 on success,
 * a positive hipError_t value if the HIP runtime reported one, or a negative HPC_RLL_E* code for
 * an invalid argument.  All tensors are dense row-major ("contiguous") device buffers; floats are
 * fp32, indices int64 (torch.long), exactly as the reference's kernels assume.
 *
 * Each declaration cites the reference interface (file:line under /root/reference) it replaces:
 * the pybind entry `Fn(std::vector<Tensor> inputs, std::vector<Tensor>& outputs, scalars...)`
 * declared in include/hpc/rll/cuda/rl_utils/entry.h and .../torch_utils/network/entry.h.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 * "scale" arguments let a data-parallel caller pass 1/(GLOBAL element count) so that per-rank
 * partial losses sum (one RCCL all-reduce) to the single-GPU result.
 */
#ifndef HPC_RLL_HIP_H_
#define HPC_RLL_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPC_RLL_OK 0
#define HPC_RLL_EINVAL (-1)     /* bad size / null pointer                      */
#define HPC_RLL_EALIGN (-2)     /* pointer not 4-byte aligned                   */
#define HPC_RLL_EUNSUPPORTED (-3) /* shape outside what the kernels implement   */
#define HPC_RLL_ETIMEOUT (-4)   /* a persistent LSTM kernel gave up waiting for its co-resident workgroups */

/* ABI version, bumped on any signature change or added entry point (3 = round 3: kernel timing, packed / grouped pad). */
int hpc_rll_abi_version(void);
/* Human readable message for a status returned by any entry point (static storage). */
const char* hpc_rll_status_string(int status);
/* Stream helpers for host bindings that must not call the HIP runtime themselves (the torch extension is host-only
 * C++): is_capturing returns 1 while `stream` records into a hipGraph, 0 if not, a negative code on error;
 * synchronize blocks the host until the stream has drained (positive hipError_t on failure). */
int hpc_rll_stream_is_capturing(void* stream);
int hpc_rll_stream_synchronize(void* stream);

/* ------------------------------------------------------------------------------------------
 * GAE  -- replaces GaeForward (include/hpc/rll/cuda/rl_utils/entry.h:62-66, src/rl_utils/gae.cu:8-28,
 *         kernel gae_kernel.h:10-29).  The reference has no backward (hpc_rll/rl_utils/gae.py:17-18);
 *         hpc_rll_gae_backward is the analytic adjoint of hpc_rll.origin.gae.
 *
 *   value (T+1,B), reward (T,B) -> adv (T,B)
 *   grad_adv (T,B) -> grad_value (T+1,B) [may be NULL], grad_reward (T,B) [may be NULL]
 *
 * `coef` is a T-float device table c_t = gamma*lambda*D_{t+1}/D_t (D_t = 1 + lambda*D_{t+1},
 * D_T = 0) that depends only on (T, gamma, lambda); fill it once with hpc_rll_gae_coef and reuse
 * it for every call with the same (T, gamma, lambda).
 * ------------------------------------------------------------------------------------------ */
int hpc_rll_gae_coef(float* coef, int T, float gamma, float lambda, void* stream);
int hpc_rll_gae_forward(const float* value, const float* reward, float* adv, const float* coef,
                        int T, int B, float gamma, void* stream);
int hpc_rll_gae_backward(const float* grad_adv, float* grad_value, float* grad_reward, const float* coef,
                         int T, int B, float gamma, void* stream);
/* Expert entry points: pin the launch configuration instead of the built-in heuristic.
 * vec in {1,2,4} columns per lane, lc in {2,4,8,16} time steps per wave chunk, nw in {1,2,4,8,16}
 * waves per workgroup; 0 for any of them = choose automatically.  flags: bit0 nontemporal loads,
 * bit1 nontemporal stores; -1 = choose automatically.  HPC_RLL_EUNSUPPORTED if the combination is
 * not instantiated. */
int hpc_rll_gae_forward_ex(const float* value, const float* reward, float* adv, const float* coef,
                           int T, int B, float gamma, int vec, int lc, int nw, int flags, void* stream);
int hpc_rll_gae_backward_ex(const float* grad_adv, float* grad_value, float* grad_reward, const float* coef,
                            int T, int B, float gamma, int vec, int lc, int nw, int flags, void* stream);
/* Flags bit 2 (value 4): half-wave tiles (32 columns, two time chunks per wave; narrow batches).  Bit 3 (value 8): the
 * software-pipelined kernel (the next chunk's row loads are issued before the current chunk's barrier / stores);
 * bit-identical results.  It needs explicit vec, lc and nw from its instantiated set -- forward (vec,lc) in (1,8) (1,16)
 * (2,4) (2,8) (2,16) (4,4) (4,8), backward (1,8) (2,2) (2,4) (2,8) (4,2) (4,4) (4,8), nw in {2,4,8} -- and stores
 * nontemporally whatever bit 1 says; any other request with bit 3 is HPC_RLL_EUNSUPPORTED and launches nothing.  A
 * backward with a NULL gradient runs the plain kernel of the same triple with bits 0-1 as given, and
 * hpc_rll_gae_last_config says so.  Bits 4 and 5 (the one-trajectory-per-wavefront mapping and XCD-contiguous column
 * tiles of rounds 3-4) left the library in round 5 (tests/tools/micro/gae_wpt.hip keeps the former):
 * HPC_RLL_EUNSUPPORTED.
 *
 * Diagnostics (no reference counterpart; the reference times whole python calls, tests/test_gae.py:31-52).
 * hpc_rll_ktime_begin(capacity) arms per-launch KERNEL timing for the next `capacity` GAE launches of this process
 * (start/stop events attached to the dispatch itself: the kernel's own begin/end, what rocprofv3 --kernel-trace
 * reports); hpc_rll_ktime_end waits for them, writes durations in milliseconds and kinds (0 forward, 1 backward) in
 * launch order, disarms and returns the number recorded.  Not thread-safe, not usable under stream capture.
 * hpc_rll_gae_last_config(dir, out[6]): the configuration the latest forward (dir 0) / backward (dir 1) launch used:
 * {columns per lane, steps per chunk, waves per workgroup, nontemporal flags, half-wave tiles, pipelined}. */
int hpc_rll_ktime_begin(int capacity);
int hpc_rll_ktime_end(float* ms, int* kind, int max);
int hpc_rll_gae_last_config(int dir, int* out);

/* ------------------------------------------------------------------------------------------
 * Episode-aware GAE with done / truncation masks (no reference counterpart; DI-engine's `gae` with `done` and
 * `traj_flag`).  Textbook GAE, not the normalised variant above.  f = traj_flag, defaulting to done; for t = T-1 .. 0:
 *     delta_t = reward_t + gamma*(1 - done_t)*nv_t - value_t,   adv_t = delta_t + gamma*lambda*(1 - f_t)*adv_{t+1}
 * with nv_t = next_value[t] (next-value form: value, next_value (T,B)) or value[t+1] (stacked form: next_value = NULL,
 * value (T+1,B)).  done and traj_flag are (T,B) masks of `mask_dtype`, either may be NULL (no episode ends / f = done):
 *     HPC_RLL_MASK_U8  bool or uint8, one byte per sample, any nonzero byte counts as 1
 *     HPC_RLL_MASK_F32 float32, (1 - m) used as written (soft masks)
 * Backward (analytic adjoint; `stacked` = 1 for the stacked form): d_t = g_t + gamma*lambda*(1 - f_{t-1})*d_{t-1},
 * grad_reward = d; next-value form: grad_value_t = -d_t, grad_next_value_t = gamma*(1 - done_t)*d_t; stacked form
 * (grad_value (T+1,B), grad_next_value must be NULL): grad_value_t = -d_t [t<T] + gamma*(1 - done_{t-1})*d_{t-1} [t>=1].
 * Any gradient output may be NULL.  Launch configuration: built-in heuristic only; no atomics, bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
#define HPC_RLL_MASK_U8 (0)   /* bool or uint8 masks */
#define HPC_RLL_MASK_F32 (1)  /* float32 masks */
int hpc_rll_gae_masked_forward(const float* value, const float* next_value, const float* reward,
                               const void* done, const void* traj_flag, int mask_dtype,
                               float* adv, int T, int B, float gamma, float lambda, void* stream);
int hpc_rll_gae_masked_backward(const float* grad_adv, const void* done, const void* traj_flag, int mask_dtype,
                                float* grad_value, float* grad_next_value, float* grad_reward, int stacked,
                                int T, int B, float gamma, float lambda, void* stream);

/* ------------------------------------------------------------------------------------------
 * Shared helpers of the scalar-loss ops.
 *   hpc_rll_partials_floats(n): floats of scratch ("partials") an op over n columns/samples needs.
 *   hpc_rll_scale_rows: out[i] = g[0]*in[i] (i < n_in), 0 (n_in <= i < n_out) -- the generic
 *     "upstream scalar x saved unit gradient" backward step.
 * Every *_forward writes per-rank SUMS times `scale`; pass scale = 1/(global count) so that a
 * data-parallel caller gets the global mean with one all-reduce(sum) of the loss scalars.
 * ------------------------------------------------------------------------------------------ */
int64_t hpc_rll_partials_floats(int64_t n);
int hpc_rll_scale_rows(const float* g, const float* in, float* out, int64_t n_in, int64_t n_out, void* stream);

/* Diagnostic of the column-scan family (no reference counterpart; read-only, modelled on hpc_rll_gae_last_config):
 * which kernel the most recent launch of this process ran for `op`, recorded on the host where the template is chosen,
 * so it names the instantiation that was launched rather than re-evaluating the selection rule.
 * out[HPC_RLL_SCAN_CONFIG_INTS] = {
 *    [0] launches of this op so far (0 = no launch yet: every other entry is then -1),
 *    [1] columns per lane, [2] steps per wave chunk, [3] waves per workgroup,
 *    [4] sub-wave groups per wave (1, 2, 4 or 8; the half-wave tiles of the episode-aware GAE are 2),
 *    [5] nontemporal loads (0 / 1),
 *    [6] mask element type of the instantiation (HPC_RLL_MASK_U8 / HPC_RLL_MASK_F32; U8 when there is no mask),
 *    [7] mask mode: 0 no masks, 1 done only (traj_flag = done), 2 done and traj_flag, 3 traj_flag only,
 *    [8] 1 = next-value form, 0 = stacked form,
 *    [9] workgroups of the launch,
 *    [10] how the loss sums were finalised: 0 the op has none, 1 folded into the launch (grids up to 512 workgroups),
 *         2 by the separate finalize launch }.
 * Calls that return before launching (empty shapes, argument errors) leave the record as it was.  Plain ints of the
 * host process, not synchronised.  HPC_RLL_EINVAL for an op outside the list or out == NULL. */
#define HPC_RLL_SCAN_OP_TD_LAMBDA (0)         /* hpc_rll_td_lambda_forward */
#define HPC_RLL_SCAN_OP_VTRACE (1)            /* hpc_rll_vtrace_forward */
#define HPC_RLL_SCAN_OP_UPGO (2)              /* hpc_rll_upgo_forward */
#define HPC_RLL_SCAN_OP_TD_LAMBDA_MASKED (3)  /* hpc_rll_td_lambda_masked_forward */
#define HPC_RLL_SCAN_OP_VTRACE_MASKED (4)     /* hpc_rll_vtrace_masked_forward */
#define HPC_RLL_SCAN_OP_GAE_MASKED_FWD (5)    /* hpc_rll_gae_masked_forward */
#define HPC_RLL_SCAN_OP_GAE_MASKED_BWD (6)    /* hpc_rll_gae_masked_backward */
#define HPC_RLL_SCAN_OPS (7)
#define HPC_RLL_SCAN_CONFIG_INTS (11)
int hpc_rll_scan_last_config(int op, int* out);

/* Categorical head over `rows` rows of N logits (rows = T*B or B), action int64 per row.
 * Replaces categoricalTarget/categoricalBehaviour (vtrace_kernel.h:11-151), crossEntropyKernel
 * (upgo_kernel.h:40-81), categoricalProbEntropy/categoricalProb (ppo_kernel.h:12-150) and the
 * backward kernels that consume their saved buffers.  forward: logp[row] = log softmax(logits)[a],
 * entropy[row] (nullable).  backward: grad[row,i] = g_logp*coef_logp[row]*(1[i==a]-p_i)
 *   + g_ent*coef_ent[row]*(-p_i*(log p_i + H));  g_* are device scalars (NULL = 1), coef_ent may
 *   be NULL (no entropy term). */
int hpc_rll_categorical_forward(const float* logits, const int64_t* action, float* logp, float* entropy,
                                int64_t rows, int N, void* stream);
int hpc_rll_categorical_backward(const float* logits, const int64_t* action, const float* coef_logp,
                                 const float* g_logp, const float* coef_ent, const float* g_ent,
                                 float* grad_logits, int64_t rows, int N, void* stream);
/* Diagnostic (no reference counterpart; read-only, modelled on hpc_rll_gae_last_config / hpc_rll_acer_last_config): which
 * categorical kernel the most recent launch of this process ran, recorded on the host where the kernel is launched.
 * direction HPC_RLL_CAT_DIR_FORWARD covers hpc_rll_categorical_forward and every op that runs the head's forward (V-trace,
 * UPGO, PPO -- its one-launch fused forward included); HPC_RLL_CAT_DIR_BACKWARD covers hpc_rll_categorical_backward and
 * those ops' backward.  out[HPC_RLL_CATEGORICAL_CONFIG_INTS] = {
 *    [0] launches in this direction so far (0 = no launch yet: every other entry is then -1),
 *    [1] kernel family, one of HPC_RLL_CAT_FAMILY_*,
 *    [2] G, [3] VEC, [4] E: lanes per row, floats per load, loads per lane and row (ROW and PPO_FUSED; BLOCKROW reports its
 *        E = float4 loads per thread, 4 / 8 / 16, with G = VEC = 0; the other families report 0, 0, 0),
 *    [5] R: rows per lane group and iteration (ROW: 4 / 2 / 1, PPO_FUSED: 4); for the families without lane groups the rows
 *        per WORKGROUP and iteration (SMALL 256, BLOCKROW 1, LDSROW 1, LONG 4),
 *    [6] 1 = the entropy half runs (forward: entropy != NULL; backward: coef_ent != NULL; PPO_FUSED: always), 0 = it does not,
 *    [7] workgroups of the launch }.
 * Calls that return before launching (rows == 0, argument errors) leave the record as it was.  Plain ints of the host
 * process, not synchronised.  HPC_RLL_EINVAL for a direction outside the two or out == NULL. */
#define HPC_RLL_CAT_DIR_FORWARD (0)
#define HPC_RLL_CAT_DIR_BACKWARD (1)
#define HPC_RLL_CAT_FAMILY_ROW (0)        /* a row per group of G lanes, in registers: the 20 (G, VEC, E) configurations */
#define HPC_RLL_CAT_FAMILY_SMALL (1)      /* N % 4 != 0, N <= 32, 16-byte aligned bases: 256 rows per workgroup through LDS */
#define HPC_RLL_CAT_FAMILY_BLOCKROW (2)   /* 2048 < N <= 16384, 16-byte loads: a row per workgroup, in registers */
#define HPC_RLL_CAT_FAMILY_LDSROW (3)     /* 512 < N <= 16384 with 4-byte loads: a row per workgroup, in LDS */
#define HPC_RLL_CAT_FAMILY_LONG (4)       /* N > 16384: a row per wave, three passes */
#define HPC_RLL_CAT_FAMILY_PPO_FUSED (5)  /* PPO's forward in one launch (both heads and the sample arithmetic) */
#define HPC_RLL_CATEGORICAL_CONFIG_INTS (8)
int hpc_rll_categorical_last_config(int direction, int* out);

/* Path switches (a test / measurement hook, not a serving API; csrc/tune.hip holds the table): process-global plain ints,
 * not synchronised -- set them while no other thread is launching work, and never between an LSTM forward and its backward.
 * Every key selects between paths that BOTH ship (each wins on some shapes under the default rule), so that tests can run one
 * against the other on the same inputs; key 3 is also the deployment switch for GPUs shared between processes.  The launch
 * parameters and the measured-and-rejected variants that rounds 1-4 exposed as keys 0-2, 4-7, 9-15, 19, 20, 23, 30, 34, 36, 39
 * are constants / gone (HISTORY.md has what each measured); those keys answer HPC_RLL_EINVAL.
 *   key  3  persistent (co-residency dependent) LSTM kernels: 1 (default) / 0 = step kernels only
 *   key  8  B <= 4, L >= 2: 1 (default) = all layers in one launch as a wavefront / 0 = one persistent kernel per layer
 *   key 16  256x256x16 GEMM tiles (16 waves) for interior products that fill the chip in whole rounds: 1 (default) / 0
 *   key 17  ScatterConnection forward: 1 (default) = LDS-staged streaming kernel where it applies / 0 = cells-per-thread kernel
 *   key 18  channels per workgroup of that kernel (a multiple of 4 up to 64; 0, default = by LDS budget)
 *   key 21  loss finalisation folded into the last workgroup of the launch (grids up to 512): 1 (default) / 0 = finalize launch
 *   key 22  group split of the padding ops: 0 (default) = runs of equal keys / 1 = the element-level DP
 *   key 24  samples per wave of the large-batch C51 / QR-DQN forwards: 0 (default) by batch size, 1 off, 8 / 16 / 32 / 64.  Those
 *           four are the widths with kernels: hpc_rll_tune_set answers HPC_RLL_EINVAL for any other value, and the forwards
 *           return HPC_RLL_EUNSUPPORTED, before anything is enqueued, for a width without a kernel that their rule leaves above 1
 *   key 25  LDS-DMA staged GEMM tiles: 1 (default) all forms / 2 the 256x256 NT tile only / 0 register staging
 *   key 26  large-batch LSTM (B >= 4096, B % 256 == 0, 768 <= H <= 1024, H % 64 == 0) row-block kernels, a bit mask: bit 0 the
 *           persistent forward, bit 3 the persistent backward (H % 128 == 0), bit 7 fence-free forward exchanges; default 9;
 *           0 = one product + one cell launch per step on the same layout (forward / backward paths mix freely)
 *   key 27  start skew of those kernels' row blocks in microseconds (0 ... 200, default 10)
 *   key 28  packed Pad1D (32 <= max_len <= 16384): 1 (default) = wave tiles in output space / 0 = the workgroup kernel
 *   key 29  mid-batch persistent LSTM forward (5 <= B <= 256, 64 <= H <= 1024, H % 16 == 0): 0 off / 1 one stream / 2 (default)
 *           two batch streams where two copies of a Wh slice fit a CU's LDS
 *   key 31  one-hot gradients of at least this many MiB are written as fill + values (default 3072; 0 = never)
 *   key 32  PPO forward in one launch: 1 (default) / 0 = three launches
 *   key 33  mid-batch persistent LSTM backward: 0 off / 1 (default) where it pays (B <= 32) / 2 every mid-batch shape
 *   key 35  16-byte quads per workgroup of the one-launch one-hot kernel (256 ... 8192; 0, default = by size)
 *   key 37  scatter owner table / chain links built inside the forward kernel: 1 (default) / 0 = index launch
 *   key 38  scatter backward in XCD-major workgroup order: 1 (default) where its pieces are below a 64-byte sector pair / 2 always / 0
 *   key 40  scatter backward by spatial tiles (a workgroup stages map rows of ALL channels and writes whole entity rows): 0 (default) by
 *           rule (16-byte pieces in the plane kernel and M * 16 >= H * W) / 1 never / 2 wherever it applies; identical results
 * hpc_rll_tune_count / hpc_rll_tune_doc enumerate the live keys (index 0 ... count-1 -> key number and a one-line description). */
int hpc_rll_tune_set(int key, int value);
int hpc_rll_tune_count(void);
const char* hpc_rll_tune_doc(int index, int* key);

/* TD(lambda) -- replaces TdLambdaForward/Backward (rl_utils/entry.h:68-77, src/rl_utils/td_lambda.cu:8-52).
 * value (T+1,B), reward (T,B), weight: mode 0 none, 1 (B,), 2 (T,B).  loss (1,) =
 * 0.5*scale*sum w (ret-V)^2; grad_buf (T,B) = d loss / d value[:T]; partials >= partials_floats(B).
 * backward: grad_value (T+1,B) = grad_loss[0] * grad_buf, last row 0. */
int hpc_rll_td_lambda_forward(const float* value, const float* reward, const float* weight, int weight_mode,
                              float* loss, float* grad_buf, float* partials, int T, int B, float gamma,
                              float lambda, float scale, void* stream);
int hpc_rll_td_lambda_backward(const float* grad_loss, const float* grad_buf, float* grad_value, int T, int B,
                               void* stream);

/* V-trace -- replaces VTraceForward/Backward (rl_utils/entry.h:131-146, src/rl_utils/vtrace.cu:8-130).
 * target/behaviour_output (T,B,N), action (T,B) int64, value (T+1,B), reward (T,B), weight (T,B) or
 * NULL.  losses (3,) = policy, value, entropy.  ws: hpc_rll_vtrace_workspace_floats(T,B) floats; its
 * first 3*T*B floats (pg / entropy coefficients, unit value gradient) must survive until backward.
 * backward recomputes the softmax from target_output (no saved (T,B,N) buffers). */
int64_t hpc_rll_vtrace_workspace_floats(int T, int B);
int hpc_rll_vtrace_forward(const float* target_output, const float* behaviour_output, const int64_t* action,
                           const float* value, const float* reward, const float* weight, float* losses, float* ws,
                           int T, int B, int N, float gamma, float lambda, float rho_clip, float c_clip,
                           float rho_pg_clip, float scale, void* stream);
int hpc_rll_vtrace_backward(const float* g_pg, const float* g_value, const float* g_ent, const float* target_output,
                            const int64_t* action, const float* ws, float* grad_target_output, float* grad_value,
                            int T, int B, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * Episode-aware TD(lambda) and V-trace with done / truncation masks (no reference counterpart: hpc_rll/origin/td.py
 * leaves terminal states to the caller).  Masks as for hpc_rll_gae_masked_*: k^d_t = 1 - done_t, k^f_t = 1 - f_t with
 * f = traj_flag defaulting to done, (T,B) of `mask_dtype`, either may be NULL; nv_t = next_value[t] (next-value form:
 * value, next_value (T,B)) or value[t+1] (stacked form: next_value = NULL, value (T+1,B)).  Time-limit truncation:
 * done_t = 0, traj_flag_t = 1 and the final observation's value in next_value[t].  k^d weights the bootstrap value,
 * k^f the continuation.  disc = gamma*lambda and gamma - disc are rounded to fp32 as in the unmasked ops.
 *
 * TD(lambda):  G_T = nv_{T-1},  G_t = r_t + (gamma*k^d_t - disc*k^f_t)*nv_t + disc*k^f_t*G_{t+1};
 *   loss (1,) = 0.5*scale*sum w (G_t - V_t)^2 with weight_mode / weight as hpc_rll_td_lambda_forward; grad_buf (T,B) =
 *   d loss / d value[:T] (G is a constant).  Backward: hpc_rll_td_lambda_backward (stacked form, grad_value (T+1,B),
 *   last row 0) or hpc_rll_scale_rows(grad_loss, grad_buf, grad_value, T*B, T*B) (next-value form).
 * V-trace:  IS, rho, c, rho_pg and the entropy as hpc_rll_vtrace_forward;  s_T = 0,
 *   s_t = rho_t*(r_t + gamma*k^d_t*nv_t - V_t) + disc*k^f_t*c_t*s_{t+1}   (vs_t = V_t + s_t),
 *   adv_t = rho_pg_t*(r_t + gamma*(k^d_t*nv_t + k^f_t*s_{t+1}) - V_t);  losses and ws as hpc_rll_vtrace_forward (same
 *   workspace size).  Backward: hpc_rll_vtrace_backward (stacked form), or hpc_rll_vtrace_backward with grad_value = NULL
 *   plus hpc_rll_scale_rows(g_value, ws + 2*T*B, grad_value, T*B, T*B) (next-value form).
 * Without masks, or with all-zero masks, both equal their unmasked op bit for bit (the same launch configuration for
 * the same (T,B)); with f = done and soft masks they are the per-step-discount forms with discount gamma*(1 - m).
 * Argument errors: HPC_RLL_EINVAL (null pointers, bad mask_dtype / weight_mode, negative sizes), HPC_RLL_EALIGN.
 * ------------------------------------------------------------------------------------------ */
int hpc_rll_td_lambda_masked_forward(const float* value, const float* next_value, const float* reward,
                                     const float* weight, int weight_mode, const void* done, const void* traj_flag,
                                     int mask_dtype, float* loss, float* grad_buf, float* partials, int T, int B,
                                     float gamma, float lambda, float scale, void* stream);
int hpc_rll_vtrace_masked_forward(const float* target_output, const float* behaviour_output, const int64_t* action,
                                  const float* value, const float* next_value, const float* reward, const float* weight,
                                  const void* done, const void* traj_flag, int mask_dtype, float* losses, float* ws,
                                  int T, int B, int N, float gamma, float lambda, float rho_clip, float c_clip,
                                  float rho_pg_clip, float scale, void* stream);

/* UPGO -- replaces UpgoForward/Backward (rl_utils/entry.h:148-156, src/rl_utils/upgo.cu:8-70).
 * target_output (T,B,N), rho (T,B), action (T,B), reward (T,B), value (T+1,B); loss (1,). */
int64_t hpc_rll_upgo_workspace_floats(int T, int B);
int hpc_rll_upgo_forward(const float* target_output, const float* rho, const int64_t* action, const float* reward,
                         const float* value, float* loss, float* ws, int T, int B, int N, float scale, void* stream);
int hpc_rll_upgo_backward(const float* g, const float* target_output, const int64_t* action, const float* ws,
                          float* grad_target_output, int T, int B, int N, void* stream);

/* Episode-aware UPGO with done / truncation masks (no reference counterpart: hpc_rll_upgo_forward carries the return and
 * the comparison r_{t+1} + V_{t+2} >= V_{t+1} across an episode end and has no discount).  Masks, mask_dtype and the two
 * value forms as hpc_rll_td_lambda_masked_forward: k^d_t = 1 - done_t, k^f_t = 1 - f_t (f = traj_flag, defaulting to
 * done), nv_t = value[t+1] (stacked: next_value = NULL, value (T+1,B)) or next_value[t] (value, next_value (T,B)).
 *   q_t   = fmaf(gamma, k^d_t*nv_t, r_t)                       the one-step target of step t
 *   lam_t = 1 for t = T-1, else [q_{t+1} >= value[t+1]]        (row t+1 of `value` in both forms; step t+1's own done)
 *   a_t   = gamma*k^f_t*lam_t,   G_T = nv_{T-1},   G_t = fmaf(gamma*k^d_t - a_t, nv_t, r_t) + a_t*G_{t+1}
 *   loss (1,) = -scale * sum rho (G_t - V_t) log pi(action), G a constant.
 * A done step returns r_t; a time-limit truncation (next-value form, done_t = 0, traj_flag_t = 1, the final observation's
 * value in next_value[t]) returns r_t + gamma*nv_t.  With gamma = 1, the stacked form and no masks (or all-zero masks) the
 * loss and the saved coefficients equal hpc_rll_upgo_forward's bit for bit (the same launch configuration).
 * ws: hpc_rll_upgo_workspace_floats(T,B) floats with the layout of hpc_rll_upgo_forward; backward: hpc_rll_upgo_backward.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (negative sizes, N <= 0, NULL loss, bad mask_dtype, other NULL
 * operands), HPC_RLL_EALIGN; T == 0 or B == 0 zeroes loss.
 * hpc_rll_upgo_masked_last_config: the HPC_RLL_SCAN_CONFIG_INTS ints of hpc_rll_scan_last_config for this op ({0, -1 ...}
 * before its first launch; HPC_RLL_EINVAL and nothing written for out == NULL).  The record is private to this entry
 * point: the op list of hpc_rll_scan_last_config is part of ABI 6 and is unchanged. */
int hpc_rll_upgo_masked_forward(const float* target_output, const float* rho, const int64_t* action, const float* reward,
                                const float* value, const float* next_value, const void* done, const void* traj_flag,
                                int mask_dtype, float* loss, float* ws, int T, int B, int N, float gamma, float scale,
                                void* stream);
int hpc_rll_upgo_masked_last_config(int* out);

/* Retrace(lambda): off-policy multi-step Q targets for discrete actions and ACER's critic loss (no reference counterpart;
 * the semantics are DI-engine's compute_q_retraces and acer_value_error).  q_values (T+1,B,N), action (T,B) int64,
 * reward, weights, loss_weight (T,B) (weights = continuation weight, e.g. 1 - done; NULL = ones, as is loss_weight).
 * With a_t = action[t,b], qa_t = q_values[t,b,a_t], v_t the state value (t = 0..T) and c_t = lambda*min(1, ratio_t):
 *   Q_T = v_T,   Q_t = r_t + gamma*w_t*(c_{t+1}*(Q_{t+1} - qa_{t+1}) + v_{t+1}),  the c*(Q - qa) term := 0 at t+1 = T
 *   scan form: a_t = (gamma*w_t)*c_{t+1},  b_t = fmaf(gamma*w_t, fmaf(-c_{t+1}, qa_{t+1}, v_{t+1}), r_t).
 * A zero weight gives Q_t = r_t exactly.  1 <= N <= 1024, beyond that HPC_RLL_EUNSUPPORTED.
 * An action outside [0,N) never addresses memory: it matches no column, so qa = 0, the gathered ratio is 0 (c = 0) in the
 * drop-in form, the fused form takes 0 for both selected logits, and the sample's gradient row is all zeros.
 * hpc_rll_retrace_forward -- the drop-in form: v_pred (T+1,B) and ratio (T,B,N) are given, ratio_t = ratio[t,b,a_t].
 *   Writes q_retraces (T+1,B).  ws: at least 2*T*B floats, layout qa (T*B) | c (T*B).
 * hpc_rll_retrace_loss_forward -- the fused form: target_output (T+1,B,N) and behaviour_output (T,B,N) are logits,
 *   pi = softmax(target_output), v_t = sum_n pi_n q_n (written to v_pred (T+1,B)), ratio_t = exp(log pi_t(a_t) - log mu_t(a_t));
 *   loss (1,) = scale * 0.5 * sum_{t<T,b} lw (Q_t - qa_t)^2 with Q a constant; q_retraces (T+1,B).
 *   ws: hpc_rll_retrace_workspace_floats(T,B) floats, layout delta (T*B) | qa (T*B) | c (T*B) | partial sums, with
 *   delta = lw*(qa_t - Q_t)*scale.  T == 0 or B == 0 zeroes loss and launches nothing.
 * hpc_rll_retrace_loss_backward -- grad_q_values (T+1,B,N), every element written once:
 *   grad[t,b,n] = g_loss*delta[t,b]*[n == a_t] for t < T, row T is zero.  g_loss is a device scalar (NULL = 1).
 * hpc_rll_retrace_last_config -- the HPC_RLL_SCAN_CONFIG_INTS ints of hpc_rll_scan_last_config for the Retrace scan of either
 *   form ({0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL).  [7] (mask mode) holds bit 0 = weights
 *   given, bit 1 = loss_weight given; [8] is 1 for the drop-in form, 0 for the fused form; [10] is 0 for the drop-in form
 *   (no loss).  The record is private to this entry point, as hpc_rll_upgo_masked_last_config's is.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands, then negative sizes or N <= 0), HPC_RLL_EALIGN (a
 * pointer off 4-byte alignment, action off 8), then HPC_RLL_EUNSUPPORTED (N > 1024); then empty shapes return 0. */
int64_t hpc_rll_retrace_workspace_floats(int T, int B);
int hpc_rll_retrace_forward(const float* q_values, const float* v_pred, const float* rewards, const int64_t* actions,
                            const float* weights, const float* ratio, float* q_retraces, float* ws, int T, int B, int N,
                            float gamma, float lambda, void* stream);
int hpc_rll_retrace_loss_forward(const float* q_values, const float* target_output, const float* behaviour_output,
                                 const int64_t* action, const float* reward, const float* weights,
                                 const float* loss_weight, float* loss, float* q_retraces, float* v_pred, float* ws, int T,
                                 int B, int N, float gamma, float lambda, float scale, void* stream);
int hpc_rll_retrace_loss_backward(const float* g_loss, const int64_t* action, const float* ws, float* grad_q_values, int T,
                                  int B, int N, void* stream);
int hpc_rll_retrace_last_config(int* out);

/* ACER's actor loss for discrete actions (no reference counterpart; the semantics restate DI-engine's acer_policy_error and
 * acer_trust_region_update).  target_output, behaviour_output, avg_output, q_values: T*B rows of N logits / values;
 * q_retraces, v_pred (T*B); action (T,B) int64; weights (T,B) (NULL = ones: nothing is multiplied); avg_output NULL = no
 * trust region.  Only the first T*B rows of an operand are read, so the (T+1,B,..) tensors hpc_rll_retrace_loss_forward
 * takes and returns pass as they are.  Per sample, with l = log_softmax(x), pi = exp l, d_n = l_n - log_softmax(y)_n,
 * k = softmax(u), A^ret = q_retraces - v_pred, A_n = q_n - v_pred, c = c_clip_ratio, beta = entropy_weight:
 *   ca = min(c, exp d_a) A^ret,   bc_n = max(0, 1 - c exp(-d_n)) pi_n A_n        (constants of the loss)
 *   La = ca l_a,  Lb = sum_n bc_n l_n,  H = -sum_n pi_n l_n
 *   out4 = { -scale sum w (La + Lb + beta H),  scale sum w La,  scale sum w Lb,  scale sum w H }
 *   g_n = -([n = a] ca + bc_n - beta pi_n (l_n + 1)),  s = max(0, (sum k g - trust_region_value) / sum k^2) (0 without
 *   avg_output),  z = g - s k,  unit_grad[t,b,n] = w scale (z_n - pi_n sum_m z_m).
 * A target logit of -inf is clamped to the most negative finite float; its column has pi_n = 0, adds exactly 0 to every
 * sum and gets gradient 0 (the sums select on pi_n > 0).  An action outside [0,N) never addresses memory: ca = 0.
 * hpc_rll_acer_policy_forward -- one launch.  unit_grad (T,B,N) may be NULL: the gradient is then not formed.
 *   ws: hpc_rll_acer_policy_workspace_floats(T,B) floats (the partial sums).  T == 0 or B == 0 zeroes out4, launches nothing.
 * hpc_rll_acer_policy_backward -- grad_target_output (target_rows,B,N) = g_loss * unit_grad for the first T rows, zero in
 *   row T when target_rows == T+1 (target_rows is T or T+1); g_loss is a device scalar (required); one streaming launch.
 * hpc_rll_acer_trust_region -- the projection alone, for DI-engine's acer_trust_region_update: actor_gradient, avg_logit
 *   (log-probabilities), out (rows,N):  out = g - max(0, (sum k g - trust_region_value) / sum k^2) k,  k = exp(avg_logit).
 * hpc_rll_acer_last_config -- out[HPC_RLL_ACER_CONFIG_INTS] = { launches of the two forward entry points so far, G, VEC, E
 *   (lanes per row, floats per load, loads per lane and row), R (rows per group and iteration), flags (bit 0 weights given,
 *   bit 1 avg_output given, bit 2 unit_grad stored), workgroups, 1 if the latest launch was hpc_rll_acer_trust_region };
 *   {0, -1 ...} before the first launch; HPC_RLL_EINVAL for out == NULL.
 * 1 <= N <= 1024, beyond that HPC_RLL_EUNSUPPORTED.  Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands,
 * then negative sizes, N <= 0 or a bad target_rows), HPC_RLL_EALIGN (a pointer off 4-byte alignment, action off 8), then
 * HPC_RLL_EUNSUPPORTED (N > 1024); then empty shapes return 0. */
#define HPC_RLL_ACER_CONFIG_INTS (8)
int64_t hpc_rll_acer_policy_workspace_floats(int T, int B);
int hpc_rll_acer_policy_forward(const float* target_output, const float* behaviour_output, const float* avg_output,
                                const float* q_values, const float* q_retraces, const float* v_pred, const int64_t* action,
                                const float* weights, float* out4, float* unit_grad, float* ws, int T, int B, int N,
                                float c_clip_ratio, float entropy_weight, float trust_region_value, float scale,
                                void* stream);
int hpc_rll_acer_policy_backward(const float* g_loss, const float* unit_grad, float* grad_target_output, int T, int B,
                                 int N, int target_rows, void* stream);
int hpc_rll_acer_trust_region(const float* actor_gradient, const float* avg_logit, float* out, int64_t rows, int N,
                              float trust_region_value, void* stream);
int hpc_rll_acer_last_config(int* out);

/* COMA: the counterfactual multi-agent actor-critic loss (no reference counterpart; the semantics restate DI-engine's
 * coma_error, Foerster et al. 2018).  logit, q_value, target_q_value (T,B,A,N); action (T,B,A) int64; reward (T,B), row T-1
 * is not read; weight (T,B,A) (NULL = ones: nothing is multiplied); done (T,B) of `mask_dtype` (HPC_RLL_MASK_U8 /
 * HPC_RLL_MASK_F32; NULL = no episode ends), k = 1 - done.  Per row (t,b,i) with x the logit row, q / q' the value rows,
 * a the action, l = log_softmax(x), pi = exp l, H = -sum_n pi_n l_n, qa = q[a], tqa = q'[a], adv = qa - sum_n pi_n q_n
 * (a constant of the loss), and per column (b,i), disc = gamma*lambda (in fp32), rest = gamma - disc:
 *   R_{T-2} = r[T-2,b] + k_{T-2} gamma tqa_{T-1},   R_t = r[t,b] + k_t (disc R_{t+1} + rest tqa_{t+1})   (a constant of the loss)
 *   scan form over T-1 steps and B*A columns: s_{T-1} = tqa_{T-1}, a_t = k_t disc, b_t = fmaf(k_t rest, tqa_{t+1}, r_t)
 *   loss[3] = { -scale_pe sum w l_a adv,   scale_q sum_{t<T-1} w (R_t - qa_t)^2,   scale_pe sum w H }
 *   grad_logit[n]   = -g_policy w adv scale_pe ([n = a] - pi_n) + g_entropy w scale_pe (-pi_n (l_n + H))
 *   grad_q_value[n] =  g_q 2 w (qa - R) scale_q [n = a]  for t < T-1;  row T-1 is zero.
 * A logit of -inf is clamped to the most negative finite float: its column has pi_n = 0, adds exactly 0 to H and to the
 * baseline and gets gradient 0.  An action outside [0,N) never addresses memory: qa = tqa = 0, the row's policy term and
 * q term are dropped and neither gradient row has a one-hot part; the entropy is unaffected.  1 <= N <= 1024, beyond that
 * HPC_RLL_EUNSUPPORTED; B*A must fit an int (HPC_RLL_EINVAL otherwise); element offsets are 64-bit.
 * hpc_rll_coma_forward -- two launches (heads over T*B*A rows, the return scan over T-1 steps; T == 1: the heads only,
 *   loss[1] = 0).  ws: hpc_rll_coma_workspace_floats(T,B,A) floats, with R = T*B*A the layout is
 *   delta (R; rows t < T-1 are written: 2 w (qa - R_t) scale_q) | qa (R) | tqa (R) | lse (R) | H (R) |
 *   w adv scale_pe (R; 0 for an action outside) | partial sums of the heads | partial sums of the scan.
 *   T, B or A == 0 zeroes loss[3] and launches nothing.
 * hpc_rll_coma_backward -- one streaming launch without reductions or atomics: reads logit once and the saved per-row
 *   floats of ws, writes every element of grad_logit and grad_q_value (T,B,A,N) once.  Either output may be NULL (it is then
 *   neither computed nor written; logit may then be NULL when grad_logit is); with both NULL nothing is launched.
 *   g_policy, g_q, g_entropy are device scalars (NULL = 1); weight and scale_pe as given to the forward.
 * hpc_rll_coma_last_config -- out[HPC_RLL_COMA_CONFIG_INTS] = {
 *    [0..10]  the HPC_RLL_SCAN_CONFIG_INTS ints of hpc_rll_scan_last_config for the COMA scan (private to this entry point, as
 *             hpc_rll_retrace_last_config's are): [6] the mask element type, [7] 1 = done given, [8] 1 = weight given,
 *    [11..17] the heads: launches so far, G, VEC, E (lanes per row, floats per load, loads per lane and row), R (rows per
 *             group and iteration), flags (bit 0 weight given), workgroups,
 *    [18..24] the backward: launches so far, G, VEC, E, R, flags (bit 0 grad_logit written, bit 1 grad_q_value written,
 *             bit 2 weight given), workgroups };
 *   each of the three parts is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands, then negative sizes, N <= 0, a B*A past an int or an
 * unknown mask_dtype), HPC_RLL_EALIGN (a pointer off 4-byte alignment, action off 8; a byte mask has none), then
 * HPC_RLL_EUNSUPPORTED (N > 1024); then empty shapes return 0. */
#define HPC_RLL_COMA_CONFIG_INTS (25)
int64_t hpc_rll_coma_workspace_floats(int T, int B, int A);
int hpc_rll_coma_forward(const float* logit, const int64_t* action, const float* q_value, const float* target_q_value,
                         const float* reward, const float* weight, const void* done, int mask_dtype, float* loss,
                         float* ws, int T, int B, int A, int N, float gamma, float lambda, float scale_pe, float scale_q,
                         void* stream);
int hpc_rll_coma_backward(const float* g_policy, const float* g_q, const float* g_entropy, const float* logit,
                          const int64_t* action, const float* weight, const float* ws, float* grad_logit,
                          float* grad_q_value, int T, int B, int A, int N, float scale_pe, void* stream);
int hpc_rll_coma_last_config(int* out);

/* R2D2 sequence loss: the n-step (double-)Q TD error of every step of a whole unroll, its loss, the replay priority and the
 * gradient, in a number of launches that does not depend on T (no reference counterpart; the semantics restate the loop of
 * DI-engine's r2d2 policy over q_nstep_td_error / q_nstep_td_error_with_rescale).  q, target_q (T,B,N); action (T,B) int64;
 * reward (T,B); done (T,B) of `mask_dtype` (HPC_RLL_MASK_U8 / HPC_RLL_MASK_F32; NULL = no episode ends), k_t = 1 - done_t;
 * weight with weight_mode 0 none (NULL: nothing is multiplied), 1 (B,), 2 (T,B) indexed by the absolute t.  The valid steps
 * are t = burnin .. T-nstep-1, L = T - nstep - burnin of them.  For a valid (t,b), with n = nstep:
 *   a = action[t,b], qa = q[t,b,a];  a* = the LOWEST index of max_n sel[t+n,b,:], sel = q (double_q) or target_q;
 *   v = target_q[t+n,b,a*], h_inverse(v) with value_rescale (eps = 1e-2, as hpc_rll_q_nstep_td_forward's rescale form);
 *   p_0 = 1, p_{j+1} = (p_j gamma) k_{t+j};  G = sum_{j<n} p_j reward[t+j,b] + p_n v, h_transform(G) with value_rescale;
 *   d = qa - G;  td_error[t-burnin,b] = d^2;  loss = scale sum_{t,b} w d^2  (G is a constant);
 *   priority[b] = eta max_t td_error[.,b] + (1 - eta) mean_t td_error[.,b]  (unweighted);
 *   grad_q[t,b,n] = g 2 w d scale [n = a] on valid rows and 0 on every other row.
 * A done at step t+j keeps reward[t+j] and cuts everything after it in that window; a done at t+n or later does not touch
 * step t.  An action outside [0,N) never addresses memory: the step is dropped (d = 0: nothing for the loss or the priority,
 * a zero gradient row).  NaN in sel is not supported.  1 <= N <= 1024, beyond that HPC_RLL_EUNSUPPORTED.
 * hpc_rll_r2d2_forward -- three launches: the heads over the rows t >= burnin (qa and v per row), the window over the L*B
 *   valid steps (td_error, delta, the loss), the priority over td_error (L,B) (fixed-order sums, no atomics).  ws:
 *   hpc_rll_r2d2_workspace_floats(T,B) floats, with R = T*B the layout is
 *   delta (R; rows burnin .. T-nstep-1 are written: 2 w d scale) | qa (R) | v (R) (rows burnin .. T-1 of both are written) |
 *   partial sums of the window launch (one per workgroup, at most 512).
 *   T == 0, B == 0 or L <= 0 zeroes loss and priority (B,) and launches nothing.
 * hpc_rll_r2d2_backward -- one streaming launch: every float of grad_q (T,B,N) written once, q is not read.  g_loss is a
 *   device scalar (NULL = 1); nstep and burnin as given to the forward.
 * hpc_rll_r2d2_last_config -- out[HPC_RLL_R2D2_CONFIG_INTS] = {
 *    [0..6]   the heads: launches so far, G, VEC, E (lanes per row, floats per load, loads per lane and row), R (rows per
 *             group and iteration), flags (bit 0 double_q, bit 1 value_rescale), workgroups,
 *    [7..11]  the window: launches so far, threads per workgroup, flags (bits 0-1 the mask: 0 none, 1 bytes, 2 floats;
 *             bits 2-3 weight_mode; bit 4 value_rescale), workgroups, finalisation (1 = inside the launch, 2 = one more launch),
 *    [12..13] the priority: launches so far, workgroups,
 *    [14..16] the backward: launches so far, floats per store, workgroups };
 *   each of the four parts is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands, then negative sizes, N <= 0, nstep < 1, burnin < 0,
 * an unknown mask_dtype or weight_mode, a weight that does not match its mode), HPC_RLL_EALIGN (a pointer off 4-byte
 * alignment, action off 8; a byte mask has none), then HPC_RLL_EUNSUPPORTED (N > 1024); then empty shapes return 0. */
#define HPC_RLL_R2D2_CONFIG_INTS (17)
int64_t hpc_rll_r2d2_workspace_floats(int T, int B);
int hpc_rll_r2d2_forward(const float* q, const float* target_q, const int64_t* action, const float* reward, const void* done,
                         int mask_dtype, const float* weight, int weight_mode, float* loss, float* td_error, float* priority,
                         float* ws, int T, int B, int N, int nstep, int burnin, float gamma, int value_rescale, int double_q,
                         float priority_eta, float scale, void* stream);
int hpc_rll_r2d2_backward(const float* g_loss, const int64_t* action, const float* ws, float* grad_q, int T, int B, int N,
                          int nstep, int burnin, void* stream);
int hpc_rll_r2d2_last_config(int* out);

/* Soft Actor-Critic for discrete actions: the soft value of the next state, the TD target, both critic losses, the policy
 * loss, the entropy and the gradients (no reference counterpart; the semantics restate DI-engine's
 * DiscreteSACPolicy._forward_learn with q_v_1step_td_error).  logit, next_logit, q1, q2, target_q1, target_q2: `rows` rows
 * of N floats; action (rows) int64; reward (rows); done (rows) of `mask_dtype` (HPC_RLL_MASK_U8 / HPC_RLL_MASK_F32; NULL =
 * no episode ends), k = 1 - done; weight (rows) (NULL = ones: an exact 1 is multiplied).  q2 and target_q2 are both given or
 * both NULL (a single critic: m = q1, m' = target_q1).  The temperature is alpha_dev[0], a device scalar, when alpha_dev is
 * given, otherwise `alpha`.  Per sample, with x, y the logit and next_logit rows and a the action:
 *   l' = log_softmax(y), p' = exp l', m' = min(target_q1, target_q2),  V' = sum_n p'_n (m'_n - alpha l'_n)
 *   G = reward + gamma k V'  (a constant),   d_i = q_i[a] - G,   td_error = mean_i d_i^2 (unweighted),   target_q = G
 *   l = log_softmax(x), p = exp l, m = min(q1, q2) (a constant),  t_n = alpha l_n - m_n,  f = sum_n p_n t_n,  H = -sum_n p_n l_n
 *   out4 = { scale sum f,  scale sum w d_1^2,  scale sum w d_2^2 (0 for a single critic),  scale sum H }
 *   unit_grad[b,n] = scale p_n (t_n - f),   grad_logit = g_policy unit_grad,   grad_q_i[b,n] = g_i 2 scale w d_i [n = a].
 * A logit of -inf is clamped to the most negative finite float: its column has p_n = 0, adds exactly 0 to V', f and H
 * whatever the critics hold there and gets gradient 0 (the sums select on p_n > 0).  An action outside [0,N) never addresses
 * memory: d_i = 0, td_error = 0 and the critic gradient rows are zero; the policy part is unaffected.
 * hpc_rll_sac_discrete_forward -- one launch.  unit_grad (rows,N) may be NULL: the logit gradient is then not formed.
 *   ws: hpc_rll_sac_discrete_workspace_floats(rows) floats: delta_1 (rows: 2 scale w d_1) | delta_2 (rows; written for twin
 *   critics) | the partial sums.  rows == 0 zeroes out4 and launches nothing.
 * hpc_rll_sac_discrete_backward -- one streaming launch without reductions or atomics: every float of each given output
 *   (rows,N) is written once.  Any output may be NULL (it is then neither computed nor written; unit_grad may be NULL when
 *   grad_logit is); with all NULL nothing is launched.  g_policy, g_critic, g_twin are device scalars (NULL = 1).
 * hpc_rll_sac_discrete_last_config -- out[HPC_RLL_SAC_CONFIG_INTS] = {
 *    [0..6]  the forward: launches so far, G, VEC, E (lanes per row, floats per load, loads per lane and row), R (rows per
 *            group and iteration), flags (bit 0 weight given; bits 1-2 done: 0 none, 1 bytes, 2 floats; bit 3 twin critics;
 *            bit 4 unit_grad stored), workgroups,
 *    [7..13] the backward: launches so far, G, VEC, E, R, flags (bit 0 grad_logit, bit 1 grad_q1, bit 2 grad_q2 written),
 *            workgroups };
 *   each part is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * 1 <= N <= 1024, beyond that HPC_RLL_EUNSUPPORTED.  Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands,
 * one of q2 / target_q2 without the other, then negative sizes, N <= 0 or an unknown mask_dtype), HPC_RLL_EALIGN (a pointer
 * off 4-byte alignment, action off 8; a byte mask has none), then HPC_RLL_EUNSUPPORTED (N > 1024); then empty shapes return 0. */
#define HPC_RLL_SAC_CONFIG_INTS (14)
int64_t hpc_rll_sac_discrete_workspace_floats(int64_t rows);
int hpc_rll_sac_discrete_forward(const float* logit, const float* next_logit, const float* q1, const float* q2,
                                 const float* target_q1, const float* target_q2, const int64_t* action, const float* reward,
                                 const void* done, int mask_dtype, const float* weight, const float* alpha_dev, float alpha,
                                 float* out4, float* td_error, float* target_q, float* unit_grad, float* ws, int64_t rows,
                                 int N, float gamma, float scale, void* stream);
int hpc_rll_sac_discrete_backward(const float* g_policy, const float* g_critic, const float* g_twin, const float* unit_grad,
                                  const int64_t* action, const float* ws, float* grad_logit, float* grad_q1, float* grad_q2,
                                  int64_t rows, int N, void* stream);
int hpc_rll_sac_discrete_last_config(int* out);

/* Soft Actor-Critic for continuous actions: the tanh-squashed Gaussian head and the SAC losses (no reference counterpart; the
 * semantics restate DI-engine's SACPolicy._forward_learn with q_v_1step_td_error).
 * The head.  mu, sigma, eps: `rows` rows of A floats; eps is standard-normal noise and a constant of the op (there is no RNG in
 * the kernel); sigma > 0 is the caller's contract.  Per row:
 *   u_j  = mu_j + sigma_j eps_j,   a_j = tanh(u_j)                                                      -> action (rows,A)
 *   logp = sum_j [ -eps_j^2/2 - log sigma_j - log(2 pi)/2 + 2|u_j| + 2 log1p(exp(-2|u_j|)) - 2 log 2 ]  -> log_prob (rows)
 * The last three terms are -log(1 - tanh^2 u_j) exactly: log_prob is formed from u, never from the rounded a (in fp32 a is
 * exactly +-1 from |u| ~ 9).  DI-engine takes log(1 - a^2 + 1e-6) there; the two agree to 1e-6 / (1 - tanh^2 u) per dimension.
 *   gu_j = g_a_j (1 - a_j^2) + 2 g_l a_j,   grad_mu_j = gu_j,   grad_sigma_j = gu_j eps_j - g_l / sigma_j
 * hpc_rll_tanh_gaussian_rsample_forward -- one launch; action (rows,A) and log_prob (rows) are written once.
 * hpc_rll_tanh_gaussian_rsample_backward -- one streaming launch without reductions or atomics.  g_action (rows,A) and
 *   g_log_prob (rows) may each be NULL (zero, not read); grad_mu and grad_sigma may each be NULL (not formed; sigma and eps are
 *   read for grad_sigma alone and may be NULL without it); with both NULL nothing is launched.  `action` is the forward's.
 *   Where a = +-1 exactly the g_action part of the gradient is exactly 0.
 * 16-byte loads and stores need A % 4 == 0 and every (rows,A) pointer the launch touches on 16 bytes, outputs included.
 * The losses.  One float per sample in every operand (`rows` floats); done (rows) of `mask_dtype` (HPC_RLL_MASK_U8 /
 * HPC_RLL_MASK_F32; NULL = no episode ends), k = 1 - done; weight (rows) (NULL = ones: an exact 1 is multiplied).  The
 * temperature is alpha_dev[0], a device scalar, when alpha_dev is given, otherwise `alpha`.
 *   m' = min(target_q1, target_q2),  G = reward + gamma k (m' - alpha next_log_prob)  (a constant),  target_q = G
 *   d_i = q_i - G,   td_error = mean_i d_i^2 (unweighted),   m = min(new_q1, new_q2)
 *   out4 = { scale sum (alpha log_prob - m),  scale sum w d_1^2,  scale sum w d_2^2 (0 for a single critic),  -scale sum log_prob }
 *   grad_q_i = g_i 2 scale w d_i,   grad_log_prob = g_policy alpha scale,   grad_new_q_i = -g_policy scale s_i
 * s_i is 1 for the strictly smaller of new_q1, new_q2, 0 for the other and 1/2 each at a tie (torch.minimum's rule); both
 * minima propagate a NaN from either side, and 0 * NaN = NaN: a NaN target critic poisons G of its row even when done = 1.
 * The critic half (q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, td_error, target_q) is absent when q1
 * is NULL and the actor half (log_prob, new_q1, new_q2) when log_prob is NULL; the sums of an absent half are 0.  The second
 * critics q2, target_q2, new_q2 of the halves that are given are all given or all NULL (a single critic).
 * hpc_rll_sac_continuous_forward -- one launch.  ws: hpc_rll_sac_continuous_workspace_floats(rows) floats: 2 scale w d_1 |
 *   2 scale w d_2 | s_1 (rows each) | the partial sums and (alpha scale, scale).  rows == 0 zeroes out4 and launches nothing.
 * hpc_rll_sac_continuous_backward -- one streaming launch, each given output (rows) written once; any may be NULL, with all
 *   NULL nothing is launched.  g_policy, g_critic, g_twin are device scalars (NULL = 1).  `ws` is the forward's.
 * hpc_rll_sac_continuous_last_config -- out[HPC_RLL_SAC_CONTINUOUS_CONFIG_INTS] = four parts of {launches so far, G, VEC, E
 *   (lanes per row, floats per load, loads per lane and row), R (rows per group and iteration), flags, workgroups}:
 *    [0..6]   the head forward: flags 0,
 *    [7..13]  the head backward: flags bit 0 g_action given, bit 1 g_log_prob given, bit 2 grad_mu, bit 3 grad_sigma written,
 *    [14..20] the loss forward (G, VEC, E, R read 0): flags bit 0 weight given; bits 1-2 done: 0 none, 1 bytes, 2 floats;
 *             bit 3 twin critics; bit 4 the critic half, bit 5 the actor half given; bit 6 alpha read from the device,
 *    [21..27] the loss backward (G, VEC, E, R read 0): flags bit 0 grad_q1, bit 1 grad_q2, bit 2 grad_log_prob,
 *             bit 3 grad_new_q1, bit 4 grad_new_q2 written;
 *   each part is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * 1 <= A <= 1024, beyond that HPC_RLL_EUNSUPPORTED.  Argument errors, before any HIP call and with nothing written:
 * HPC_RLL_EINVAL (null operands, one of a twin set without the others, both halves absent, then negative sizes, A <= 0 or an
 * unknown mask_dtype), HPC_RLL_EALIGN (a float pointer off 4-byte alignment; a byte mask has none), then
 * HPC_RLL_EUNSUPPORTED (A > 1024); then empty shapes return 0. */
#define HPC_RLL_SAC_CONTINUOUS_CONFIG_INTS (28)
int hpc_rll_tanh_gaussian_rsample_forward(const float* mu, const float* sigma, const float* eps, float* action,
                                          float* log_prob, int64_t rows, int A, void* stream);
int hpc_rll_tanh_gaussian_rsample_backward(const float* g_action, const float* g_log_prob, const float* sigma,
                                           const float* eps, const float* action, float* grad_mu, float* grad_sigma,
                                           int64_t rows, int A, void* stream);
int64_t hpc_rll_sac_continuous_workspace_floats(int64_t rows);
int hpc_rll_sac_continuous_forward(const float* q1, const float* q2, const float* target_q1, const float* target_q2,
                                   const float* next_log_prob, const float* reward, const void* done, int mask_dtype,
                                   const float* weight, const float* log_prob, const float* new_q1, const float* new_q2,
                                   const float* alpha_dev, float alpha, float* out4, float* td_error, float* target_q,
                                   float* ws, int64_t rows, float gamma, float scale, void* stream);
int hpc_rll_sac_continuous_backward(const float* g_policy, const float* g_critic, const float* g_twin, const float* ws,
                                    float* grad_q1, float* grad_q2, float* grad_log_prob, float* grad_new_q1,
                                    float* grad_new_q2, int64_t rows, void* stream);
int hpc_rll_sac_continuous_last_config(int* out);

/* QMIX: the monotonic mixing network from the hypernetworks' outputs on, and the mixed one-step TD loss of a learner (no
 * reference counterpart; the semantics restate DI-engine's Mixer.forward and v_1step_td_error on the mixed values).  Per
 * sample (row): agent_q (A) the agents' chosen-action values; w1 (A,E) row-major, element [a,e] at a*E + e; b1 (E); w2 (E);
 * b2 (1) -- the RAW hypernetwork outputs, the absolute values are taken here.  The arrays hold `rows` such rows back to back.
 *   pre_e = b1_e + sum_a q_a |w1[a,e]|,   h_e = elu(pre_e) = pre_e > 0 ? pre_e : expm1(pre_e),   q_tot = b2 + sum_e h_e |w2_e|
 * The learner's loss takes the same five operands of the target network (target_*; they get no gradient), reward (rows),
 * done (rows) of `mask_dtype` (HPC_RLL_MASK_U8 / HPC_RLL_MASK_F32; NULL = no episode ends), k = 1 - done, and weight (rows)
 * (NULL = ones: an exact 1 is multiplied):
 *   y = reward + gamma k target_q_tot  (a constant),   d = q_tot - y,   td_error = d^2 (unweighted),
 *   loss[0] = scale sum_rows w d^2,   delta = 2 scale w d.
 * A NaN or inf of the target side reaches y even where done = 1 (k multiplies): it poisons td_error, delta and the gradients
 * of its own row, and the loss sum, and nothing else.
 * Gradients from g = dL/dq_tot per row:  dpre_e = g |w2_e| (pre_e > 0 ? 1 : exp(pre_e)),  grad_b2 = g,
 *   grad_w2_e = g h_e sgn(w2_e),  grad_b1_e = dpre_e,  grad_w1[a,e] = dpre_e q_a sgn(w1[a,e]),  grad_q_a = sum_e dpre_e |w1[a,e]|
 * with sgn(0) = 0: an entry of w1 or w2 that is exactly 0 gets gradient exactly 0.  pre_e is accumulated in fp32; the sum over
 * e, y and d are formed in fp64 and rounded once (td_error squares a difference of two long sums).
 * hpc_rll_qmix_mix_forward -- one launch: q_tot (rows).  Every input float is read once, nothing else is written.
 * hpc_rll_qmix_td_forward -- one launch: both mixes, td_error, q_tot, target_q_tot (rows each) and loss[0].
 *   ws: hpc_rll_qmix_workspace_floats(rows) floats: delta (rows) | the partial sums.  rows == 0 zeroes loss[0] and launches
 *   nothing.
 * hpc_rll_qmix_backward -- one launch without atomics: every float of each given output (grad_q (rows,A), grad_w1 (rows,A,E),
 *   grad_b1, grad_w2 (rows,E), grad_b2 (rows)) is written once.  Any output may be NULL (it is then neither computed nor
 *   written); with all NULL nothing is launched.  g is g_rows[row] when g_rows (rows), the upstream gradient of the plain mix,
 *   is given; otherwise delta[row] of `ws` times g_loss[0], a device scalar (NULL = 1).  pre_e is recomputed from the inputs;
 *   w1 is read a second time when grad_w1 or grad_q is wanted.
 * hpc_rll_qmix_last_config -- out[HPC_RLL_QMIX_CONFIG_INTS] = {
 *    [0..6]  the last forward of either kind: launches so far, G, VEC, PL (lanes per row, floats per load, loads per lane and
 *            E floats), R (rows per group and iteration), flags (bit 0 weight given; bits 1-2 done: 0 none, 1 bytes,
 *            2 floats; bit 3 the TD form), workgroups,
 *    [7..13] the backward: launches so far, G, VEC, PL, R, flags (bits 0-4 grad_q, grad_w1, grad_b1, grad_w2, grad_b2
 *            written; bit 5 g_rows given), workgroups };
 *   each part is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * The 16-byte loads and stores (VEC = 4) need E % 4 == 0 and w1, b1, w2 (of both networks; in the backward also grad_w1,
 * grad_b1, grad_w2) on 16 bytes; agent_q, b2 and the per-row arrays restrict nothing.
 * 1 <= A <= 64 and 1 <= E <= 256, beyond that HPC_RLL_EUNSUPPORTED.  Argument errors, before any HIP call: HPC_RLL_EINVAL
 * (null operands, then negative sizes, A <= 0, E <= 0 or an unknown mask_dtype), HPC_RLL_EALIGN (a float pointer off 4-byte
 * alignment; a byte mask has none), then HPC_RLL_EUNSUPPORTED; then empty shapes return 0. */
#define HPC_RLL_QMIX_CONFIG_INTS (14)
int64_t hpc_rll_qmix_workspace_floats(int64_t rows);
int hpc_rll_qmix_mix_forward(const float* agent_q, const float* w1, const float* b1, const float* w2, const float* b2,
                             float* q_tot, int64_t rows, int A, int E, void* stream);
int hpc_rll_qmix_td_forward(const float* agent_q, const float* w1, const float* b1, const float* w2, const float* b2,
                            const float* target_agent_q, const float* target_w1, const float* target_b1,
                            const float* target_w2, const float* target_b2, const float* reward, const void* done,
                            int mask_dtype, const float* weight, float* loss, float* td_error, float* q_tot,
                            float* target_q_tot, float* ws, int64_t rows, int A, int E, float gamma, float scale,
                            void* stream);
int hpc_rll_qmix_backward(const float* g_loss, const float* g_rows, const float* ws, const float* agent_q, const float* w1,
                          const float* b1, const float* w2, const float* b2, float* grad_q, float* grad_w1, float* grad_b1,
                          float* grad_w2, float* grad_b2, int64_t rows, int A, int E, void* stream);
int hpc_rll_qmix_last_config(int* out);

/* Categorical value losses: value regression as classification (no reference counterpart; the semantics restate the scalar
 * transforms and the two-hot of MuZero-style learners as LightZero writes them, DI-engine's symlog, DreamerV3's two-hot critic
 * targets and the HL-Gauss histogram loss of Farebrother et al. 2024).  logits (rows,N) contiguous.  The support is N atoms
 * v_i = v_min + i D, D = (v_max - v_min) / (N - 1); `transform` phi is HPC_RLL_TWOHOT_PHI_IDENTITY, _H (h of the n-step TD
 * losses with `eps` > 0) or _SYMLOG (sign(x) log(1 + |x|)).  `target_kind` says what `target` holds:
 *   HPC_RLL_TWOHOT_KIND_TWOHOT   target (rows) scalars y; c = clamp(phi(y), v_min, v_max), pos = (c - v_min) / D,
 *                                lo = min(floor(pos), N - 2), w = pos - lo:  t_lo = 1 - w, t_{lo+1} = w, every other t_i = 0
 *   HPC_RLL_TWOHOT_KIND_HLGAUSS  target (rows) scalars y; c as above, edges e_i = v_i - D/2 (i = 0..N), `sigma` > 0 in
 *                                transformed units, F(e) = erf((e - c) / (sqrt(2) sigma)):
 *                                t_i = (F(e_{i+1}) - F(e_i)) / (F(e_N) - F(e_0))
 *   HPC_RLL_TWOHOT_KIND_DENSE    target (rows,N) rows of probabilities t; transform, eps, sigma, v_min, v_max are not read
 * Per row, with p = softmax(x):  l = lse(x) - sum_i t_i x_i,  dl/dx_i = p_i - t_i.  A column with t_i == 0 adds exactly 0 to l
 * also where x_i = -inf (a masked action).  weight (rows), NULL = ones:  loss[0] = scale sum_r w_r l_r.  A row with w_r == 0
 * is dead: ell[r] = 0, its gradient row is zeros, and NaNs in its logits or target reach nothing.  A NaN scalar target of a
 * live row gives a NaN ell[r], a NaN loss[0] and a NaN gradient row; a NaN in a dense target row a NaN ell[r] and loss[0] and
 * a NaN gradient at its column; other rows are not affected.
 * The scalars of a row (phi(y), pos, w, the HL-Gauss centre and normaliser, sum_i t_i x_i, the expectation and phi^-1) are
 * formed in fp64 and rounded once; the row itself (maximum, exponentials, their sum, the logarithm, erff of the bin edges) is
 * fp32.
 * hpc_rll_twohot_ce_forward -- one launch: ell (rows), the unweighted per-row loss, and loss[0].
 *   ws: hpc_rll_twohot_workspace_floats(rows) floats: lse (rows) | coef (rows), coef_r = scale w_r | the partial sums.
 *   rows == 0 zeroes loss[0] and launches nothing.
 * hpc_rll_twohot_ce_backward -- one launch without atomics: every float of grad_logits (rows,N) is written once, row r as
 *   g_r (p - t) with p = exp(x - lse_r) and t rebuilt from the target;  g_r = g_rows[r] when g_rows (rows), the upstream
 *   gradient of ell, is given, otherwise coef_r times g_loss[0], a device scalar (NULL = 1); dead rows (coef_r == 0) are zeros
 *   in both forms.  `ws`, logits, target and the support are those of the forward.
 * hpc_rll_twohot_decode -- one launch: value (rows) = phi^-1(E), E = sum_i p_i v_i, and expected (rows) = E unless NULL.
 * hpc_rll_twohot_encode -- one launch: probs (rows,N), the two-hot or HL-Gauss rows of target (rows); a dense kind is
 *   HPC_RLL_EINVAL.
 * hpc_rll_twohot_last_config -- out[HPC_RLL_TWOHOT_CONFIG_INTS] = four parts of 7 ints, for the last forward, backward, decode
 *   and encode: launches so far, G, VEC, E (lanes per row, floats per load, loads per lane and row), R (rows per group and
 *   iteration), flags, workgroups.  flags: bits 1-2 target_kind, bits 3-4 transform (both 0 where not read); bit 0 weight
 *   given (forward), g_rows given (backward), expected wanted (decode); bit 5 g_loss used (backward).  The encode uses no row
 *   mapping: its G, E and R read 0.  Each part is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * The 16-byte loads and stores (VEC = 4) need N % 4 == 0 and logits (a dense target too; in the backward grad_logits, in the
 * encode probs) on 16 bytes; the per-row arrays restrict nothing.
 * 2 <= N <= 1024 (1 <= N for a dense target).  Argument errors, before any HIP call and with nothing written: HPC_RLL_EINVAL
 * (null operands, then negative rows, an unknown target_kind or transform, N below its minimum, v_max <= v_min, sigma <= 0 for
 * HL-Gauss, eps <= 0 for h), HPC_RLL_EALIGN (a pointer off 4-byte alignment), then HPC_RLL_EUNSUPPORTED (N > 1024); then empty
 * shapes return 0. */
#define HPC_RLL_TWOHOT_KIND_TWOHOT (0)
#define HPC_RLL_TWOHOT_KIND_HLGAUSS (1)
#define HPC_RLL_TWOHOT_KIND_DENSE (2)
#define HPC_RLL_TWOHOT_PHI_IDENTITY (0)
#define HPC_RLL_TWOHOT_PHI_H (1)
#define HPC_RLL_TWOHOT_PHI_SYMLOG (2)
#define HPC_RLL_TWOHOT_CONFIG_INTS (28)
int64_t hpc_rll_twohot_workspace_floats(int64_t rows);
int hpc_rll_twohot_ce_forward(const float* logits, const float* target, const float* weight, float* loss, float* ell,
                              float* ws, int64_t rows, int N, int target_kind, int transform, float eps, float sigma,
                              float v_min, float v_max, float scale, void* stream);
int hpc_rll_twohot_ce_backward(const float* g_loss, const float* g_rows, const float* ws, const float* logits,
                               const float* target, float* grad_logits, int64_t rows, int N, int target_kind, int transform,
                               float eps, float sigma, float v_min, float v_max, void* stream);
int hpc_rll_twohot_decode(const float* logits, float* value, float* expected, int64_t rows, int N, int transform, float eps,
                          float v_min, float v_max, void* stream);
int hpc_rll_twohot_encode(const float* target, float* probs, int64_t rows, int N, int target_kind, int transform, float eps,
                          float sigma, float v_min, float v_max, void* stream);
int hpc_rll_twohot_last_config(int* out);

/* Prioritized replay: a sum tree and a min tree over `capacity` leaves, fan-out 64, entirely in device memory (no reference
 * counterpart; the semantics restate DI-engine's AdvancedReplayBuffer with its SumSegmentTree / MinSegmentTree).  Forward only.
 * Every launching call runs on `stream`, never synchronises with the host and keeps nothing on the host that changes from
 * call to call, so it can be captured in a hipGraph and replayed.
 *
 * STATE: one buffer of hpc_rll_per_state_bytes(capacity) bytes, addressed in 4-byte words.  depth = ceil(log64(capacity)), at
 * least 1; level l (0 = root .. depth = leaves) has n_l = ceil(capacity / 64^(depth-l)) values and is padded to a multiple
 * of 64 words with 0 (sum tree) or +inf (min tree), so that the 64 children of node i of level l are the words 64 i .. 64 i
 * + 63 of level l + 1: one 256-byte read of a wave.  Order: the sum tree's levels 0..depth, the min tree's levels 0..depth,
 * HPC_RLL_PER_SCALAR_WORDS scalars, `capacity` stamps (int32, 0 between calls).  Scalars: [0] max_priority (float, 1 after
 * init), [1] the maximum the running update has seen (float bits), from [64] on the per-wave maxima of a batch-normalised
 * sample.  hpc_rll_per_state_bytes is strictly increasing in capacity; hpc_rll_per_capacity_of inverts it (HPC_RLL_EINVAL for
 * a size that is no state's).
 * hpc_rll_per_layout -- host only: out[HPC_RLL_PER_LAYOUT_INTS] = depth, words of the state, then (offset, n_l) in words for
 *   levels 0..4 of the sum tree, the same for the min tree ((-1, 0) for a level beyond depth), (offset, words) of the
 *   scalars and of the stamps.
 *
 * LEAF: (p + eps)^alpha of a priority p, formed in fp64 and rounded to fp32, at most 1e30; alpha = 1 and alpha = 0 are exact
 * (p + eps and 1).  A priority that is negative, NaN or infinite is replaced by max_priority as it was BEFORE the call.  After
 * the call max_priority is the larger of its old value and the finite, non-negative priorities of the call's in-range
 * entries (the losers of duplicates included).  A leaf never written is 0 in the sum tree; the min tree holds +inf for a
 * leaf that is 0.
 * NODE: recomputed from its 64 children c_0..c_63, never adjusted: the inclusive prefixes P_j are what the steps s = 1, 2, 4,
 * 8, 16, 32 of `x_j += x_{j-s} for j >= s` (all j at once, fp32) leave in x_j, and the node is P_63, that is
 * ((c_0+c_1)+(c_2+c_3))+... pairwise over neighbours, 6 roundings deep.  The min is exact in any order.  Integer leaves with a
 * total below 2^24 make every node and prefix exact; otherwise a node or prefix is within 48 * 2^-24 of the total.
 *
 * hpc_rll_per_init -- one launch: every leaf unwritten, max_priority = 1.
 * hpc_rll_per_update -- leaf idx[k] = leaf(priority[k]) for k < M, priority == NULL: leaf(max_priority).  Of several k with
 *   one index the highest k wins; an index outside [0, capacity) is skipped.  2 + depth launches: stamps (integer atomicMax of
 *   k + 1), leaves (written where the stamp is k + 1, which clears it), then levels depth-1 .. 0, in each of which a wave
 *   recomputes the sum and min of one parent: the parents of the M entries (an entry whose predecessor has the same parent
 *   leaves it to the predecessor), or every node of the level when it has no more than M.  No float atomics: same bits on
 *   every run.
 * hpc_rll_per_rebuild -- the whole index from priority (capacity): leaf i = leaf(priority[i]) for a finite priority >= 0,
 *   unwritten otherwise; max_priority = max(1, those priorities).  2 + depth launches (init, leaves, one per level over all
 *   its nodes).  The same bits as hpc_rll_per_init followed by updates that leave the same leaves.
 * hpc_rll_per_sample -- one wave per sample.  u (B) in [0,1), NaN counts as 0.  total = the root.  Target mass m = ((k +
 *   u_k) / B) total (stratified != 0) or u_k total, formed in fp64 and rounded to fp32.  At each node, from the root: j = the
 *   smallest with m < P_j and c_j > 0, or the last with c_j > 0 if there is none; then m = m - P_{j-1} (P_{-1} = 0) clamped
 *   into [0, c_j), and child j is the next node.  idx (B) int64 = the leaf reached, always one with a positive value; prob =
 *   leaf / total; weight = (size prob)^-beta, where size = *size_dev when size_dev != NULL and `size` otherwise.  normalize
 *   HPC_RLL_PER_NORM_BUFFER divides by (size min_leaf / total)^-beta with min_leaf the min tree's root, that is weight = (leaf
 *   / min_leaf)^-beta <= 1, HPC_RLL_PER_NORM_BATCH by the batch's largest weight (a second launch over the per-wave maxima),
 *   _NONE by nothing.  x^-beta is exp2(-beta log2 x) in fp32 (1 for beta = 0), within 4e-6 relative for |beta log2 x| <= 30.  A root
 *   that is not a positive finite number gives idx = -1, prob = weight = 0.  weight and prob may each be NULL.
 * hpc_rll_per_last_config -- out[HPC_RLL_PER_CONFIG_INTS] = two parts of 6 ints, for the last update (or rebuild) and the
 *   last sample: calls that launched so far, kernel, depth, workgroups of the first tree launch, launches of the call, flags.
 *   Update: kernel 0 = every level below the root through the touched parents, 1 = at least one of them recomputed in full,
 *   2 = rebuild; flags = bit l set when level l was recomputed in full (bit 0, the root, always: it is one parent either way).  Sample: kernel = normalize, flags = bit 0 stratified, bit 1 weight
 *   wanted, bit 2 prob wanted, bit 3 size read from the device.  {0, -1 ...} before the first launch.
 * Argument errors, before any HIP call and with nothing written: HPC_RLL_EINVAL (null operands, then capacity < 1, M or B
 * negative or past 2^31 - 2, alpha or eps negative or NaN, beta negative or NaN, a host size < 1, an unknown normalize),
 * HPC_RLL_EALIGN (a pointer off 4-byte alignment, idx or size_dev off 8), then HPC_RLL_EUNSUPPORTED (capacity > 2^24); then
 * M == 0 or B == 0 return 0 without a launch. */
#define HPC_RLL_PER_NORM_NONE (0)
#define HPC_RLL_PER_NORM_BUFFER (1)
#define HPC_RLL_PER_NORM_BATCH (2)
#define HPC_RLL_PER_MAX_CAPACITY (16777216)
#define HPC_RLL_PER_SCALAR_WORDS (8256)
#define HPC_RLL_PER_LAYOUT_INTS (26)
#define HPC_RLL_PER_CONFIG_INTS (12)
int64_t hpc_rll_per_state_bytes(int64_t capacity);
int64_t hpc_rll_per_capacity_of(int64_t state_bytes);
int hpc_rll_per_layout(int64_t capacity, int64_t* out);
int hpc_rll_per_init(void* state, int64_t capacity, void* stream);
int hpc_rll_per_update(void* state, int64_t capacity, const int64_t* idx, const float* priority, int64_t M, float alpha,
                       float eps, void* stream);
int hpc_rll_per_rebuild(void* state, int64_t capacity, const float* priority, float alpha, float eps, void* stream);
int hpc_rll_per_sample(void* state, int64_t capacity, const float* u, int64_t* idx, float* weight, float* prob, int64_t B,
                       int stratified, int normalize, float beta, int64_t size, const int64_t* size_dev, void* stream);
int hpc_rll_per_last_config(int* out);

/* Language-model policy losses: the per-token log-probability over a large vocabulary and GRPO's clipped-ratio + k3-KL token
 * loss with per-sequence masked means (no reference counterpart; the semantics restate DI-engine's grpo_policy_error /
 * rloo_policy_error and their log_prob_utils helper).  Logits are (rows, V) of element type HPC_RLL_ELEM_F32 or
 * HPC_RLL_ELEM_BF16, contiguous, 1 <= V <= 262144; action (rows) int64; lp(x) = x[a] - logsumexp(x).  A row whose action is
 * outside [0,V), or whose weight is 0, is DROPPED: its logits are not read (they may hold anything), logp = lse = 0, it
 * adds nothing to any sum and its gradient row is exact zeros.  -inf logits are vocabulary entries of probability 0; a
 * chosen token whose own logit is -inf is not supported.  NaN in a LIVE row is not propagated: the clamp that maps -inf to
 * the most negative finite float maps NaN there too, so such an entry counts with probability 0 (as hpc_rll_categorical_*).
 * hpc_rll_token_logp_forward -- one launch, one read of every live row: logp (rows), lse (rows; may be NULL); weight
 *   (rows; may be NULL) only selects the rows to drop.
 * hpc_rll_token_logp_backward -- one streaming launch: grad_logits[r,v] = g_logp[r] ([v = a] - exp(x_v - lse[r])) in the
 *   logits' element type (bf16: round to nearest even); a row with g_logp[r] == 0 is zero-filled without reading its logits.
 * hpc_rll_grpo_forward -- logit_new (B,S,V) of elem_new; old and ref are logits (kind = their element type) or per-token
 *   log-probs (B,S) fp32 (kind HPC_RLL_GRPO_LOGP); ref may be NULL (no KL term, beta ignored: RLOO / token-level PPO);
 *   adv (B); weight (B,S) or NULL (= ones).  Per token, with pn, po, pr the three log-probs:
 *     d = pr - pn, kl = exp(d) - d - 1, r = exp(pn - po), rc = clamp(r, 1 - clip, 1 + clip),
 *     l = -min(r adv_b, rc adv_b) + beta kl,  dl/dpn = -adv_b r [not (rc adv_b < r adv_b)] - beta (exp(d) - 1);
 *     loss = scale sum_b (sum_s w l / sum_s w)   (scale <= 0: 1/B; a sequence with sum_s w = 0 contributes 0);
 *   out4 = loss, mean_kl, mean_ratio, mean_clipped, the last three sum w x / sum w over all tokens for x = kl, r,
 *   [r > 1 + clip or r < 1 - clip].  One head launch per logits tensor, the token launch (a wave per sequence, fixed-order
 *   sums, no float atomics), a one-workgroup launch that forms the three means.  ws: hpc_rll_grpo_workspace_floats(B,S)
 *   floats, with R = B*S the layout is
 *   lse (R) | coef (R): w scale / (sum_s w) dl/dpn | logp of logit_new, old, ref (R each) | the five sums (8) | partial sums.
 *   B == 0, S == 0 or V == 0 zeroes out4 and launches nothing.
 * hpc_rll_grpo_backward -- one streaming launch: grad_logit[b,s,v] = g coef ([v = a] - exp(x_v - lse)) in logit_new's
 *   element type; g_loss is a device scalar (NULL = 1); a row whose g coef is exactly 0 is zero-filled without reading its
 *   logits (decided on the device).  ws as the forward left it (lse and coef are read).
 * hpc_rll_grpo_last_config -- out[HPC_RLL_GRPO_CONFIG_INTS] = {
 *    [0..6]   the head launch last issued: launches so far, element type, bytes per load of the row's body (16), peeled (1:
 *             the elements outside the row's 16-byte grid are loaded one by one; 0: base and pitch are on 16 bytes),
 *             threads per row (64: a wave per row; 256: a workgroup per row), rows per workgroup, workgroups,
 *    [7..9]   the token launch: launches so far, threads per workgroup, workgroups,
 *    [10..15] the gradient launch: launches so far, element type, bytes per load and store (16, or the element's size when
 *             a base or the pitch is off 16 bytes), threads per row, rows per workgroup, workgroups };
 *   each of the three parts is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * Argument errors of the first four, before any HIP call: HPC_RLL_EINVAL (null operands, then negative sizes or an unknown
 * element type / kind), HPC_RLL_EALIGN (a float array off 4-byte alignment, action off 8, logits off their element size),
 * then HPC_RLL_EUNSUPPORTED (V > 262144); then empty shapes return 0. */
#define HPC_RLL_ELEM_F32 (0)
#define HPC_RLL_ELEM_BF16 (1)
#define HPC_RLL_GRPO_LOGP (2)
#define HPC_RLL_GRPO_CONFIG_INTS (16)
int hpc_rll_token_logp_forward(const void* logits, int elem, const int64_t* action, const float* weight, float* logp,
                               float* lse, int64_t rows, int V, void* stream);
int hpc_rll_token_logp_backward(const float* g_logp, const void* logits, int elem, const int64_t* action, const float* lse,
                                void* grad_logits, int64_t rows, int V, void* stream);
int64_t hpc_rll_grpo_workspace_floats(int B, int S);
int hpc_rll_grpo_forward(const void* logit_new, int elem_new, const void* old, int old_kind, const void* ref, int ref_kind,
                         const int64_t* action, const float* adv, const float* weight, float* out4, float* ws, int B, int S,
                         int V, float clip_ratio, float beta, float scale, void* stream);
int hpc_rll_grpo_backward(const float* g_loss, const void* logit_new, int elem, const int64_t* action, const float* ws,
                          void* grad_logit, int B, int S, int V, void* stream);
int hpc_rll_grpo_last_config(int* out);

/* Token-level PPO for language models (no reference counterpart; the semantics are those of TRL's / OpenRLHF's PPO trainers):
 * the head of hpc_rll_token_logp_forward with the entropy over the vocabulary, GAE on the (B,S) layout under a response mask,
 * and the clipped token loss with value loss and entropy.  Logits, element types, the limit 1 <= V <= 262144, dropped rows
 * (action outside [0,V) or weight 0: not read, every output 0, gradient row exact zeros) and the -inf / NaN clamp are those of
 * the GRPO entry points above.
 * hpc_rll_lm_head_forward -- one launch, one read of every live row.  Every lane keeps an online triple (m, s = sum e^(x-m),
 *   u = sum e^(x-m) (x-m)); lse = m + ln s, logp = x[a] - lse, entropy H = ln s - u/s.  An entry of probability 0 adds exactly 0
 *   to u.  logp, lse, entropy (rows), all required; weight (rows; may be NULL) only selects the rows to drop.
 * hpc_rll_lm_head_backward -- one streaming launch:
 *     grad_logits[r,v] = g_logp[r] ([v = a] - p_v) - g_entropy[r] p_v (x_v - lse[r] + H[r]),   p_v = exp(x_v - lse[r])
 *   in the logits' element type (bf16: round to nearest even), nontemporal stores.  g_logp, g_entropy (rows) may each be NULL
 *   (= zeros).  A row whose two coefficients are exactly 0 is zero-filled without reading its logits (decided on the device).
 * hpc_rll_lm_gae -- value, weight (NULL = ones), kl (NULL = none), adv, ret (B,S); reward (B,S), or (B) with
 *   reward_per_sequence != 0: a terminal score credited to the last live token of the sequence.  A token is live iff w != 0; the
 *   live tokens j_1 < ... < j_L of a sequence are its trajectory, dropped ones are skipped (they may hold NaN; adv = ret = 0):
 *     r_i = reward_i - beta kl_i,  delta_i = r_i + gamma V_(i+1) - V_i,  A_i = delta_i + gamma lam A_(i+1),  V_(L+1) = A_(L+1) = 0,
 *     ret_i = A_i + V_i;   whiten != 0: adv = (A - mu) / sqrt(var + 1e-8), mu and the biased var over the n live tokens of the
 *   batch (Chan's merge of centred sums in a fixed order; n = 0 gives zeros, n = 1 gives adv = 0), else adv = A.
 *   One launch (a wave per sequence, 64 tokens per step), plus one for the whitening, whatever B and S are; no atomics, no host
 *   synchronisation, the same bits on every run.  ws: hpc_rll_lm_gae_workspace_floats() floats; (n, mean, M2) per workgroup of
 *   the first launch are written, nothing else.  B == 0 or S == 0 launches nothing.
 * hpc_rll_lm_ppo_forward -- logit_new (B,S,V) of elem; old_logp, adv, weight (NULL = ones) (B,S) fp32; action (B,S) int64;
 *   value_new, value_old, ret (B,S): all three or all NULL.  Per live token, with pn and H from the head:
 *     r = exp(pn - po), rc = clamp(r, 1 - clip, 1 + clip), l = max(-A r, -A rc); dual_clip = c > 1 and A < 0: l = min(l, -c A);
 *     dl/dpn = -A r where the unclipped term is the maximum (a tie counts as unclipped) and the dual clip is not active, else 0;
 *     lv = max((v - ret)^2, (vc - ret)^2) / 2, vc = v_old + clamp(v - v_old, -value_clip, value_clip)  (use_value_clip == 0:
 *     lv = (v - ret)^2 / 2);  the clipped branch has no gradient.
 *   Aggregation of a per-token x: seq_mean == 0 ('token'): sum w x / sum w over the batch; seq_mean != 0 ('sequence'):
 *     scale sum_b (sum_s w x / sum_s w), scale <= 0: 1/B, a sequence without weight contributes 0.  sum w == 0 gives zeros.
 *   out8 = policy_loss, value_loss, entropy, approx_kl ((r - 1) - log r), mean_ratio, clipfrac ([r outside 1 +- clip]),
 *     den (sum w in 'token' mode, 1 in 'sequence' mode), 0.  raw != 0: the six are left as numerators (not divided by den): a
 *     sharded caller sums numerators and den over the ranks and divides then.
 *   Three launches: the head, the token launch (a wave per sequence, fixed-order sums), a one-workgroup launch for out8.
 *   ws: hpc_rll_lm_ppo_workspace_floats(B,S) floats, with R = B*S the layout is
 *   lse (R) | entropy (R) | cp (R) | ce (R) | cv (R) | logp (R) | the seven sums (8; 7 written) | partial sums (7 per workgroup);
 *   cp, ce, cv are the unit gradients of the three numerators towards logp, entropy and value_new (cv is written only with value
 *   operands).  B == 0, S == 0 or V == 0 zeroes out8 and launches nothing.
 * hpc_rll_lm_ppo_backward -- g_policy, g_entropy, g_value: device scalars, the upstream gradients of the three outputs; NULL
 *   means the output was not differentiated (gradient 0).  use_den != 0 ('token' mode, raw == 0): they are divided by the
 *   sum w the forward left in ws, read on the device.  grad_logit (may be NULL): one streaming launch of the head's gradient
 *   kernel with the per-row coefficients g_policy cp / den and g_entropy ce / den; weight as given to the forward.
 *   grad_value (B,S) (may be NULL) = g_value cv / den, one small launch.
 * hpc_rll_lm_ppo_last_config -- out[HPC_RLL_LM_PPO_CONFIG_INTS] = {
 *    [0..6]   the head launch last issued: launches so far, element type, bytes per load of the row's body (16), peeled (1:
 *             the elements outside the row's 16-byte grid are loaded one by one; 0: base and pitch are on 16 bytes),
 *             threads per row (64: a wave per row; 256: a workgroup per row), rows per workgroup, workgroups,
 *    [7..11]  the GAE launch: launches so far, threads per sequence (64), sequences per workgroup (4), tokens per step (64),
 *             workgroups,
 *    [12..14] the whitening launch: launches so far, threads per workgroup, workgroups,
 *    [15..17] the token launch: launches so far, threads per workgroup, workgroups,
 *    [18..23] the gradient launch: launches so far, element type, bytes per load and store (16, or the element's size when
 *             a base or the pitch is off 16 bytes), threads per row, rows per workgroup, workgroups };
 *   each of the five parts is {0, -1 ...} before its first launch; HPC_RLL_EINVAL for out == NULL.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands, value operands given in part, then negative sizes or an
 * unknown element type), HPC_RLL_EALIGN (a float array off 4-byte alignment, action off 8, logits off their element size),
 * then HPC_RLL_EUNSUPPORTED (V > 262144); then empty shapes return 0. */
#define HPC_RLL_LM_PPO_CONFIG_INTS (24)
int hpc_rll_lm_head_forward(const void* logits, int elem, const int64_t* action, const float* weight, float* logp, float* lse,
                            float* entropy, int64_t rows, int V, void* stream);
int hpc_rll_lm_head_backward(const float* g_logp, const float* g_entropy, const void* logits, int elem, const int64_t* action,
                             const float* weight, const float* lse, const float* entropy, void* grad_logits, int64_t rows,
                             int V, void* stream);
int64_t hpc_rll_lm_gae_workspace_floats(void);
int hpc_rll_lm_gae(const float* value, const float* weight, const float* reward, int reward_per_sequence, const float* kl,
                   float* adv, float* ret, float* ws, int B, int S, float beta, float gamma, float lam, int whiten,
                   void* stream);
int64_t hpc_rll_lm_ppo_workspace_floats(int B, int S);
int hpc_rll_lm_ppo_forward(const void* logit_new, int elem, const float* old_logp, const int64_t* action, const float* adv,
                           const float* weight, const float* value_new, const float* value_old, const float* ret, float* out8,
                           float* ws, int B, int S, int V, float clip_ratio, float dual_clip, int use_value_clip,
                           float value_clip, int seq_mean, int raw, float scale, void* stream);
int hpc_rll_lm_ppo_backward(const float* g_policy, const float* g_entropy, const float* g_value, const void* logit_new,
                            int elem, const int64_t* action, const float* weight, const float* ws, void* grad_logit,
                            float* grad_value, int B, int S, int V, int use_den, void* stream);
int hpc_rll_lm_ppo_last_config(int* out);

/* PPO -- replaces PPOForward/Backward (rl_utils/entry.h:158-165, src/rl_utils/ppo.cu:8-111).
 * logits (B,N), action (B,), value_new/old, adv, ret, weight (B,) (weight NULL = ones).
 * out5 = policy_loss, value_loss, entropy_loss, approx_kl, clipfrac.  dual_clip < 1 disables dual clip
 * (the reference encodes None as 0: hpc_rll/rl_utils/ppo.py:136-137). */
int64_t hpc_rll_ppo_workspace_floats(int B);
int hpc_rll_ppo_forward(const float* logits_new, const float* logits_old, const int64_t* action,
                        const float* value_new, const float* value_old, const float* adv, const float* ret,
                        const float* weight, float* out5, float* ws, int B, int N, float clip_ratio,
                        int use_value_clip, float dual_clip, float scale, void* stream);
int hpc_rll_ppo_backward(const float* g_policy, const float* g_value, const float* g_ent, const float* logits_new,
                         const int64_t* action, const float* ws, float* grad_logits_new, float* grad_value_new,
                         int B, int N, void* stream);

/* PPO for diagonal-Gaussian policies (continuous actions; no reference counterpart, semantics of DI-engine's
 * ppo_error_continuous).  mu_new, sigma_new, mu_old, sigma_old, action (B,A) fp32; value_new/old, adv, ret, weight (B,)
 * (weight NULL = ones).  sigma is the standard deviation and must be > 0 (not checked: device values).  With
 * z = (a - mu)/sigma: logp = sum_j [-z_j^2/2 - log sigma_j - log(2 pi)/2], H = sum_j [1/2 + log(2 pi)/2 + log sigma_new_j],
 * ratio = exp(logp_new - logp_old); from there on, and out5 / dual_clip / scale, exactly hpc_rll_ppo_forward.
 * ws: hpc_rll_ppo_continuous_workspace_floats(B) floats (3 per sample + the partial sums; nothing of size B*A is saved).
 * backward: g_* device scalars (NULL = 1); grad_mu, grad_sigma (B,A) and grad_value (B,) may each be NULL (not wanted):
 *   grad_mu = k1 z/sigma, grad_sigma = (k1 (z^2 - 1) + k2)/sigma, k1 = g_policy*ws[b], k2 = g_ent*ws[B+b],
 *   grad_value = g_value*ws[2B+b].  One launch each way; 1 <= A <= 1024, beyond that HPC_RLL_EUNSUPPORTED.
 * B == 0: out5 = 0, nothing launched.  Null pointers / negative sizes: HPC_RLL_EINVAL before any HIP call. */
int64_t hpc_rll_ppo_continuous_workspace_floats(int B);
int hpc_rll_ppo_continuous_forward(const float* mu_new, const float* sigma_new, const float* mu_old,
                                   const float* sigma_old, const float* action, const float* value_new,
                                   const float* value_old, const float* adv, const float* ret, const float* weight,
                                   float* out5, float* ws, int B, int A, float clip_ratio, int use_value_clip,
                                   float dual_clip, float scale, void* stream);
int hpc_rll_ppo_continuous_backward(const float* g_policy, const float* g_value, const float* g_ent, const float* mu_new,
                                    const float* sigma_new, const float* action, const float* ws, float* grad_mu,
                                    float* grad_sigma, float* grad_value, int B, int A, void* stream);

/* Gaussian heads and V-trace for diagonal-Gaussian policies (continuous actions; no reference counterpart, semantics of
 * DI-engine's vtrace_error_continuous_action).  sigma is the standard deviation and must be > 0 (not checked: device values);
 * 1 <= A <= 1024, beyond that HPC_RLL_EUNSUPPORTED.
 * hpc_rll_gaussian_forward -- the head alone for a PAIR of policies over one action, the analogue of
 *   hpc_rll_categorical_forward: mu, sigma (the policy whose logp and entropy are wanted), mu_b, sigma_b (the other policy),
 *   action (rows,A) fp32 -> logp, entropy, logp_b (rows,), all eight pointers required.  With z = (a - mu)/sigma:
 *     logp = sum_j [-z_j^2/2 - log sigma_j] - A log(2 pi)/2,   entropy = A (1/2 + log(2 pi)/2) + sum_j log sigma_j,
 *     logp_b = logp - d,   d = sum_j [(z_b,j - z_j)(z_b,j + z_j)/2 + (log sigma_b,j - log sigma_j)]
 *   so that logp - logp_b recovers the log ratio d to within half an ulp of logp (|logp| ~ 1.4 A) instead of subtracting two
 *   independently rounded sums of size ~A; identical policies give logp_b == logp bit for bit.  rows == 0: OK, nothing launched.
 * hpc_rll_vtrace_continuous_forward -- that head over T*B rows into the workspace, then the scan of
 *   hpc_rll_vtrace_masked_forward: masks, mask_dtype, the two value forms, the formulas, losses (3,), the workspace
 *   (hpc_rll_vtrace_workspace_floats(T,B), layout coef_pg | coef_ent | gv_unit | logp_t | ent | d | partials) and the
 *   dispatch record (HPC_RLL_SCAN_OP_VTRACE_MASKED) are that entry point's.  One difference: the head hands the scan the log
 *   ratio d itself (the slot that holds logp_b for the categorical op) and the scan forms IS = exp(d): logp is of size ~1.4 A,
 *   and a logp_b rounded to fp32 would give d back only to half an ulp of logp (6e-5 at A = 1024), an error the policy loss
 *   would carry whatever T*B is.  T == 0 or B == 0 zeroes losses.
 * hpc_rll_vtrace_continuous_backward -- g_* device scalars (NULL = 1); grad_mu, grad_sigma (T,B,A) and grad_value may each be
 *   NULL (not wanted): grad_mu = k1 z/sigma, grad_sigma = (k1 (z^2 - 1) + k2)/sigma, k1 = g_pg*ws[i], k2 = g_ent*ws[T*B + i].
 *   grad_value is the STACKED form's (T+1,B) = g_value*ws[2*T*B + i] with the bootstrap row zeroed; in the next-value form
 *   pass grad_value = NULL and call hpc_rll_scale_rows(g_value, ws + 2*T*B, grad_value, T*B, T*B), as for
 *   hpc_rll_vtrace_masked_forward.  Nothing flows to the behaviour policy or the action.
 * Argument errors, before any HIP call: HPC_RLL_EINVAL (null operands, negative sizes, A <= 0, bad mask_dtype), HPC_RLL_EALIGN
 * (a pointer off 4-byte alignment), then HPC_RLL_EUNSUPPORTED (A > 1024). */
int hpc_rll_gaussian_forward(const float* mu, const float* sigma, const float* mu_b, const float* sigma_b,
                             const float* action, float* logp, float* entropy, float* logp_b,
                             int64_t rows, int A, void* stream);
int hpc_rll_vtrace_continuous_forward(const float* mu_target, const float* sigma_target, const float* mu_behaviour,
                                      const float* sigma_behaviour, const float* action, const float* value,
                                      const float* next_value, const float* reward, const float* weight,
                                      const void* done, const void* traj_flag, int mask_dtype, float* losses, float* ws,
                                      int T, int B, int A, float gamma, float lambda, float rho_clip, float c_clip,
                                      float rho_pg_clip, float scale, void* stream);
int hpc_rll_vtrace_continuous_backward(const float* g_pg, const float* g_value, const float* g_ent,
                                       const float* mu_target, const float* sigma_target, const float* action,
                                       const float* ws, float* grad_mu, float* grad_sigma, float* grad_value,
                                       int T, int B, int A, void* stream);

/* q n-step TD (rescale=0)/ with value rescaling (rescale=1) -- replaces QNStepTd{,Rescale}Forward/Backward
 * (rl_utils/entry.h:89-109).  q,next_n_q (B,N); action,next_n_action (B,) int64; reward (nstep,B); done,
 * weight (B,) float (weight NULL = ones).  loss (1,), td_err (B,), grad_buf (B,). */
int hpc_rll_q_nstep_td_forward(const float* q, const float* next_n_q, const int64_t* action,
                               const int64_t* next_n_action, const float* reward, const float* done,
                               const float* weight, float* loss, float* td_err, float* grad_buf, float* partials,
                               int nstep, int B, int N, float gamma, int rescale, float scale, void* stream);
int hpc_rll_q_nstep_td_backward(const float* grad_loss, const float* grad_buf, const int64_t* action, float* grad_q,
                                int B, int N, void* stream);

/* dist (C51) n-step TD -- replaces DistNStepTdForward/Backward (rl_utils/entry.h:79-87).
 * dist,next_n_dist (B,N,n_atom); buf (B,n_atom) = unit gradient wrt dist[b,a_b,:]. */
int hpc_rll_dist_nstep_td_forward(const float* dist, const float* next_n_dist, const int64_t* action,
                                  const int64_t* next_n_action, const float* reward, const float* done,
                                  const float* weight, float* loss, float* td_err, float* buf, float* partials,
                                  int nstep, int B, int N, int n_atom, float gamma, float v_min, float v_max,
                                  float scale, void* stream);
int hpc_rll_dist_nstep_td_backward(const float* grad_loss, const float* buf, const int64_t* action,
                                   float* grad_dist, int B, int N, int n_atom, void* stream);

/* IQN n-step TD -- replaces IQNNStepTDErrorForward/Backward (rl_utils/entry.h:111-119).
 * q (tau,B,N), next_n_q (tau',B,N), replay_quantiles (tau,B), value_gamma (B,) or NULL (= gamma^nstep);
 * buf (B,tau) = unit gradient wrt q[:,b,a_b]. */
int hpc_rll_iqn_nstep_td_forward(const float* q, const float* next_n_q, const int64_t* action,
                                 const int64_t* next_n_action, const float* reward, const float* done,
                                 const float* replay_quantiles, const float* weight, const float* value_gamma,
                                 float* loss, float* td_err, float* buf, float* partials, int tau, int tau_prime,
                                 int nstep, int B, int N, float gamma, float kappa, float scale, void* stream);
int hpc_rll_iqn_nstep_td_backward(const float* grad_loss, const float* buf, const int64_t* action, float* grad_q,
                                  int tau, int B, int N, void* stream);
/* ABI 6 (not in the reference): the same loss with the quantile axis INNERMOST -- q (B,N,tau), next_n_q (B,N,tau'), grad_q
 * (B,N,tau), the layout of the QR-DQN op (rl_utils/entry.h:121-129); replay_quantiles stays (tau,B), buf (B,tau).  A sample's
 * quantiles are one contiguous row instead of tau values a (B,N) plane apart: 2 cache lines per sample instead of 2 tau
 * (iqn_nstep_td_error_kernel.h:11-70 reads the (tau,B,N) layout). */
int hpc_rll_iqn_nstep_td_forward_bnt(const float* q, const float* next_n_q, const int64_t* action,
                                     const int64_t* next_n_action, const float* reward, const float* done,
                                     const float* replay_quantiles, const float* weight, const float* value_gamma,
                                     float* loss, float* td_err, float* buf, float* partials, int tau, int tau_prime,
                                     int nstep, int B, int N, float gamma, float kappa, float scale, void* stream);
int hpc_rll_iqn_nstep_td_backward_bnt(const float* grad_loss, const float* buf, const int64_t* action, float* grad_q,
                                      int tau, int B, int N, void* stream);

/* QR-DQN n-step TD -- replaces QRDQNNStepTDErrorForward/Backward (rl_utils/entry.h:121-129).
 * q,next_n_q (B,N,tau); tau_value = the `tau` the caller passes to the oracle (the reference kernel hard
 * codes the integer count, qrdqn_nstep_td_error_kernel.h:60); buf (B,tau). */
int hpc_rll_qrdqn_nstep_td_forward(const float* q, const float* next_n_q, const int64_t* action,
                                   const int64_t* next_n_action, const float* reward, const float* done,
                                   const float* weight, const float* value_gamma, float* loss, float* td_err,
                                   float* buf, float* partials, int tau, int nstep, int B, int N, float gamma,
                                   float tau_value, float scale, void* stream);
int hpc_rll_qrdqn_nstep_td_backward(const float* grad_loss, const float* buf, const int64_t* action, float* grad_q,
                                    int tau, int B, int N, void* stream);
/* Diagnostic (no reference counterpart; read-only, modelled on hpc_rll_categorical_last_config / hpc_rll_r2d2_last_config): which
 * forward kernel the most recent launch of hpc_rll_dist_nstep_td_forward (op HPC_RLL_DIST_OP_C51), of
 * hpc_rll_iqn_nstep_td_forward / _forward_bnt (HPC_RLL_DIST_OP_IQN) or of hpc_rll_qrdqn_nstep_td_forward
 * (HPC_RLL_DIST_OP_QRDQN) ran in this process, recorded on the host where the kernel is launched.  Each op keeps its own
 * record.  out[HPC_RLL_DIST_CONFIG_INTS] = {
 *    [0] forward launches of this op so far (0 = no launch yet: every other entry is then -1),
 *    [1] kernel family, one of HPC_RLL_DIST_FAMILY_*,
 *    [2] G: lanes that hold one sample -- 8 / 16 / 32 / 64 for GROUP, BATCH and QUAD of IQN / QR-DQN (QUAD: 8 or 16, four
 *        quantiles per lane), 64 for every kernel that gives a sample the whole wave (WAVE, and all three C51 families),
 *    [3] SW: consecutive samples a wave walks, 8 / 16 / 32 / 64 for BATCH and QUAD (tune key 24, or by batch size); 0 for the
 *        families without that loop,
 *    [4] FULL: 1 = the instantiation without a tail (QR-DQN BATCH: tau == G, QUAD: tau == 4 G), else 0,
 *    [5] layout: 1 = quantile axis innermost (hpc_rll_iqn_nstep_td_forward_bnt), 0 otherwise,
 *    [6] workgroups of the launch,
 *    [7] 1 = the loss was finalised inside the launch (the fold of tune key 21), 0 = by a separate finalize launch }.
 * Calls that return before launching (B == 0, argument errors) leave the record as it was; the backward entry points keep
 * no record.  Plain ints of the host process, not synchronised.  HPC_RLL_EINVAL for an op outside the three or out == NULL. */
#define HPC_RLL_DIST_OP_C51 (0)
#define HPC_RLL_DIST_OP_IQN (1)
#define HPC_RLL_DIST_OP_QRDQN (2)
#define HPC_RLL_DIST_OPS (3)
#define HPC_RLL_DIST_FAMILY_WAVE (0)      /* IQN, QR-DQN: a wave per sample, any tau (the only kernels for tau or tau' > 64) */
#define HPC_RLL_DIST_FAMILY_GROUP (1)     /* IQN, QR-DQN: a sample per group of G lanes, 64 / G samples per wave */
#define HPC_RLL_DIST_FAMILY_BATCH (2)     /* C51 (n_atom <= 64), QR-DQN: SW consecutive samples per wave */
#define HPC_RLL_DIST_FAMILY_QUAD (3)      /* QR-DQN: BATCH with four quantiles per lane (tau % 4 == 0, tau >= 8, 16-byte aligned rows) */
#define HPC_RLL_DIST_FAMILY_WAVE64 (4)    /* C51, n_atom <= 64: a wave per sample, sources gathered in source order */
#define HPC_RLL_DIST_FAMILY_GENERAL (5)   /* C51, n_atom > 64: a wave per sample, every target walks every source */
#define HPC_RLL_DIST_CONFIG_INTS (8)
int hpc_rll_dist_last_config(int op, int* out);

/* ------------------------------------------------------------------------------------------
 * FQF (Fully parameterized Quantile Function, Yang et al. 2019) -- no reference counterpart; the formulas restate DI-engine's
 * fqf_nstep_td_error / fqf_calculate_fraction_loss (ding/rl_utils/td.py) and the fraction proposal of its FQFHead.
 * K fractions, N actions, B samples; fp32 contiguous, actions int64.  Every entry point answers argument errors before any HIP
 * call, in this order: HPC_RLL_EINVAL (sizes, then null pointers), HPC_RLL_EALIGN (a float pointer off 4 bytes, an action
 * pointer off 8), HPC_RLL_EUNSUPPORTED; then an empty batch (B == 0) clears `loss` where there is one and returns 0.  An
 * action outside [0, N) never addresses memory: the value it would select reads as 0 and its gradient row is zero.
 *
 *   fractions  : logits (B,K) -> quantiles (B,K+1) = {0, inclusive scan of softmax}, quantiles_hats (B,K) = midpoints,
 *                entropies (B,) = -sum p log p.  1 <= K <= 1024.  backward: grad_quantiles (B,K+1) and grad_entropies (B,) may
 *                each be NULL (= zero); `entropies` is the forward's output.
 *   nstep_td   : q (B,K,N), next_n_q (B,K',N), reward (nstep,B), done (B,), quantiles_hats (B,K), weight / value_gamma (B,) or
 *                NULL.  loss (1,) = scale * sum_b weight_b td_err_b, td_err (B,), buf (B,K) = unit gradient wrt q[b,:,a_b];
 *                partials: hpc_rll_partials_floats(B) floats.  backward: grad_q (B,K,N), rows one-hot at action[b]; B * K < 2^31, else
 *                HPC_RLL_EUNSUPPORTED.
 *   fraction_loss : q_tau_i (B,K-1,N), q_value (B,K,N), quantiles (B,K+1).  loss (1,) = scale * sum_b sum_i g_i quantiles[b,i+1],
 *                g (B,K-1) (K == 1: empty, q_tau_i and g may be NULL, the loss is 0).  backward: grad_quantiles (B,K+1) =
 *                grad_loss * scale * g in columns 1..K-1, zero in columns 0 and K.
 *   q_value    : logit (B,N) = sum_i (quantiles[b,i+1] - quantiles[b,i]) q[b,i,:]; action (B,) int64 = argmax_n, ties to the
 *                lowest index, in the same launch; NULL: no argmax. */
int hpc_rll_fqf_fractions_forward(const float* logits, float* quantiles, float* quantiles_hats, float* entropies, int B,
                                  int K, void* stream);
int hpc_rll_fqf_fractions_backward(const float* logits, const float* entropies, const float* grad_quantiles,
                                   const float* grad_entropies, float* grad_logits, int B, int K, void* stream);
int hpc_rll_fqf_nstep_td_forward(const float* q, const float* next_n_q, const int64_t* action,
                                 const int64_t* next_n_action, const float* reward, const float* done,
                                 const float* quantiles_hats, const float* weight, const float* value_gamma, float* loss,
                                 float* td_err, float* buf, float* partials, int K, int K_prime, int nstep, int B, int N,
                                 float gamma, float kappa, float scale, void* stream);
int hpc_rll_fqf_nstep_td_backward(const float* grad_loss, const float* buf, const int64_t* action, float* grad_q, int K,
                                  int B, int N, void* stream);
int hpc_rll_fqf_fraction_loss_forward(const float* q_tau_i, const float* q_value, const float* quantiles,
                                      const int64_t* action, float* loss, float* g, float* partials, int K, int B, int N,
                                      float scale, void* stream);
int hpc_rll_fqf_fraction_loss_backward(const float* grad_loss, const float* g, float* grad_quantiles, int K, int B,
                                       float scale, void* stream);
int hpc_rll_fqf_q_value(const float* q, const float* quantiles, float* logit, int64_t* action, int B, int K, int N,
                        void* stream);
/* Diagnostic (read-only, modelled on hpc_rll_dist_last_config): the instantiation the most recent launch of each KIND ran in
 * this process, noted on the host beside the launch.  out[HPC_RLL_FQF_CONFIG_INTS] holds HPC_RLL_FQF_LAUNCHES parts of
 * HPC_RLL_FQF_PART_INTS ints, part k (HPC_RLL_FQF_LAUNCH_*) = {
 *    [0] launches of this kind so far (0 = none yet: every other entry of the part is then -1),
 *    [1] kernel family, one of HPC_RLL_FQF_FAMILY_*,
 *    [2] G: lanes that hold one sample or row (8 / 16 / 32 / 64; 64 for WAVE), 0 for the elementwise streaming kernels,
 *    [3] workgroups of the launch,
 *    [4] 1 = the loss was finalised inside the launch, 0 = by a separate finalize launch or the kind has no loss,
 *    [5] floats per load / store of the streamed operand (4 = 16 bytes, 1 = scalar) }.
 * Calls that return before launching leave the record as it was.  HPC_RLL_EINVAL for out == NULL. */
#define HPC_RLL_FQF_LAUNCH_TD_FORWARD (0)
#define HPC_RLL_FQF_LAUNCH_TD_BACKWARD (1)
#define HPC_RLL_FQF_LAUNCH_FRACTION_LOSS_FORWARD (2)
#define HPC_RLL_FQF_LAUNCH_FRACTION_LOSS_BACKWARD (3)
#define HPC_RLL_FQF_LAUNCH_FRACTIONS_FORWARD (4)
#define HPC_RLL_FQF_LAUNCH_FRACTIONS_BACKWARD (5)
#define HPC_RLL_FQF_LAUNCH_Q_VALUE (6)
#define HPC_RLL_FQF_LAUNCHES (7)
#define HPC_RLL_FQF_FAMILY_WAVE (0)            /* a wave per sample / row: TD loss and fraction loss above 64 fractions, fractions for 64 < K <= 1024 */
#define HPC_RLL_FQF_FAMILY_GROUP (1)           /* a sample / row per group of G lanes, 64 / G per wave */
#define HPC_RLL_FQF_FAMILY_STREAM (2)          /* streaming: TD backward, fraction-loss backward, q_value without argmax */
#define HPC_RLL_FQF_FAMILY_STREAM_ARGMAX (3)   /* q_value with the greedy action in the same launch */
#define HPC_RLL_FQF_PART_INTS (6)
#define HPC_RLL_FQF_CONFIG_INTS (42)
int hpc_rll_fqf_last_config(int* out);

/* ------------------------------------------------------------------------------------------
 * Pad / Unpad of a ragged list of n contiguous fp32 tensors of rank 1..3 -- replaces Pad{1,2,3}DForward,
 * GroupPad{1,2,3}DForward, Unpad{1,2,3}DForward (rl_utils/entry.h:10-59, src/rl_utils/padding.cu:111-582).
 * A rank-1 tensor of length L is described as (d0,d1,d2) = (1,1,L), rank-2 (a,b) as (1,a,b).
 *   pad  : table (device, n x 4 int64) = {source pointer, d0, d1, d2}; new_x (n,m0,m1,m2) fp32 gets the
 *          data and `value` elsewhere; mask (same shape, int32) gets 1 inside and `value` outside.
 *   unpad: table (device, n x 4 int64) = {offset of tensor i in `flat` (elements), d0, d1, d2}, offsets
 *          ascending; flat (total floats) receives the tensors back to back.
 * Group padding = one pad call per group (the grouping policy is host logic, below).
 * ------------------------------------------------------------------------------------------ */
int hpc_rll_pad_forward(const int64_t* table, float* new_x, int32_t* mask, int64_t n, int m0, int m1, int m2,
                        int value, void* stream);
int hpc_rll_unpad_forward(const float* padded, const int64_t* table, float* flat, int64_t n, int64_t total,
                          int m0, int m1, int m2, void* stream);
/* Packed (CSR-style) ragged input: lengths (n,) int64 on the device -> the (n,4) table the two kernels above take,
 * row i = {base + stride * sum(lengths[:i]), 1, 1, lengths[i]} (pad: base = address of the flat buffer, stride = 4;
 * unpad: base = 0, stride = 1).  A device-side exclusive scan: no host loop, no synchronisation.
 * scratch: hpc_rll_packed_table_scratch_int64(n) int64. */
int64_t hpc_rll_packed_table_scratch_int64(int64_t n);
int hpc_rll_packed_table(const int64_t* lengths, int64_t n, int64_t base, int64_t stride, int64_t* table,
                         int64_t* scratch, void* stream);
/* Pad1DForward / Unpad1DForward (src/rl_utils/padding.cu:111-140, 228-260; kernels padding_kernel.h:92-127) for PACKED
 * rows: the two directions with the rows' contiguity exploited (a workgroup's rows are ONE span of the flat buffer,
 * staged through LDS with 16-byte accesses).  `table` as built by hpc_rll_packed_table: pad -- base = address of `flat`,
 * stride 4; unpad -- base 0, stride 1.  Same results as hpc_rll_pad_forward / hpc_rll_unpad_forward with m0 = m1 = 1
 * (to which they hand over when a pointer is not aligned for 16-byte accesses, or when max_len > 15200 so that not even one
 * row fits the workgroup kernels' 60 KB of LDS -- except that the pad's wave kernel, tune key 28 = 1, needs no such room and
 * takes every 32 <= max_len <= 16384). */
int hpc_rll_pad1d_packed_forward(const float* flat, const int64_t* table, float* new_x, int32_t* mask, int64_t n,
                                 int max_len, int value, void* stream);
int hpc_rll_unpad1d_packed_forward(const float* padded, const int64_t* table, float* flat, int64_t n, int64_t total,
                                   int max_len, void* stream);
/* Group-split policies over a list sorted by numel (host code; padding.cu:8-108).  sizes: n x dim int32.
 * Write <= `group` rows of `dim` ints to group_shapes and <= group+1 boundaries to positions; return the
 * number of groups (>= 1) or a negative HPC_RLL_E* code.  oracle = the O(group * n^2) DP minimising padded
 * elements (ties -> smallest split point); sample = random cuts (deterministic for a given seed). */
int hpc_rll_oracle_split_group(const int32_t* sizes, int n, int dim, int group, int32_t* group_shapes,
                               int32_t* positions);
int hpc_rll_sample_split_group(const int32_t* sizes, int n, int dim, int group, uint64_t seed,
                               int32_t* group_shapes, int32_t* positions);
/* Grouped padding of PACKED 1-D rows entirely on the device (what hpc_rll/rl_utils/padding.py:20-45 does on the host
 * with a python sorted() + the split policies above + one pad per group; SURVEY.md 8f-3: ~1M rows at configs[4]).
 * lengths (n,) int64 on the device, every length in [0, max_len], max_len <= 16384, group <= 63.
 *   plan  : histogram of the lengths -> runs of equal lengths -> the split policy on the runs (mode 0 = oracle: the same
 *           cuts as hpc_rll_oracle_split_group incl. its tie rule; mode 1 = sample with `seed`) -> `plan`, 3*group+4
 *           int64 on the device: [0] number of groups ng, [1] status (1 = a length was outside [0,max_len] and clamped),
 *           [2 .. 2+group] cut positions in sorted order, [3+group .. 3+2*group) group widths,
 *           [3+2*group .. 4+3*group) offsets of the groups in the concatenated output (ng+1 used);
 *           and a STABLE radix sort of (length, row) -> order (n,) int64: order[p] = original row of sorted position p
 *           (ascending length, original order among equal lengths = python's sorted()).
 *           ws: hpc_rll_pad1d_group_workspace_int64(n, max_len, group) int64.  No host synchronisation.
 *           Cost of the plan step: the histogram and the sort stream `lengths` (HBM-bound); the oracle policy
 *           itself is a DP over the D <= max_len+1 DISTINCT lengths that runs in ONE workgroup, group * D^2 / 1024 steps of
 *           ~10 ns: microseconds at configs[4] (D <= 96: len ~ U[32,128)), ~2 ms at D = 4096 with group = 8, ~0.25 s at the
 *           limits D = 16385, group = 63 -- there the host's divide-and-conquer DP (hpc_rll_oracle_split_group on the
 *           histogram's runs) is the faster route; the prefix scan of the sort is single-workgroup too: n <= 2^28.
 *   forward: all groups in ONE launch.  table = hpc_rll_packed_table rows of the ORIGINAL order; out / mask hold the
 *           groups back to back (group g: (cuts[g+1]-cuts[g]) rows of width[g] at offset[g]); total_out = offset[ng]. */
int64_t hpc_rll_pad1d_group_workspace_int64(int64_t n, int max_len, int group);
int hpc_rll_pad1d_group_plan(const int64_t* lengths, int64_t n, int max_len, int group, int mode, uint64_t seed,
                             int64_t* ws, int64_t* plan, int64_t* order, void* stream);
int hpc_rll_pad1d_group_forward(const int64_t* table, const int64_t* order, const int64_t* plan, int group, float* out,
                                int32_t* mask, int64_t total_out, int value, void* stream);

/* ScatterConnection -- replaces ScatterConnectionForward/Backward (torch_utils/network/entry.h:21-29,
 * src/torch_utils/network/scatter_connection.cu:8-73).  x (B,M,N) fp32, location (B,M,2) int64 (y,x),
 * out (B,N,H,W) fp32 (fully written: no pre-zeroing needed); add=0: "cover" (the largest m at a cell wins,
 * like the CPU oracle), add=1: sum in ascending m.  ws: hpc_rll_scatter_workspace_ints(B,M,H,W) int32 of scratch
 * (contents unspecified afterwards; untouched where the output kernel builds its tables in LDS, tune key 37).
 * backward: grad_x[b,m,:] = grad_out[b,:,y,x] for every entity (also the covered ones). */
int64_t hpc_rll_scatter_workspace_ints(int B, int M, int H, int W);
int hpc_rll_scatter_connection_forward(const float* x, const int64_t* location, float* out, int32_t* ws, int B,
                                       int M, int N, int H, int W, int add, void* stream);
int hpc_rll_scatter_connection_backward(const float* grad_out, const int64_t* location, float* grad_x, int B, int M,
                                        int N, int H, int W, void* stream);
/* Diagnostic (no reference counterpart; read-only, modelled on hpc_rll_dist_last_config / hpc_rll_per_last_config): which
 * kernel the most recent launching call of hpc_rll_pad_forward (op HPC_RLL_PADSC_OP_PAD), hpc_rll_unpad_forward (_UNPAD),
 * hpc_rll_pad1d_packed_forward (_PAD_PACKED), hpc_rll_unpad1d_packed_forward (_UNPAD_PACKED),
 * hpc_rll_scatter_connection_forward (_SCATTER_FWD) or hpc_rll_scatter_connection_backward (_SCATTER_BWD) ran in this
 * process, noted on the host beside the launch with the values of that launch.  Each op keeps its own record.
 * out[HPC_RLL_PAD_SCATTER_CONFIG_INTS] = {
 *    [0] calls of this op that launched so far (0 = none yet: every other entry is then -1),
 *    [1] the kernel, one of HPC_RLL_PADSC_KERNEL_*,
 *    [2] grid.x, [3] grid.y * grid.z, [4] threads per workgroup, [5] dynamic LDS bytes of that launch (all 0 for _HANDED_OVER
 *        and _SCATTER_BWD_MEMSET; the scatter forward's index launch, where there is one, is one workgroup of 256 threads per
 *        batch element and shows in the flags only),
 *    [6], [7] by op:
 *        PAD, UNPAD          [6] output (pad) / padded (unpad) elements per thread step: 4 for the 16-byte kernels, 1 for the
 *                                element-wise ones,  [7] 1 = called as the hand-over target of the packed entry point, else 0
 *        PAD_PACKED,         [6] RB, the rows per workgroup that 60 KB of LDS hold: min(16, (15360 - 160) / max_len), 0 above
 *        UNPAD_PACKED            max_len = 15200 (the wave kernel does not use it),  [7] 1 = handed over to the list entry point
 *                                (kernel = _HANDED_OVER; the PAD / UNPAD record then names the kernel that ran), else 0
 *        SCATTER_FWD         [6] channels per workgroup (npb of the LDS-staged kernel, n_per_block of the other two),
 *                            [7] flags: bit 0 add, bit 1 owner table built inside the kernel (tune key 37), bits 2-3 the `parts`
 *                                of the index launch before it (0 = no index launch, 1 = head + next, 2 = last, 3 = all three),
 *                                bit 4 vec: x is read 16 bytes at a time (N % 4 == 0 and x 16-byte aligned; LDS-staged kernel:
 *                                and npb % 4 == 0), else element-wise
 *        SCATTER_BWD         [6] NG, the planes per workgroup (_SCATTER_BWD_LDS), TR, the map rows per tile (_TILE), else 0,
 *                            [7] the XCD order of the launch: 0 launch order, 1 XCD-major, 2 neighbouring batch elements }.
 * A packed call that hands over notes BOTH records.  Calls that return before launching (empty shapes, argument errors) leave
 * every record as it was.  Plain ints of the host process, not synchronised.  HPC_RLL_EINVAL for an op outside the six or
 * out == NULL (nothing written). */
#define HPC_RLL_PADSC_OP_PAD (0)
#define HPC_RLL_PADSC_OP_UNPAD (1)
#define HPC_RLL_PADSC_OP_PAD_PACKED (2)
#define HPC_RLL_PADSC_OP_UNPAD_PACKED (3)
#define HPC_RLL_PADSC_OP_SCATTER_FWD (4)
#define HPC_RLL_PADSC_OP_SCATTER_BWD (5)
#define HPC_RLL_PADSC_OPS (6)
#define HPC_RLL_PADSC_KERNEL_PAD (0)                 /* pad_kernel: one output element per thread, any rank, any alignment */
#define HPC_RLL_PADSC_KERNEL_PAD4 (1)                /* pad4_kernel: four per thread (total % 4 == 0, new_x and mask 16-byte aligned) */
#define HPC_RLL_PADSC_KERNEL_PAD1D4 (2)              /* pad1d4_kernel: pad4 for m0 = m1 = 1 and total < 2^32 */
#define HPC_RLL_PADSC_KERNEL_UNPAD (3)               /* unpad_kernel: one flat element per thread, binary search for its tensor */
#define HPC_RLL_PADSC_KERNEL_UNPAD1D4 (4)            /* unpad1d4_kernel: a quad of the padded tensor per thread (m0 = m1 = 1, n * m2 % 4 == 0, < 2^32, padded aligned) */
#define HPC_RLL_PADSC_KERNEL_PAD1D_PACKED (5)        /* pad1d_packed_kernel: RB rows per workgroup through LDS */
#define HPC_RLL_PADSC_KERNEL_PAD1D_PACKED_WAVE (6)   /* pad1d_packed_wave_kernel: 1024 output elements per wave (32 <= max_len <= 16384, key 28) */
#define HPC_RLL_PADSC_KERNEL_UNPAD1D_PACKED (7)      /* unpad1d_packed_kernel: RB rows per workgroup through LDS */
#define HPC_RLL_PADSC_KERNEL_HANDED_OVER (8)         /* a packed entry point that called the list entry point instead */
#define HPC_RLL_PADSC_KERNEL_SCATTER_OUT (9)         /* scatter_out_kernel<ADD>: a cell per thread behind the index launch */
#define HPC_RLL_PADSC_KERNEL_SCATTER_OUT4 (10)       /* scatter_out4_kernel<ADD>: four cells x four channels per step behind the index launch */
#define HPC_RLL_PADSC_KERNEL_SCATTER_OUT_LDS (11)    /* scatter_out_lds_kernel<ADD, BUILD>: the LDS-staged streaming kernel */
#define HPC_RLL_PADSC_KERNEL_SCATTER_BWD_LDS (12)    /* scatter_bwd_lds_kernel: whole planes of grad_out staged per workgroup */
#define HPC_RLL_PADSC_KERNEL_SCATTER_BWD_TILE (13)   /* scatter_bwd_tile_kernel: map rows of all channels staged per workgroup (key 40) */
#define HPC_RLL_PADSC_KERNEL_SCATTER_BWD_DIRECT (14) /* scatter_bwd_direct_kernel: planes above 128 KB, gathered from memory */
#define HPC_RLL_PADSC_KERNEL_SCATTER_BWD_MEMSET (15) /* H * W == 0: grad_x is cleared by a memset, no kernel */
#define HPC_RLL_PADSC_KERNELS (16)
#define HPC_RLL_PAD_SCATTER_CONFIG_INTS (8)
int hpc_rll_pad_scatter_last_config(int op, int* out);

/* ------------------------------------------------------------------------------------------
 * LayerNorm-LSTM -- replaces LstmForward/LstmBackward (torch_utils/network/entry.h:11-19,
 * src/torch_utils/network/lstm.cu:29-379).  x (S,B,I); h0,c0 (L,B,H); wx = concat_l row-major [in_l,4H]
 * (in_0 = I, in_l = H); wh = L x [H,4H]; bias (L,4H); ln_gamma/ln_beta (L, 2*4H) = [x-half | h-half];
 * gate order i,f,o,u.  Outputs y (S,B,H), hn,cn (L,B,H).  ws: hpc_rll_lstm_workspace_floats(...) floats,
 * must be kept (unmodified) from forward to backward.  All GEMMs are exact fp32 on the matrix cores.
 * dropout_p in [0,1): inter-layer dropout, mask = stateless hash of (seed, layer, element).
 * backward: dy (S,B,H), dhn, dcn (L,B,H) may each be NULL (= zero).  Unlike the reference, gradients
 * flowing in through hn / cn are honoured.  dx may be NULL when the gradient of x is not needed: the
 * S*B x I x 4H input-gradient product of layer 0 is then skipped.
 * ------------------------------------------------------------------------------------------ */
int64_t hpc_rll_lstm_workspace_floats(int S, int B, int I, int H, int L, float dropout_p);
/* Float offset of the last layer's h sequence inside ws.  It IS y (the reference keeps it the same way: ym[L-1],
 * rnn.py:27-31): a forward called with y = ws + offset writes y in place and skips the (S,B,H) copy; any other y is
 * filled by a copy as before.  -1 on invalid arguments. */
int64_t hpc_rll_lstm_workspace_y_offset(int S, int B, int I, int H, int L, float dropout_p);
int hpc_rll_lstm_forward(const float* x, const float* h0, const float* c0, const float* wx, const float* wh,
                         const float* bias, const float* ln_gamma, const float* ln_beta, float* y, float* hn,
                         float* cn, float* ws, int S, int B, int I, int H, int L, float dropout_p, uint64_t seed,
                         void* stream);
int hpc_rll_lstm_backward(const float* dy, const float* dhn, const float* dcn, const float* x, const float* h0,
                          const float* c0, const float* wx, const float* wh, const float* ln_gamma, float* ws,
                          float* dx, float* dh0, float* dc0, float* dwx, float* dwh, float* dbias, float* dln_gamma,
                          float* dln_beta, int S, int B, int I, int H, int L, float dropout_p, uint64_t seed,
                          void* stream);
/* ABI 4: the pair a framework binding uses.  y is the caller's own (S,B,H) tensor AND the last layer's saved h sequence
 * (the reference keeps the same array in both roles: ym[L-1], rnn.py:27-31, read again by LstmBackward lstm.cu:352-370):
 * the forward's cells write y directly -- no (S,B,H) copy and no view of the workspace handed out, so a holder of y pins
 * S*B*H floats, not the workspace -- and the SAME y is passed to the backward, which reads the sequence from it.  y must
 * not be modified in between (the binding's job to detect; torch's saved-tensor version counter does). */
int hpc_rll_lstm_forward_y(const float* x, const float* h0, const float* c0, const float* wx, const float* wh,
                           const float* bias, const float* ln_gamma, const float* ln_beta, float* y, float* hn,
                           float* cn, float* ws, int S, int B, int I, int H, int L, float dropout_p, uint64_t seed,
                           void* stream);
int hpc_rll_lstm_backward_y(const float* dy, const float* dhn, const float* dcn, const float* x, const float* h0,
                            const float* c0, const float* wx, const float* wh, const float* ln_gamma, const float* y,
                            float* ws, float* dx, float* dh0, float* dc0, float* dwx, float* dwh, float* dbias,
                            float* dln_gamma, float* dln_beta, int S, int B, int I, int H, int L, float dropout_p,
                            uint64_t seed, void* stream);
/* Diagnostic: the kernels the most recent hpc_rll_lstm_forward* call of this process ran its recurrence on.  0 = one product
 * + one cell launch per step (what src/torch_utils/network/lstm.cu:145-161 does with three launches), 1 = per-layer
 * persistent kernels (B <= 4), 2 = layer wavefront (B <= 4, L >= 2), 3 = step kernels on gate-interleaved pre-activations
 * (large batch), 4 = persistent row-block kernel (large batch, tune key 26), 5 = persistent mid-batch kernel (5 <= B <= 256,
 * tune key 29); -1 = no forward yet.  Operands off a 16-byte boundary are accepted everywhere but on the large-batch shapes
 * of 3 / 4 (HPC_RLL_EALIGN): 1 and 2 need ws on an 8-byte boundary (their exchange words are 8-byte atomics), 5 needs ws and
 * h0 (forward) or ws (backward) on a 16-byte one; a call that does not meet this runs on the step kernels, 0. */
int hpc_rll_lstm_last_forward_path(void);
int hpc_rll_lstm_last_backward_path(void);   /* the same for the most recent hpc_rll_lstm_backward* call (its last layer; 5 = mid-batch kernel, key 33) */
/* Asynchronous status of the persistent small-batch LSTM kernels (B <= 4).  Their workgroups exchange data through
 * memory and must all be resident at once; that is checked against the runtime's occupancy figure at dispatch and
 * launches of one process are serialised per device, but ANOTHER PROCESS holding compute units for seconds can still
 * starve one.  The kernel then gives up (no trap, no hang), and -- like an asynchronous HIP error -- every later
 * hpc_rll_lstm_* call returns HPC_RLL_ETIMEOUT (the results of the launch that timed out are invalid) until
 * hpc_rll_clear_async_error(), after which the process uses the step kernels only.  hpc_rll_async_error() reads the
 * status without touching the device. */
int hpc_rll_async_error(void);
int hpc_rll_clear_async_error(void);
/* Test hooks, not operators.  occupy_device: launch `blocks` workgroups of 1024 threads and 80 KB of LDS (two of them
 * fill a CU completely; 0 = 2 per CU = the whole device) that spin for ~ms milliseconds on `stream`.  set_persist_spin_limit: polls a persistent LSTM kernel of the current
 * device waits before it gives up (0 = the shipped value, ~seconds). */
int hpc_rll_test_occupy_device(int ms, int blocks, void* stream);
int hpc_rll_test_set_persist_spin_limit(int64_t polls);
/* Exact-fp32 MFMA GEMM used by the LSTM, exposed for tests/benchmarks: C (M,N; row stride ldc) (+)= A * B with
 * A(m,k) = A[m*a_sm + k*a_sk], B(k,n) = B[k*b_sk + n*b_sn]. */
int hpc_rll_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int64_t a_sm, int64_t a_sk,
                     int64_t b_sk, int64_t b_sn, int64_t ldc, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * hpc_models: AlphaStar actor-critic inference helpers, forward only -- replaces actor_critic_update_ae,
 * actor_critic_lstm_activation, actor_critic_pre_sample (include/hpc/rll/cuda/models/entry.h:11-21,
 * src/models/actor_critic.cu:8-83).
 *   update_ae      : ae (B,D) += key_embeddings[b, sample_entity[b], :] unless sample_entity[b] == entity_num[b]
 *   lstm_activation: gates = ih + hh + bias (B,4H; order i,f,g,o); c (B,H) updated in place, h (B,H) written
 *   pre_sample     : out (B,E) = mask ? dot(mat[b,e,:], vec[b,:]) / div : mask_value / div   (mask: 1 byte per entry)
 * ------------------------------------------------------------------------------------------ */
int hpc_rll_actor_critic_update_ae(const float* key_embeddings, const int64_t* sample_entity,
                                   const int64_t* entity_num, float* autoregressive_embedding, int64_t B, int64_t E,
                                   int64_t D, void* stream);
int hpc_rll_actor_critic_lstm_activation(const float* ih, const float* hh, const float* bias, float* h, float* c,
                                         int64_t B, int64_t H, void* stream);
int hpc_rll_actor_critic_pre_sample(const float* mat, const float* vec, const uint8_t* mask, float* out, int64_t B,
                                    int64_t E, int64_t H, float mask_value, float div_factor, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HPC_RLL_HIP_H_ */
