/*
 * manytor_hip.h -- C ABI of libmanytor_hip.so (gfx950 / MI355X).
 *
 * Batched manipulator-environment step engine: N lock-stepped arms per handle,
 * state resident in HBM as struct-of-arrays, one HIP launch per step.
 *
 * The reference (victorkich/ManyTor, manytor.py) has no FFI boundary: its
 * boundary is the Python class surface of `Environment` / `Multienv`.  Each entry
 * point below names the reference interface it replaces (file:line in the
 * reference checkout) -- the Python host code in manytor_amd/ binds them with
 * ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns an mt_status (0 = ok, < 0 = error); the message of
 *     the last error is available through mt_last_error().
 *   - plain pointers and sizes only; no C++ / torch types.
 *   - a handle owns one device, one HIP stream (replaceable with
 *     mt_set_stream / mt_use_own_stream) and all of its device buffers.  A handle is not
 *     re-entrant; different handles may be used from different threads.
 *   - launches are asynchronous on the handle's stream; mt_sync() or any
 *     host-destination mt_get() synchronises.
 *   - angles are DEGREES (manytor.py:39), lengths are the DH table's units.
 *   - "env-major" = the reference's array shapes with a leading env axis, e.g.
 *     points (N, K, 3), obs (N, 3K).  "SoA" = the resident device layout, one
 *     row of length `ld` (>= N, multiple of 256) per scalar field component,
 *     e.g. points row (3*k + axis).
 */
#ifndef MANYTOR_HIP_H
#define MANYTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MT_API __attribute__((visibility("default")))
#else
#define MT_API
#endif

#define MT_VERSION 500      /* major*10000 + minor*100 + patch */
#define MT_MAX_DOF 8
#define MT_MAX_TARGETS 32
#define MT_MAX_RETURN_RING 64
#define MT_UNIQUE_ID_BYTES 128     /* = NCCL_UNIQUE_ID_BYTES of RCCL */

typedef struct mt_engine* mt_handle;

typedef enum mt_status {
  MT_OK = 0,
  MT_ERR_INVALID_ARG = -1,
  MT_ERR_HIP = -2,              /* a HIP runtime call failed; see mt_last_error */
  MT_ERR_NO_DEVICE = -3,
  MT_ERR_ALLOC = -4,
  MT_ERR_STATE = -5,            /* call order violated (e.g. step before reset) */
  MT_ERR_UNSUPPORTED = -6
} mt_status;

/* Fields of the resident state (mt_get / mt_set / mt_device_ptr). */
typedef enum mt_field {
  MT_F_ACTIONS = 0,       /* f32  env-major (N, D)      SoA rows: D        staged action, degrees            */
  MT_F_GOALS = 1,         /* f32  (N, D)                rows: D            manytor.py:133 `goals`            */
  MT_F_POINTS = 2,        /* f32  (N, K, 3)             rows: 3K           manytor.py:137 `points`           */
  MT_F_ALIVE = 3,         /* u8   (N, K) via mt_get; device: u32 bitmask per env (bit p = target p alive)    */
  MT_F_OBS = 4,           /* f32  (N, 3K)               rows: 3K           obs2 of the last step / observe   */
  MT_F_REWARD = 5,        /* i32  (N,)                                      reward of the last step           */
  MT_F_DONE = 6,          /* u8   (N,)   done of the last step: 0 running, 1 finished (mt_reset_done will re-arm it),  */
                          /*             2 finished and already re-armed inside mt_rollout_fused(auto_reset)          */
  MT_F_DONE_BITS = 7,     /* u64  (ceil(N/64),) one wavefront ballot per 64 envs, bit l = env 64*w + l       */
  MT_F_EE = 8,            /* f32  (N, 3)                rows: 3            end effector = joints_coordinates[-1] */
  MT_F_TOTAL_REWARD = 9,  /* f32  (N,)                                      manytor.py:138 `total_reward`     */
  MT_F_JOINTS = 10,       /* f32  (N, D, 3) computed on demand from goals (manytor.py:188-189); mt_get only  */
  MT_F_EPISODES = 11,     /* u32  (N,)   episode index of each env: set by a reset, +1 per auto re-arm          */
  MT_F_LAST_RETURN = 12,  /* f32  (N,)   total_reward the env had when it was last reset / re-armed             */
  MT_F_RETURN_RING = 13,  /* f32  (N, R) rows: R = mt_config.return_ring.  The return of the c-th episode an env finished */
                          /*             since the last full reset (re-armed by mt_reset_done or in-kernel) is in slot   */
                          /*             c % R; c = MT_F_EPISODES - (episode of the last full reset)                     */
  MT_F_TRACE = 14,        /* f32  (N, S, 3) rows: 3S.  End effector at each of the S sub-step poses of the last step     */
                          /*             (the rows manytor.py:190 appends to `trajectory`); needs MT_FLAG_TRACE          */
  MT_F_ZMIN = 15,         /* f32  (N,)   DEBUG (needs MT_FLAG_DEBUG_ZMIN): signed minimum z of the observation and pickup     */
                          /*             frames over ALL S sub-step poses of the last step, exactly the value the step     */
                          /*             kernel compares with 0 for the ground flag (manytor.py:191-192)                    */
  MT_F_COUNT = 16
} mt_field;

typedef enum mt_dtype { MT_F32 = 0, MT_F64 = 1, MT_I32 = 2, MT_I64 = 3, MT_U8 = 4, MT_U32 = 5, MT_U64 = 6 } mt_dtype;

typedef enum mt_layout { MT_ENV_MAJOR = 0, MT_SOA = 1 } mt_layout;

/* Engine flags (mt_config.flags).  0 = the default kernels, which reproduce the reference's semantics. */
#define MT_FLAG_TERMINATE_ON_GROUND 0x1u /* done |= ground hit (README.md:44 intent; NOT what manytor.py:170 does)  */
/* Measured alternatives of the step kernel (profiles/r01_variants.md); same results within the fp32 tolerance. */
#define MT_FLAG_HW_TRIG 0x2u             /* v_sin/v_cos at every interior sub-step instead of the recurrence       */
#define MT_FLAG_DH_IN_LDS 0x4u           /* DH constants staged in LDS instead of SGPRs (implies NO_SPECIALIZE)    */
#define MT_FLAG_DIRECT_TRIG 0x8u         /* polynomial sincos at every interior sub-step (no recurrence)           */
#define MT_FLAG_NO_SPECIALIZE 0x10u      /* never use a compile-time DH table, even if the table matches one       */
#define MT_FLAG_TRACE 0x20u              /* keep MT_F_TRACE: every step also writes the end effector of each       */
                                         /* sub-step pose (300 B/env-step at S = 25; off by default, manytor.py:190) */
#define MT_FLAG_DEBUG_ZMIN 0x40u         /* keep MT_F_ZMIN: the step / rollout kernels also store the z-minimum    */
                                         /* their ground test used (4 B/env-step; parity tests pin the sub-step    */
                                         /* recurrence of the timed kernels with it; off by default)               */
/* Profiling builds.  OUTPUTS ARE WRONG ON PURPOSE; never set outside bench.py --ablate. */
#define MT_FLAG_ABLATE_LOOP 0x100u       /* skip the interior sub-steps                                            */
#define MT_FLAG_ABLATE_OBS 0x200u        /* with ABLATE_LOOP: also skip the observation arithmetic (memory only);  */
                                         /* alone: keep all arithmetic, drop target loads / observation stores     */

/* Constructor arguments.  Replaces Environment.__init__/Multienv.__init__
 * (manytor.py:130-139, :77-82) plus the literals the reference hard-codes:
 * DH table manytor.py:42-48, substeps :178, pickup tolerance :162, radius :231. */
typedef struct mt_config {
  int32_t struct_size;          /* = sizeof(mt_config), checked                                  */
  int32_t device;               /* HIP device ordinal                                            */
  int64_t n_envs;               /* envs owned by this handle (this rank's shard)                 */
  int64_t env_id_base;          /* global id of local env 0: keys the device RNG so results do   */
                                /* not depend on the shard count                                 */
  int32_t dof;                  /* 2..MT_MAX_DOF joints                                          */
  int32_t n_targets;            /* 1..MT_MAX_TARGETS  (obj_number)                               */
  int32_t substeps;             /* >= 2; reference 25                                            */
  uint32_t flags;               /* MT_FLAG_*                                                     */
  float pickup_tol;             /* reference 8.0                                                 */
  float radius;                 /* target hemisphere radius, reference 51.3                      */
  float dh_table[MT_MAX_DOF * 4]; /* rows (a, alpha_rad, d, theta_offset_rad), manytor.py:42-48 */
  int32_t return_ring;          /* slots of MT_F_RETURN_RING per env, 0..MT_MAX_RETURN_RING (0 = none) */
  int32_t obs_frame;            /* row of joints_coordinates the observation is measured from: -dof..dof-1, Python   */
                                /* indexing; the reference uses [2] = -2, the elbow (manytor.py:143)                 */
  int32_t ee_frame;             /* row the pickup test uses; reference [3] = -1, the end effector (manytor.py:162).  */
                                /* The ground test looks at the z of both rows (manytor.py:191).  Row 0 = the origin */
  int32_t reserved;             /* must be 0                                                     */
} mt_config;

MT_API int mt_version(void);
MT_API const char* mt_status_string(int status);
/* Message of the last failing call on this handle (or, with h == NULL, of the
 * last failing call on the calling thread that had no handle). */
MT_API const char* mt_last_error(mt_handle h);
MT_API int mt_device_count(int* count);

/* Environment()/Multienv() constructors, manytor.py:130-139 / :77-82. */
MT_API int mt_create(mt_handle* out, const mt_config* cfg);
MT_API int mt_destroy(mt_handle h);
/* Which instantiation mt_step / mt_step_random launch for this handle (the schedule is picked by batch size and table
 * at mt_create; every schedule gives the same bits): e.g. "step_kernel<Ref4Table, trig=0, lds=false, pf=8>",
 * "step_split_kernel<RtTable<5>, L=4>".  For benchmark records and profiles; valid until the next call on the handle. */
MT_API const char* mt_step_kernel_name(mt_handle h);
/* The dispatch of this handle as data: a JSON object with the schedule resolved for every entry point ("step",
 * "chains", "rollout", "fused", "reset"), the MT_* environment overrides that were in effect at mt_create ("overrides")
 * and the library's one table of size thresholds ("policy": engine.hip kPolicy).  Tests assert regimes from it instead
 * of parsing kernel names; valid until the next mt_describe_dispatch on the handle. */
MT_API const char* mt_describe_dispatch(mt_handle h);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream), so that the handle's launches are ordered with
 * the caller's own work on that stream.  NULL means what it means to HIP: the legacy default stream (which is what
 * torch's default stream is).  mt_use_own_stream goes back to the handle's private non-blocking stream, which is
 * NOT ordered against any other stream: readers of the device buffers must then mt_sync() first.  Both calls
 * drain the stream the handle was on. */
MT_API int mt_set_stream(mt_handle h, void* hip_stream);
MT_API int mt_use_own_stream(mt_handle h);
MT_API int mt_sync(mt_handle h);

/* Environment.reset(), manytor.py:219-253, for all envs.
 * mt_reset: targets supplied by the caller (parity mode: the host draws them from
 * numpy's global RNG in the reference's order).  `points` is (N, K, 3) f32
 * env-major or (3K, ld) SoA, in host or device memory.
 * mt_reset_random: targets rejection-sampled on the device (Philox-4x32-10 keyed by
 * seed / global env id / episode), same law as manytor.py:229-239. */
/* Host arrays are screened: a NaN or an infinite coordinate is MT_ERR_INVALID_ARG and nothing is written.  Targets handed
 * over in device memory cannot be screened on the host: the reset kernel drops an unusable one (dead from the start,
 * coordinates zeroed) and counts it (mt_bad_action_count). */
MT_API int mt_reset(mt_handle h, const float* points, int layout, int is_device);
/* On a handle that runs on its OWN stream and whose mt_rollout runs several steps per launch (<= 262 144 envs), the launch of
 * mt_reset_random is deferred: the next mt_rollout performs the reset as the prologue of its first launch (the same state,
 * bit for bit, one launch and one round trip of the state less), and every other entry point -- mt_sync included, which is
 * what the own-stream contract asks for before anything else looks at the state -- launches it first; only the region
 * timers (mt_timer_start / mt_timer_stop*) leave it alone, it belongs to what follows them.  A single-step mt_rollout absorbs it
 * as well.  On a caller's stream (mt_set_stream) the reset is launched by the call itself, in stream order.
 * MT_DEFER_RESET=0 disables the deferral. */
MT_API int mt_reset_random(mt_handle h, uint64_t seed, uint32_t episode);
/* Re-arm only the envs whose done byte is 1: their return goes to MT_F_LAST_RETURN and into MT_F_RETURN_RING, their
 * episode index (MT_F_EPISODES) advances by one and keys the new targets (device RNG), pose and return are zeroed.
 * Envs with done == 2 were already re-armed inside mt_rollout_fused: only their flag is cleared.  Not in the
 * reference (the caller resets everything, test_multi.py:34; reset on done is caller-driven, test_single.py:20-21,32);
 * SURVEY.md 8(f) rank 1. */
MT_API int mt_reset_done(mt_handle h, uint64_t seed);
/* `multienv.environment[i].reset()` (manytor.py:82 + :219-253): reset ONE env of the batch.  `points` = K x 3 host
 * floats, or NULL to draw them on the device (Philox keyed by seed / global env id / `episode`). */
MT_API int mt_env_reset(mt_handle h, int64_t env, const float* points, uint64_t seed, uint32_t episode);

/* Stage the action of the next mt_step: (N, D) env-major or (D, ld) SoA, degrees,
 * any of f32/f64/i32/i64 (Environment.action_sample returns np.int64, manytor.py:216). */
MT_API int mt_set_actions(mt_handle h, const void* actions, int dtype, int layout, int is_device);
/* Environment.action_sample(), manytor.py:215-217, for all envs on the device:
 * integer degrees uniform in [-180, 180), written to the action buffer. */
MT_API int mt_sample_actions(mt_handle h, uint64_t seed, uint32_t step_idx);

/* Environment.step() = get_observations() side effect + action() + return
 * accumulation + is_done(), manytor.py:255-260, :175-213, for all envs, one launch. */
/* On a multi-chain handle (163 840 .. 3 M envs, see mt_rollout) that runs on its OWN stream the step is two launches, one
 * per half of the env range on its own stream; mt_set_actions from DEVICE memory and mt_sample_actions stage each half's
 * rows on the same streams, so a policy loop (set actions / step / ...) keeps the halves independent from call to call
 * (any other call and mt_sync fold them back): 42 -> 37.5 us per step at 1 M envs.  On a caller's stream (mt_set_stream)
 * the step stays one launch: forking behind the caller's work and joining back for a single launch costs more than it
 * hides.  Same bits either way. */
MT_API int mt_step(mt_handle h);
/* One host round trip of Multienv.step (manytor.py:115-122): (N, D) host actions in, obs2 (N, 3K) f32, reward (N,)
 * i32 and done (N,) u8 out, through one page-locked staging buffer and ONE stream synchronisation (instead of the
 * four that mt_set_actions + mt_step + 3 x mt_get cost).  For small batches driven from host code. */
MT_API int mt_step_host(mt_handle h, const void* actions, int dtype, float* obs, int32_t* reward, uint8_t* done);
/* `multienv.environment[i].step(action)` (manytor.py:82,118 + :255-260): step ONE env of the batch with a host action of
 * D degrees; the other envs are untouched.  obs (3K f32), reward, done are written to host memory; synchronises. */
MT_API int mt_env_step(mt_handle h, int64_t env, const float* action, float* obs, int32_t* reward, uint8_t* done);
/* Number of (env, step) pairs so far whose staged action was not a finite angle of magnitude <= 32768 degrees (NaN,
 * +-inf from a diverging policy ...).  Such an env holds its pose for that step instead of poisoning its state.
 * Synchronises.  The reference has no such check (numpy would propagate the NaN into goals, manytor.py:184).
 * Every angle inside that range is a full citizen: positions and the ground test keep their 1e-4 accuracy against the
 * fp64 reference up to +-32768 degrees (beyond +-180 the kernels form the route's angles in double, modulo 360).
 * Also counts the targets mt_reset dropped because a coordinate handed over in device memory was NaN / infinite. */
MT_API int mt_bad_action_count(mt_handle h, uint64_t* count);
/* The same with the action drawn in-kernel (results bit-identical to mt_sample_actions followed by
 * mt_step).  The drawn action is not stored in MT_F_ACTIONS: it is the new MT_F_GOALS (goals = action after a
 * step, manytor.py:184), which saves 4*D bytes of traffic per env. */
MT_API int mt_step_random(mt_handle h, uint64_t seed, uint32_t step_idx);
/* n_steps x mt_step_random with step indices step_idx0, step_idx0+1, ... (the
 * inner loop of test_multi.py:19-21).  The call exposes the state after n_steps steps and the outputs of the LAST one
 * (obs, reward, done, end effector), so on small shards (<= 262 144 envs) it runs FIVE steps per launch through the
 * kernels of mt_rollout_fused -- joint angles, alive mask and return in registers, targets in LDS between them; every
 * step still computes and writes its outputs -- bit-identical to the launch-per-step sequence, without four of five
 * kernel boundaries and state re-fetches (MT_ROLLOUT_K=1 gives one launch per step back; then batches <= 131 072 envs are
 * replayed from a HIP graph that the handle captures once per segment length).
 * On large batches (above 262 144 and up to 3 M envs; from 163 840 with MT_ROLLOUT_K=1) the call runs as TWO independent chains of launches -- the two halves of the env
 * range (256-aligned) on two streams forked from the handle's stream: a step of env i depends only on env i, so the
 * results are bit-identical, and one half's kernel boundary is hidden behind the other half's kernel (-10 % per step at
 * 1 M envs).  On the handle's own stream the chains stay forked when the call returns: the next mt_rollout continues them,
 * mt_reset_random resets each half behind its own last step, mt_gather_returns_begin snapshots each half on its chain;
 * mt_step / mt_sample_actions / mt_set_actions(device) run per half as well (see mt_step); every other call -- mt_sync,
 * getters, setters, mt_reset_done, timers' begin ... -- folds them back into the
 * handle's stream first, so "mt_sync before foreign reads" means what it did.  On a caller's stream (mt_set_stream) the
 * chains are joined before the call returns: work queued on that stream afterwards sees the completed rollout. */
MT_API int mt_rollout(mt_handle h, int n_steps, uint64_t seed, uint32_t step_idx0);
/* The same n_steps steps in ONE launch: joint angles, alive mask and return stay in registers and the targets
 * in LDS between steps, so a step only writes its outputs (obs, reward, done, end effector; MT_F_* hold the last
 * step's).  auto_reset != 0 re-arms an env in the step it finishes, exactly like mt_reset_done after every step:
 * every finished return lands in MT_F_RETURN_RING, and an env that finished in the LAST step keeps done == 2
 * (finished, already re-armed) so that a following mt_reset_done does not reset it twice.
 * State after the call is bit-identical to the launch-per-step sequence. */
MT_API int mt_rollout_fused(mt_handle h, int n_steps, uint64_t seed, uint32_t step_idx0, int auto_reset);

/* The same residency for actions the CALLER chose: T steps in one launch, driven by a (T, D, N) block of angles that is
 * already on the device (a sampling planner's candidates, a recorded episode, an open-loop chunk of a policy).
 * A committing call behaves as T x (mt_set_actions(tape row t); mt_step), with MT_TAPE_AUTO_RESET as T x (...;
 * mt_reset_done(seed)): MT_F_* hold the state after T steps and the outputs of the LAST step (MT_F_DONE == 2 for an env
 * re-armed in it), ring / MT_F_LAST_RETURN / MT_F_EPISODES behave as with mt_rollout_fused(auto_reset), bit for bit.  An
 * unusable action (NaN, +-inf, beyond +-32768 degrees) makes that env hold its pose for that step and is counted
 * (mt_bad_action_count).  Intermediate steps neither compute nor store observations; per step the call writes only the
 * two log bytes, where asked for.  One launch on the handle's stream, no allocation, no host wait: legal under stream
 * capture.  MT_TAPE_DRY_RUN evaluates only: logs and return_out are written, nothing resident changes (state, MT_F_*
 * outputs, ring, counters) -- "what would these T actions earn from here?".
 * MT_ERR_UNSUPPORTED on handles whose flags the rollout kernels do not implement (HW_TRIG, DIRECT_TRIG, DH_IN_LDS,
 * TRACE, custom frames); MT_ERR_STATE before a reset; n_steps == 0 is a no-op. */
#define MT_TAPE_AUTO_RESET 0x1u   /* re-arm an env in the step it finishes, as mt_reset_done(seed) after every step would */
#define MT_TAPE_DRY_RUN    0x2u   /* evaluate only: nothing resident changes (state, MT_F_* outputs, ring, counters) */
typedef struct mt_tape {
  int32_t struct_size;      /* = sizeof(mt_tape), checked */
  int32_t n_steps;          /* T >= 0 */
  const float* actions;     /* DEVICE, f32, degrees: joint j of env i at step t = actions[(t*D + j)*ld + i] */
  int64_t ld;               /* row pitch in elements, >= n_envs (no other alignment asked) */
  int8_t*  reward_log;      /* DEVICE or NULL: reward of env i at step t -> reward_log[t*log_ld + i] */
  uint8_t* done_log;        /* DEVICE or NULL: 1 where env i finished in step t, else 0 */
  int64_t log_ld;           /* >= n_envs when a log is given */
  float* return_out;        /* DEVICE or NULL: (N,) sum of the call's T rewards of env i (across re-arms) */
  uint64_t seed;            /* keys the targets of re-armed envs (MT_TAPE_AUTO_RESET) */
  uint32_t flags;           /* MT_TAPE_* */
  uint32_t reserved;        /* must be 0 */
} mt_tape;
MT_API int mt_rollout_tape(mt_handle h, const mt_tape* tape);

/* A sampling planner's round in one call: score C candidate tapes per env from the SAME resident state, name each env's
 * best, and (commit_steps = H > 0) execute the first H steps of that best plan for real.
 * Evaluation: returns_out[c*ret_ld + i] is what mt_rollout_tape(MT_TAPE_DRY_RUN, actions = plane c, the same ld) writes to
 * return_out[i], bit for bit; best_out[i] is the SMALLEST c whose return is maximal (numpy's argmax), best_return_out[i]
 * that return.  The state is read once for all candidates, the selection happens on the device, nothing resident changes
 * and unusable actions (see mt_rollout_tape) hold the pose without being counted.
 * Commit: afterwards the handle is in the state mt_rollout_tape leaves for n_steps = H, the same seed, MT_TAPE_AUTO_RESET
 * iff MT_SHOOT_AUTO_RESET, and the gathered tape chosen[(t*D + j)*ld + i] = actions[best_out[i]*cand_stride + (t*D + j)*ld + i]
 * -- every field, the logs, return_out and mt_bad_action_count (the H committed steps of the chosen plane, once each).
 * At most two launches on the handle's stream (evaluate + select, commit), no allocation, no host wait: legal under
 * stream capture.  MT_ERR_UNSUPPORTED / MT_ERR_STATE as mt_rollout_tape; n_steps == 0 is a no-op. */
#define MT_SHOOT_AUTO_RESET 0x1u  /* the committed steps re-arm finished envs, as MT_TAPE_AUTO_RESET */
struct mt_shoot {          /* the struct and the call share the name, so the type is always written `struct mt_shoot` */
  int32_t struct_size;     /* = sizeof(struct mt_shoot), checked */
  int32_t n_steps;         /* T >= 0: horizon every candidate is scored over */
  int32_t n_candidates;    /* C, 1..64 */
  int32_t commit_steps;    /* H, 0..T: 0 = evaluate only; else execute steps 0..H-1 of each env's best plan for real */
  const float* actions;    /* DEVICE f32 degrees: candidate c, step t, joint j, env i = actions[c*cand_stride + (t*D + j)*ld + i] */
  int64_t ld;              /* >= n_envs */
  int64_t cand_stride;     /* elements between candidates, >= T*D*ld */
  float* returns_out;      /* DEVICE or NULL: (C, ret_ld) return of every candidate */
  int64_t ret_ld;          /* >= n_envs when returns_out is given */
  int32_t* best_out;       /* DEVICE (N,): index of each env's best candidate; required when commit_steps > 0, else optional */
  float* best_return_out;  /* DEVICE or NULL (N,): that candidate's return over the T steps */
  int8_t* reward_log; uint8_t* done_log; int64_t log_ld;   /* (H, log_ld) logs of the COMMITTED steps, as in mt_tape */
  float* return_out;       /* DEVICE or NULL (N,): sum of the H committed rewards (across re-arms) */
  uint64_t seed;           /* keys re-armed envs' targets (MT_SHOOT_AUTO_RESET) */
  uint32_t flags, reserved;
};
MT_API int mt_shoot(mt_handle h, const struct mt_shoot* s);

/* One iteration of the cross-entropy method (CEM) in one call: draw C candidate plans per env around (mean, sigma), score
 * them as mt_shoot does, pick the best and the E best ("elites"), refit (mean, sigma) from the elites and (commit_steps =
 * H > 0) execute the first H steps of the best plan.  No (C, T, D, N) block exists: the candidates are drawn in the kernel.
 *
 * The candidate stream.  For the global env id e = env_id_base + i, candidate c, step t and joint j:
 *   w = Philox-4x32-10 block of counter (e_lo, e_hi[23:0] | 3 << 24, draw, (c << 24) | (b << 16) | t), key = seed,
 *       b = 0 and word j for j < 4, b = 1 and word j - 4 for j >= 4
 *   z = (float)((int)(sum of the four bytes of w) - 510) * KZ,  KZ = the fp32 nearest to 1 / sqrt(21845)
 *       (Irwin-Hall of four uniform bytes: mean 0, variance 1, |z| <= 3.4506; the multiply is the only rounding)
 *   x = mean[(t*D + j)*ld + i] + sigma[(t*D + j)*ld + i] * z      (an fp32 multiply, then an fp32 add)
 *   x is handed on as it is when it is unusable (NaN, +-inf, beyond +-32768 degrees: the step holds the pose, as for any
 *   tape), else clamped: min(max(x, lo), hi).  MT_CEM_KEEP_MEAN: candidate 0 has z = 0, i.e. it is the clamped mean.
 * mean and sigma are device memory and cannot be screened: a non-finite mean or sigma of env i makes env i's candidates
 * score as held poses and leaves its refit unspecified; no other env's outputs change.
 *
 * mt_sample_plans writes exactly this block P, P[c][t][j][i] = plans_out[c*cand_stride + (t*D + j)*ld + i] (mt_shoot's
 * layout; plans_out is DEVICE f32).  It reads n_steps, n_candidates, draw, mean, sigma, ld, lo, hi, seed and flags only,
 * and needs no reset.
 *
 * mt_cem, with P the block mt_sample_plans writes for the same struct:
 *   evaluation  returns_out, best_out, best_return_out are, bit for bit, what mt_shoot writes for actions = P (the lowest
 *               index wins a tie; nothing resident changes; a refused angle is not counted).
 *   elites      order the candidates of env i by (return descending, index ascending); the first E are its elites and
 *               elite_mask_out[i] has exactly their bits set.
 *   refit       in fp32, one rounding per operation: with the elites e0 < e1 < ... and x_k = P[e_k][t][j][i],
 *               m = (((x_0 + x_1) + x_2) + ...) * invE, invE = the fp32 nearest to 1 / E;  d_k = x_k - m;
 *               v = (((d_0*d_0 + d_1*d_1) + ...)) * invE;  mean_out = m, sigma_out = max(sqrt(v), sigma_min).
 *               mean_out / sigma_out may be EXACTLY mean / sigma (same pointer, out_ld == ld): the refit is then in place.
 *               Any other overlap of mean_out / sigma_out / chosen_out with mean / sigma or each other is refused.
 *   commit      chosen_out[(t*D + j)*chosen_ld + i] = P[best[i]][t][j][i] for t < H, and the handle is afterwards where
 *               mt_rollout_tape(n_steps = H, actions = chosen_out, the same seed, MT_TAPE_AUTO_RESET iff MT_CEM_AUTO_RESET)
 *               leaves it: every field, the logs, return_out, mt_bad_action_count.
 * At most two launches on the handle's stream, no allocation, no host wait: legal under stream capture.
 * MT_ERR_UNSUPPORTED / MT_ERR_STATE as mt_shoot; n_steps == 0 is a no-op; lo, hi (finite, lo <= hi, within +-32768) and
 * sigma_min (finite, >= 0) are screened on the host. */
#define MT_CEM_AUTO_RESET 0x1u   /* committed steps re-arm finished envs, as MT_TAPE_AUTO_RESET */
#define MT_CEM_KEEP_MEAN  0x2u   /* candidate 0 is the clamped mean (z = 0) */
struct mt_cem {            /* as with mt_shoot, the type is always written `struct mt_cem` */
  int32_t struct_size;     /* = sizeof(struct mt_cem), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_candidates;    /* C, 1..64 */
  int32_t n_elites;        /* E, 1..C */
  int32_t commit_steps;    /* H, 0..T */
  uint32_t draw;           /* major counter word of the plan stream (e.g. the iteration number) */
  const float *mean, *sigma; int64_t ld;         /* DEVICE (T, D, ld), ld >= n_envs */
  float *mean_out, *sigma_out; int64_t out_ld;   /* DEVICE or both NULL: the refit; may be EXACTLY mean / sigma with out_ld == ld */
  float lo, hi, sigma_min;
  float* returns_out; int64_t ret_ld;            /* DEVICE or NULL: (C, ret_ld) return of every candidate */
  int32_t* best_out; float* best_return_out;     /* DEVICE or NULL (N,): as mt_shoot */
  uint64_t* elite_mask_out;                      /* DEVICE or NULL (N,): bit c set iff candidate c is an elite of env i */
  float* chosen_out; int64_t chosen_ld;          /* DEVICE (H, D, chosen_ld): steps 0..H-1 of each env's best candidate; required when H > 0 */
  int8_t* reward_log; uint8_t* done_log; int64_t log_ld; float* return_out;   /* of the committed steps, as mt_shoot */
  uint64_t seed;           /* keys the plan stream AND the re-armed envs' targets */
  uint32_t flags, reserved;
};
MT_API int mt_cem(mt_handle h, const struct mt_cem* s);
/* (plans_out is a void* like mt_get's destination: the block is output only, there is nothing to screen) */
MT_API int mt_sample_plans(mt_handle h, const struct mt_cem* s, void* plans_out, int64_t ld, int64_t cand_stride);

/* One MPPI (model-predictive path integral) iteration in one call: draw C candidate plans per env around (mean, sigma),
 * score them as mt_shoot does, weigh EVERY candidate by exp((R_c - R_best) / lambda), refit the mean (and on request sigma)
 * as the weighted moments of the candidates and (commit_steps = H > 0) execute the first H steps of the best plan.  No
 * (C, T, D, N) block exists, and no transcendental function is evaluated: a step's reward is -1, 0 or +1, so a return over
 * T steps is an integer in [-T, T], the gap to the best return an integer k in [0, 2T], and with decay = rho =
 * exp(-1 / lambda) the weight is rho^k, read from a table of 2T + 1 powers.
 *
 * mt_mppi, with P the block mt_sample_plans writes for a struct mt_cem with the same n_steps, n_candidates, draw, mean,
 * sigma, ld, lo, hi, seed and KEEP_MEAN (the same Philox tag 3, counter and rounding: there is no new stream):
 *   evaluation  returns_out, best_out, best_return_out are, bit for bit, what mt_shoot writes for actions = P (the lowest
 *               index wins a tie; nothing resident changes; a refused angle is not counted).
 *   weights     W[0] = 1, W[k] = W[k-1] * decay for k <= 2T, one fp32 rounding per entry; k_c = (int)(best_return - R_c),
 *               exact because both are integer-valued; w_c = W[k_c]; weights_out[c*w_ld + i] = w_c.  decay = 0 is the
 *               hard maximum (only candidates tied with the best count), decay = 1 the plain average.
 *   refit       in fp32, one rounding per operation; every sum starts from +0 and takes c = 0, 1, ..., C-1 in order.
 *               With x_c = P[c][t][j][i]:  S = sum of w_c;  A = sum of fl(w_c * x_c);  m = A / S (one correctly rounded
 *               division);  mean_out = m.  With sigma_out: d_c = x_c - m, Q = sum of fl(w_c * fl(d_c * d_c)),
 *               sigma_out = max(sqrt(Q / S), sigma_min).  weight_sum_out[i] = S; S >= 1, the best candidate weighs 1.
 *               (A term whose weight is 0 may be skipped: with finite x it adds +-0 to a sum that started from +0.)
 *               mean_out alone is a fixed-sigma MPPI; both, or neither, are allowed; sigma_out without mean_out is refused.
 *               mean_out / sigma_out may be EXACTLY mean / sigma (same pointer, out_ld == ld): the refit is then in place.
 *               Any other overlap of mean_out / sigma_out / chosen_out with mean / sigma or each other is refused.
 *               The refit of env i is unspecified when its mean or sigma is non-finite or any of its drawn angles is
 *               unusable; no other env's outputs change.
 *   commit      chosen_out[(t*D + j)*chosen_ld + i] = P[best[i]][t][j][i] for t < H, and the handle is afterwards where
 *               mt_rollout_tape(n_steps = H, actions = chosen_out, the same seed, MT_TAPE_AUTO_RESET iff MT_MPPI_AUTO_RESET)
 *               leaves it: every field, the logs, return_out, mt_bad_action_count.
 * At most two launches on the handle's stream, no allocation, no host wait: legal under stream capture.
 * MT_ERR_UNSUPPORTED / MT_ERR_STATE as mt_cem; n_steps == 0 is a no-op; lo, hi (finite, lo <= hi, within +-32768),
 * sigma_min (finite, >= 0) and decay (finite, 0 <= decay <= 1) are screened on the host. */
#define MT_MPPI_AUTO_RESET 0x1u   /* committed steps re-arm finished envs, as MT_TAPE_AUTO_RESET */
#define MT_MPPI_KEEP_MEAN  0x2u   /* candidate 0 is the clamped mean (z = 0), as MT_CEM_KEEP_MEAN */
#define MT_MPPI_MAX_STEPS  127    /* 2T + 1 <= 255 table entries: every possible gap has its own weight, no clamp */
struct mt_mppi {           /* as with mt_cem, the type is always written `struct mt_mppi` */
  int32_t struct_size;     /* = sizeof(struct mt_mppi), checked */
  int32_t n_steps;         /* T, 0..MT_MPPI_MAX_STEPS */
  int32_t n_candidates;    /* C, 1..64 */
  int32_t commit_steps;    /* H, 0..T */
  uint32_t draw;           /* major counter word of the plan stream (e.g. the iteration number) */
  float decay;             /* rho = exp(-1 / lambda), finite, 0 <= rho <= 1 */
  const float *mean, *sigma; int64_t ld;         /* DEVICE (T, D, ld), ld >= n_envs */
  float *mean_out, *sigma_out; int64_t out_ld;   /* DEVICE or NULL: the refit (mean_out alone, both, or neither); may be EXACTLY mean / sigma with out_ld == ld */
  float lo, hi, sigma_min;
  float* returns_out; int64_t ret_ld;            /* DEVICE or NULL: (C, ret_ld) return of every candidate */
  float* weights_out; int64_t w_ld;              /* DEVICE or NULL: (C, w_ld) weight of every candidate */
  float* weight_sum_out;                         /* DEVICE or NULL (N,): S, the sum of env i's weights */
  int32_t* best_out; float* best_return_out;     /* DEVICE or NULL (N,): as mt_shoot */
  float* chosen_out; int64_t chosen_ld;          /* DEVICE (H, D, chosen_ld): steps 0..H-1 of each env's best candidate; required when H > 0 */
  int8_t* reward_log; uint8_t* done_log; int64_t log_ld; float* return_out;   /* of the committed steps, as mt_shoot */
  uint64_t seed;           /* keys the plan stream AND the re-armed envs' targets */
  uint32_t flags, reserved;
};
MT_API int mt_mppi(mt_handle h, const struct mt_mppi* s);

/* A policy in the loop, in one launch: T x (observe; MLP; step) with the residency of mt_rollout_tape -- pose, alive mask
 * and return in registers, targets in LDS, the state read and written once per call.  The third action source of the
 * rollout kernels (in-kernel random draws: mt_rollout_fused; a device tape: mt_rollout_tape; a policy: this call).
 *
 * Input.  At every step t the policy of env i sees x, the IN-vector mt_observe would write to MT_F_OBS for the state the
 * step STARTS from: for target k the triple (dist, r, theta) measured from the observation frame at the current pose,
 * (0, 0, 0) for a dead target; IN = 3K, with MT_POLICY_SEE_POSE the D joint angles in degrees follow (IN = 3K + D).
 * After an in-kernel re-arm the current state is the zero pose with the new targets.  NOTE that x is not the obs2 the
 * previous step returned: a step's observation is taken BEFORE its pickup (manytor.py:91-93), so obs2 still shows the
 * target the step just picked, while x shows it dead.
 * Layers.  h_0 = x;  y = W_l h_l + b_l in fp32 (accumulation order and fusing unspecified, but fixed: results are
 * deterministic and a function of the env's own state, the weights and (seed, global env id, draw, t) -- batch size and
 * sharding change no bit);  h_{l+1} = hidden_act(y) for l < L-1;  a_j = out_scale * out_act(y_j) for the last layer,
 * which has D outputs.  tanh is 1 - 2 / (exp(2y) + 1) with hardware exp2 / reciprocal, absolute error < 1e-6.
 * Weights and biases are device memory and cannot be screened; they are expected to be finite.  A NaN among them goes
 * through every activation and ends in an unusable action; an infinite weight does the same wherever its input is 0
 * (0 * inf).  No word outside the (out, in) matrices and (out,) vectors is read, whatever the widths.
 * Noise.  With sigma_j > 0, a_j += sigma_j * z (an fp32 multiply, then an fp32 add), z the Irwin-Hall variate of mt_cem
 * (the same byte sum, the same KZ) of word j (j < 4: b = 0) or j - 4 (b = 1) of the Philox-4x32-10 block with counter
 * (e_lo, e_hi[23:0] | 4 << 24, draw, (b << 16) | t), key = seed: tag 4, a stream of its own.  t counts the steps of the
 * call and keeps counting across re-arms.
 * The result is handed on as it is when it is unusable (NaN, +-inf, beyond +-32768 degrees: the env holds its pose for
 * that step and the pair is counted, as for any tape), else clamped: min(max(a, lo), hi).  action_log gets what was
 * handed on.
 * A committing call leaves the handle where mt_rollout_tape leaves it for the same start state, actions = action_log,
 * the same T and seed, MT_TAPE_AUTO_RESET iff MT_POLICY_AUTO_RESET: every field, the outputs of the last step, the logs,
 * return_out, ring / MT_F_LAST_RETURN / MT_F_EPISODES and mt_bad_action_count, bit for bit.  MT_POLICY_DRY_RUN writes
 * the logs, action_log, obs_log and return_out and nothing resident; together with MT_POLICY_AUTO_RESET it is refused.
 * One launch on the handle's stream, no allocation, no host wait: legal under stream capture.  The weights are read in
 * stream order; they stay the caller's until then.  MT_ERR_UNSUPPORTED / MT_ERR_STATE as mt_rollout_tape; n_steps == 0
 * is a no-op; everything the host can see of the struct is screened (MT_ERR_INVALID_ARG). */
#define MT_POLICY_AUTO_RESET 0x1u   /* re-arm finished envs in the step they finish, as MT_TAPE_AUTO_RESET */
#define MT_POLICY_DRY_RUN    0x2u   /* evaluate only: logs and return_out are written, nothing resident changes */
#define MT_POLICY_SEE_POSE   0x4u   /* the D joint angles (degrees) are appended to the policy's input */
#define MT_POLICY_MAX_LAYERS 3      /* linear layers: at most two hidden ones and the output layer */
#define MT_POLICY_MAX_WIDTH  64
enum { MT_ACT_IDENTITY = 0, MT_ACT_TANH = 1, MT_ACT_RELU = 2 };
struct mt_policy {         /* as with mt_cem, the type is always written `struct mt_policy` */
  int32_t struct_size;     /* = sizeof(struct mt_policy), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_layers;        /* L, 1..MT_POLICY_MAX_LAYERS */
  int32_t width[2];        /* outputs of hidden layer 0 .. L-2, each 1..MT_POLICY_MAX_WIDTH; the last layer has D outputs */
  int32_t hidden_act;      /* MT_ACT_TANH or MT_ACT_RELU */
  int32_t out_act;         /* MT_ACT_TANH or MT_ACT_IDENTITY */
  uint32_t draw;           /* major counter word of the exploration-noise stream */
  const float* weight[3];  /* DEVICE f32, dense row-major (out, in): torch.nn.Linear.weight as it lies in memory */
  const float* bias[3];    /* DEVICE f32 (out,) */
  float out_scale, lo, hi; /* action = clamp(out_scale * out_act(y) + noise, lo, hi) */
  float sigma[MT_MAX_DOF]; /* per-joint exploration sigma in degrees, finite, >= 0; all zero = deterministic */
  uint32_t flags;          /* MT_POLICY_* */
  float* action_log; int64_t act_ld;   /* DEVICE or NULL: (T, D, act_ld), mt_tape's layout: the action handed to step t */
  float* obs_log;    int64_t obs_ld;   /* DEVICE or NULL: (T, IN, obs_ld): the input vector the policy saw at step t */
  int8_t* reward_log; uint8_t* done_log; int64_t log_ld; float* return_out;   /* as mt_tape */
  uint64_t seed;           /* keys the noise stream AND re-armed envs' targets */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_rollout_policy(mt_handle h, const struct mt_policy* p);

/* mt_rollout_policy with what an actor-critic collection wants from the same launch: the log-probability of every action
 * under the policy that drew it, and a critic's value of every state, the one behind the last step included.
 *
 * Resident state.  `policy` is mt_rollout_policy's argument, its own struct_size included, and everything that call does
 * for it this call does, bit for bit: every field, the logs, return_out, ring / MT_F_LAST_RETURN / MT_F_EPISODES,
 * mt_bad_action_count, the flags, the refusals (their messages name mt_actor_critic.policy).
 * logp_log[t, i] is mt_policy_eval's logp_out for x = obs_log[t, :, i], a = action_log[t, :, i], the policy's weights and
 * policy.sigma, bit for bit: e = a_j - mu_j, d = e * inv_var_j, lp = fmaf(e, d, lp) for ascending j, -0.5f * lp, with
 * inv_var_j the fp32 nearest to 1 / sigma_j^2, mu_j the mean in front of the noise and a_j what action_log gets; a sample
 * whose action is unusable gets exactly 0.  With logp_log every sigma_j, j < D, must be finite and > 0.  Neither obs_log
 * nor action_log has to be given.
 * The critic is an MLP of the policy's shape and limits whose last layer has ONE output, on the same x (IN as the policy's,
 * MT_POLICY_SEE_POSE included): value_log[t, i] is mt_policy_eval's mean_out with n_out = 1 for it, bit for bit, and
 * last_value_out[i] the same for x_T, the input a step T would start from (after a re-arm in the last step: the zero pose
 * with the new targets).  last_value_out is written by a dry run too.
 * With a critic the kernel keeps x of a block in LDS behind the targets: 3 K + IN <= MT_ACTOR_CRITIC_MAX_LDS / 1024 = 160,
 * that is K <= 26 without MT_POLICY_SEE_POSE; a handle beyond that gets MT_ERR_UNSUPPORTED (logp_log alone has no limit).
 * critic_layers == 0 with value_log or last_value_out, and a call with neither a critic nor logp_log (which is
 * mt_rollout_policy), are MT_ERR_INVALID_ARG; so are an ld below n_envs and any overlap of the three outputs with the
 * weights of either network, with the policy's logs or with each other.  n_steps == 0 is a no-op: nothing is written.
 * One launch on the handle's stream, no allocation, no host wait: legal under stream capture. */
#define MT_ACTOR_CRITIC_MAX_LDS 163840   /* bytes of LDS a block may hold: (3 K + IN) * 256 lanes * 4 */
struct mt_actor_critic {   /* as with mt_cem, the type is always written `struct mt_actor_critic` */
  int32_t struct_size;     /* = sizeof(struct mt_actor_critic), checked */
  int32_t critic_layers;   /* 0 = no critic, else 1..MT_POLICY_MAX_LAYERS */
  struct mt_policy policy; /* everything mt_rollout_policy reads; policy.struct_size = sizeof(struct mt_policy), checked */
  int32_t critic_width[2]; /* hidden widths of the critic, each 1..MT_POLICY_MAX_WIDTH */
  int32_t critic_hidden_act, critic_out_act;   /* as mt_value_grad: out is MT_ACT_IDENTITY or MT_ACT_TANH */
  const float* critic_weight[3];   /* DEVICE f32 (out, in); the last layer is (1, in) */
  const float* critic_bias[3];     /* DEVICE f32 (out,) */
  float critic_out_scale;  /* V = critic_out_scale * critic_out_act(y), finite */
  uint32_t pad_;           /* (not read) */
  float* logp_log;   int64_t logp_ld;    /* DEVICE or NULL: (T, logp_ld) */
  float* value_log;  int64_t value_ld;   /* DEVICE or NULL: (T, value_ld); needs a critic */
  float* last_value_out;                 /* DEVICE or NULL: (n_envs,); needs a critic */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_rollout_actor_critic(mt_handle h, const struct mt_actor_critic* p);

/* An evolution-strategies generation: the planners' three levels (mt_sample_plans; mt_shoot; mt_cem / mt_mppi) in
 * PARAMETER space -- mt_es_sample perturbs, mt_rollout_population scores, mt_es runs the generation in one call.
 *
 * Population shape.  M members, M even, 2 <= M <= MT_ES_MAX_MEMBERS.  Member m owns the G = n_envs / M consecutive envs
 * [mG, (m+1)G) of the handle; G must be a multiple of 256, the rollout block, so that every block, and with it every
 * wave, belongs to one member and the weights stay wave-uniform scalar operands.  Anything else is MT_ERR_INVALID_ARG.
 * Flat parameters.  theta is P floats, W0 (n_out0 x IN) | b0 | W1 | b1 | W2 | b2, each W dense row-major (out, in): what
 * struct mt_policy's weight[l] / bias[l] point at, laid end to end.  IN, the widths, L, the activations, out_scale, lo, hi
 * and MT_POLICY_SEE_POSE are those of mt_rollout_policy.  A population is (M, pitch) f32 in DEVICE memory, pitch >= P,
 * the caller's workspace: no call allocates.
 * Perturbation (mt_es_sample).  Pair p = m >> 1, sign + for even m and - for odd m (antithetic).  eps(p, i) is the
 * Irwin-Hall variate of mt_cem -- (byte sum - 510) * KZ -- of word i & 3 of the Philox-4x32-10 block with counter
 * (p, 5 << 24, draw, i >> 2), key = seed: tag 5, the pair in the env's place.  pop[m][i] = theta[i] +- (sigma * eps): one
 * fp32 multiply, then one fp32 add or subtract, not fused.  sigma is one finite positive float.  One launch; words
 * [P, pitch) of a row are not written.
 * Scoring (mt_rollout_population).  mt_rollout_policy with one change: a block reads its member's weights, every weight
 * and bias pointer advanced by m * pitch.  No action noise (ES explores in parameter space).  The flags
 * (MT_POLICY_AUTO_RESET, _DRY_RUN, _SEE_POSE), the logs, return_out, the commit semantics, the refusals and legality
 * under capture are mt_rollout_policy's: env i of member m gets, bit for bit, what mt_rollout_policy gives env i with row
 * m as the weights.  fitness_out (needs return_out) adds one small launch: fitness[m] as defined below.
 * Update (mt_es): sample -> score -> update on the handle's stream, four launches, no host wait, no allocation.  The
 * caller supplies theta, the population, a (n_envs,) f32 return row (pop.return_out) and (M / 2 + M,) int64 words for
 * the coefficients and the sums; all are left filled.  R_i, the call's return of env i, is an integer-valued float, |R_i| <= 127 T < 2^24.
 *   S_m        = sum of R_i over member m, in int64 (the order is free)
 *   fitness[m] = (float)S_m * inv_G, inv_G the fp32 nearest to 1 / G: one conversion, one multiply
 *   best       = the lowest m with the largest S_m
 *   c_m        = MT_ES_SHAPE_RANK: 2 #{j : S_j < S_m} + #{j != m : S_j == S_m} (centred mid-ranks: ties favour neither
 *                half of a pair);  MT_ES_SHAPE_RAW: S_m.  A baseline cancels in an antithetic difference: none is taken.
 *   coeff[p]   = c_2p - c_2p+1
 *   A_i        = sum over p of coeff[p] * (bytesum(p, i) - 510), in int64
 *   grad[i]    = (float)A_i * scale, scale the fp32 nearest to the double KZ / (M sigma 2(M-1)) (rank) or
 *                KZ / (M sigma G) (raw), from the fp32 KZ and the fp32 sigma
 * The noise is regenerated from Philox: no (M, P) noise tensor exists.  grad_out is always written; with MT_ES_INPLACE
 * theta[i] += lr * grad[i], a multiply, then an add.  MT_ES_UPDATE_ONLY skips sample and score and takes pop.return_out as
 * the caller filled it (integer-valued, |R_i| <= 127 T): the update of returns shaped or gathered elsewhere.  The host
 * refuses M, G and T with which A_i could leave int64.  n_steps == 0 is a no-op. */
#define MT_ES_MAX_MEMBERS 4096
#define MT_ES_INPLACE     0x1u
#define MT_ES_UPDATE_ONLY 0x2u
enum { MT_ES_SHAPE_RANK = 0, MT_ES_SHAPE_RAW = 1 };
struct mt_es_sample {      /* as with mt_cem, the type is always written `struct mt_es_sample` */
  int32_t struct_size;     /* = sizeof(struct mt_es_sample), checked */
  int32_t n_members;       /* M */
  int64_t n_params;        /* P, 1..2^31 */
  const float* theta;      /* DEVICE f32 (P,) */
  float* pop;              /* DEVICE f32 (M, pitch): written; must not overlap theta */
  int64_t pitch;           /* floats between rows, >= P */
  float sigma;             /* finite, > 0 */
  uint32_t draw;           /* major counter word of the parameter-noise stream */
  uint64_t seed;
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_es_sample(mt_handle h, const struct mt_es_sample* s);

struct mt_population {     /* mt_policy with the weights taken from a population's rows, without sigma / draw */
  int32_t struct_size;     /* = sizeof(struct mt_population), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_members;       /* M */
  int32_t n_layers;        /* L, as mt_policy */
  int32_t width[2];
  int32_t hidden_act;
  int32_t out_act;
  const float* pop;        /* DEVICE f32 (M, pitch) */
  int64_t pitch;           /* >= P of the policy's shape */
  float out_scale, lo, hi;
  uint32_t flags;          /* MT_POLICY_* */
  float* action_log; int64_t act_ld;
  float* obs_log;    int64_t obs_ld;
  int8_t* reward_log; uint8_t* done_log; int64_t log_ld; float* return_out;   /* as mt_policy */
  float* fitness_out;      /* DEVICE or NULL: (M,) */
  uint64_t seed;           /* keys re-armed envs' targets */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_rollout_population(mt_handle h, const struct mt_population* p);

struct mt_es {
  int32_t struct_size;     /* = sizeof(struct mt_es), checked */
  int32_t shaping;         /* MT_ES_SHAPE_* */
  float sigma;             /* finite, > 0 */
  float lr;                /* finite; read with MT_ES_INPLACE */
  uint32_t draw;
  uint32_t flags;          /* MT_ES_* */
  float* theta;            /* DEVICE f32 (P,): read; updated with MT_ES_INPLACE */
  float* grad_out;         /* DEVICE f32 (P,): always written */
  int32_t* best_out;       /* DEVICE or NULL: (1,) */
  int64_t* coeff_out;      /* DEVICE int64 (M / 2 + M,): workspace, left holding coeff[p], p < M / 2, then S_m, m < M */
  struct mt_population pop; /* the scoring: pop.pop is the (M, pitch) workspace the sample writes, pop.return_out the
                              (n_envs,) return row (both required), pop.fitness_out the fitness; pop.seed keys the
                              parameter noise as well */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_es(mt_handle h, const struct mt_es* s);

/* The weighted log-likelihood gradient of the MLP policy: the gradient-based rung on top of mt_rollout_policy's logs
 * (REINFORCE with coef = reward-to-go, behaviour cloning of a planner's actions with coef = 1 and sigma = 1).
 *
 * Samples.  s = (t, i), t < n_steps, i < n_envs: x = obs[t, :, i] (IN floats, obs_log's layout), a = action[t, :, i]
 * (D floats, action_log's / mt_tape's layout), c = coef[t, i].
 * mu(x) is mt_rollout_policy's action before noise and clamp, out_scale * out_act(y_L): the same layers, activations and
 * tanh, evaluated with the same fmaf chains, so mu is bit for bit what mt_rollout_policy computes for that x.
 *   logp_s = -1/2 sum_j ((a_j - mu_j) / sigma_j)^2                 (constants dropped)
 *   grad   = scale * sum_s c_s d logp_s / d theta                   (P floats, mt_es's flat layout W0|b0|W1|b1|W2|b2)
 *   loss   = scale * sum_s c_s logp_s
 * with tanh' = 1 - h^2 taken from the forward value and relu' = 1 where the forward output is > 0, else 0.  action_log holds
 * CLAMPED actions; the likelihood ignores the clamp (a clamped a is scored as if the Gaussian had produced it).
 * Every sigma_j, j < D, must be finite and > 0 (MT_ERR_INVALID_ARG otherwise); behaviour cloning passes sigma = 1.
 * Skipped samples.  A sample contributes exactly nothing when c == 0 or when any a_j is unusable by the rule of every
 * tape (NaN, +-inf, beyond +-32768 degrees: the env held its pose): its x and a are then never read into the arithmetic,
 * NaN among them included.  This is how a caller masks the steps behind `done` (mt_reward_to_go's
 * MT_RTG_MASK_AFTER_DONE writes such zeros).
 * Contract.  Two launches on the handle's stream (one when n_steps == 0, which writes zeros), no allocation, no host
 * wait: legal under stream capture.  Nothing resident is read or written but the handle's shape (n_envs, K, D).
 * Everything the host can see is screened; grad_out, loss_out and the workspace must not overlap the weights, obs, action
 * or coef, nor each other.  The workspace holds per-block partial sums, mt_policy_grad_workspace() bytes (a function of
 * the handle's n_envs and device, the policy's shape and n_steps); a second pass adds them in ascending block order and
 * applies scale once.  No floating-point atomics: two calls with the same arguments on the same handle give the same
 * bits.  The bits may depend on n_steps, n_envs and the launch shape (the device's CU count); they do not depend on the
 * ld's, and a sample's contribution does not depend on the values of other samples.
 * No word outside the (out, in) matrices, the (out,) vectors and the first n_envs columns of each row of obs, action and
 * coef is read, whatever the widths (down to 1) and the ld's (>= n_envs). */
struct mt_policy_grad {    /* as with mt_cem, the type is always written `struct mt_policy_grad` */
  int32_t struct_size;     /* = sizeof(struct mt_policy_grad), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_layers;        /* L, as mt_policy */
  int32_t width[2];
  int32_t hidden_act;
  int32_t out_act;
  const float* weight[3];  /* DEVICE f32, as mt_policy */
  const float* bias[3];
  float out_scale;         /* finite */
  float sigma[MT_MAX_DOF]; /* per joint, degrees: finite, > 0 for j < D (entries behind D: finite, >= 0, not read) */
  uint32_t flags;          /* MT_POLICY_SEE_POSE only: it fixes IN */
  const float* obs;    int64_t obs_ld;    /* DEVICE (T, IN, obs_ld) */
  const float* action; int64_t act_ld;    /* DEVICE (T, D, act_ld) */
  const float* coef;   int64_t coef_ld;   /* DEVICE (T, coef_ld) f32: the weight c of sample (t, i) */
  float scale;             /* finite; applied once, at the final conversion */
  float* grad_out;         /* DEVICE f32 (P,): always written */
  float* loss_out;         /* DEVICE f32 (1,) or NULL */
  void* workspace;         /* DEVICE, 4-byte aligned; may be NULL when mt_policy_grad_workspace() is 0 */
  size_t workspace_bytes;  /* >= mt_policy_grad_workspace() */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_policy_grad(mt_handle h, const struct mt_policy_grad* p);
/* Bytes of workspace mt_policy_grad needs on this handle for a policy of that shape and n_steps (0 for n_steps == 0, and
 * for arguments mt_policy_grad would refuse). */
MT_API size_t mt_policy_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps);

/* The usual sample weights of mt_policy_grad from mt_rollout_policy's logs: the discounted reward-to-go.  One lane per env
 * runs backwards over t:  R_t = fmaf(gamma, done_t ? 0 : R_t+1, (float)r_t),  R_T = 0;  out[t, i] = R_t - baseline (one
 * fp32 subtraction).  gamma is an fp32 in [0, 1]; with gamma = 1 every R_t is an integer.  A done flag cuts the sum: with
 * MT_POLICY_AUTO_RESET the step behind it belongs to the next episode.  MT_RTG_MASK_AFTER_DONE, for logs without
 * auto-reset (the env steps on after its episode ended): every step behind the env's FIRST done gets exactly 0, which
 * mt_policy_grad skips.  One launch on the handle's stream, capturable; reads the first n_envs columns of the T rows. */
#define MT_RTG_MASK_AFTER_DONE 0x1u
struct mt_reward_to_go {   /* as with mt_cem, the type is always written `struct mt_reward_to_go` */
  int32_t struct_size;     /* = sizeof(struct mt_reward_to_go), checked */
  int32_t n_steps;         /* T, 0..65535; 0 is a no-op */
  const int8_t* reward_log;   /* DEVICE (T, log_ld) */
  const uint8_t* done_log;    /* DEVICE (T, log_ld) */
  int64_t log_ld;          /* >= n_envs */
  float gamma;             /* 0 <= gamma <= 1 */
  float baseline;          /* finite */
  float* out;              /* DEVICE f32 (T, out_ld) */
  int64_t out_ld;          /* >= n_envs */
  uint32_t flags;          /* MT_RTG_* */
  uint32_t reserved;       /* must be 0 */
};
MT_API int mt_reward_to_go(mt_handle h, const struct mt_reward_to_go* s);

/* The MLP's forward pass over logged observations: the mean of every sample and, given the logged actions, their
 * log-probability under the CURRENT weights -- what actor-critic and PPO need next to mt_policy_grad (the value of every
 * observation with a one-output head; the old and the new log-probability per sample).
 *
 * Samples, x and the layers are mt_policy_grad's.  The last layer has n_out outputs: 0 means the handle's D (a policy),
 * otherwise 1..MT_MAX_DOF (a value head has 1); IN does not depend on it.
 *   mean_out[t, j, i] = mu_j = out_scale * out_act(y_L)_j: the same helpers in the same order as mt_rollout_policy and
 *                       mt_policy_grad, so the same fmaf chains and the same bits for the same x.
 *   logp_out[t, i]    = -0.5f * lp,  lp = 0;  for j = 0 .. n_out-1:  e = a_j - mu_j;  d = e * inv_var_j;  lp = fmaf(e, d, lp)
 *                       with inv_var_j the fp32 nearest to 1 / sigma_j^2 (formed in double on the host): mt_policy_grad's
 *                       sequence, so its loss with a one-hot coef and scale = 1 is this number.
 * A sample with any unusable a_j (NaN, +-inf, beyond +-32768: the rule of every tape) gets logp exactly 0; its mean is
 * still written, mu does not depend on the action.
 * Contract.  At least one of mean_out and logp_out; logp_out needs action, and every sigma_j, j < n_out, finite and > 0
 * (entries behind n_out: finite, >= 0, not read; sigma is not read at all without logp_out).  Everything the host can see
 * is screened (MT_ERR_INVALID_ARG): the ld's >= n_envs, and an output may overlap neither the weights, obs, action nor the
 * other output.  Weights cannot be screened: a NaN among them goes through to the mean, as in the rollout.  One launch on
 * the handle's stream, no allocation, no host wait: legal under stream capture; n_steps == 0 is a no-op.  Nothing
 * resident is read but the handle's shape.  No word outside the (out, in) matrices, the (out,) vectors and the first
 * n_envs columns of each row of obs, action, mean_out and logp_out is read or written, whatever the widths (down to 1) and
 * the ld's. */
struct mt_policy_eval {    /* as with mt_cem, the type is always written `struct mt_policy_eval` */
  int32_t struct_size;     /* = sizeof(struct mt_policy_eval), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_layers;        /* L, as mt_policy */
  int32_t width[2];
  int32_t hidden_act;
  int32_t out_act;
  const float* weight[3];  /* DEVICE f32, as mt_policy; the last layer is (n_out, in) */
  const float* bias[3];
  float out_scale;         /* finite */
  uint32_t flags;          /* MT_POLICY_SEE_POSE only: it fixes IN */
  const float* obs;    int64_t obs_ld;    /* DEVICE (T, IN, obs_ld) */
  int32_t n_out;           /* outputs of the last layer: 0 = the handle's D, else 1..MT_MAX_DOF */
  float* mean_out;     int64_t mean_ld;   /* DEVICE or NULL: (T, n_out, mean_ld) */
  const float* action; int64_t act_ld;    /* DEVICE or NULL: (T, n_out, act_ld) */
  float sigma[MT_MAX_DOF]; /* read with logp_out: finite, > 0 for j < n_out */
  float* logp_out;     int64_t logp_ld;   /* DEVICE or NULL: (T, logp_ld) */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_policy_eval(mt_handle h, const struct mt_policy_eval* p);

/* Generalised advantage estimation over mt_rollout_policy's logs and a critic's values (mt_policy_eval with n_out = 1).
 * One lane per env runs backwards over t.  With gl the fp32 product gamma * lambda (formed once on the host),
 * V_T = last_value (0 when NULL), A_T = 0, and for t = T-1 .. 0:
 *   nv    = done_t ? 0 : V_t+1
 *   delta = fmaf(gamma, nv, (float)r_t) - V_t          (one fma, one fp32 subtraction)
 *   A_t   = fmaf(gl, done_t ? 0 : A_t+1, delta)        -> adv_out[t, i]
 *   ret_t = A_t + V_t                                  (one fp32 add) -> ret_out[t, i], the critic's regression target
 * weight_out gets 1.0f for every step.  MT_GAE_MASK_AFTER_DONE, for logs without auto-reset: every step behind the env's
 * FIRST done gets exactly 0 in adv_out, ret_out and weight_out and does not enter the recurrence (mt_reward_to_go's
 * mask); weight_out is then the `coef` that takes those steps out of mt_value_grad.  With lambda = 1, value all zeros and
 * last_value NULL adv_out is mt_reward_to_go's output for baseline 0 and the same mask, bit for bit.
 * gamma and lambda are fp32 in [0, 1].  value and last_value are device memory and cannot be screened.  One launch on the
 * handle's stream, capturable; reads and writes the first n_envs columns of the T rows only; the outputs may overlap
 * neither the inputs nor each other; n_steps == 0 is a no-op. */
#define MT_GAE_MASK_AFTER_DONE 0x1u
struct mt_gae {            /* as with mt_cem, the type is always written `struct mt_gae` */
  int32_t struct_size;     /* = sizeof(struct mt_gae), checked */
  int32_t n_steps;         /* T, 0..65535; 0 is a no-op */
  const int8_t* reward_log;   /* DEVICE (T, log_ld) */
  const uint8_t* done_log;    /* DEVICE (T, log_ld) */
  int64_t log_ld;          /* >= n_envs */
  const float* value;      int64_t value_ld;    /* DEVICE (T, value_ld): V of the observation step t started from */
  const float* last_value; /* DEVICE (n_envs,) or NULL (= 0): V of the state behind the last step */
  float gamma, lambda;     /* each in [0, 1] */
  float* adv_out;          int64_t adv_ld;      /* DEVICE (T, adv_ld): required */
  float* ret_out;          int64_t ret_ld;      /* DEVICE (T, ret_ld) or NULL */
  float* weight_out;       int64_t weight_ld;   /* DEVICE (T, weight_ld) or NULL */
  uint32_t flags;          /* MT_GAE_* */
  uint32_t reserved;       /* must be 0 */
};
MT_API int mt_gae(mt_handle h, const struct mt_gae* s);

/* The critic's regression gradient, on mt_policy_grad's kernels: the value head is an MLP of the policy's shape whose
 * last layer has ONE output, V = out_scale * out_act(y), and
 *   grad = scale * sum_s c_s (R_s - V_s) dV_s / dtheta          (P_v floats, the flat layout W0|b0|W1|b1|W2|b2)
 *   loss = scale * sum_s c_s (-1/2 (R_s - V_s)^2)
 * with R = target[t, i] and c = coef[t, i]: 1/2 c (R - V)^2 is mt_policy_grad's log-likelihood with one output, sigma = 1
 * and the target in the action's place, so theta += lr * grad DESCENDS the squared error (mt_policy_grad's sign).
 * The tape rule comes with the kernel: a sample with c == 0, or whose target is NaN, +-inf or beyond +-32768, contributes
 * exactly nothing and its x is never read (mt_gae's weight_out is such a c).  Determinism, the workspace
 * (mt_value_grad_workspace() bytes), the refusal of aliased buffers and legality under capture are mt_policy_grad's.
 * With MT_POLICY_SEE_POSE the handle's D must be 3, 4, 6 or 7 (the kernels read x as triples and at most one single word
 * when the last layer has one output); other joint counts are MT_ERR_UNSUPPORTED. */
struct mt_value_grad {     /* as with mt_cem, the type is always written `struct mt_value_grad` */
  int32_t struct_size;     /* = sizeof(struct mt_value_grad), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_layers;        /* L, as mt_policy; the last layer has one output */
  int32_t width[2];
  int32_t hidden_act;
  int32_t out_act;         /* MT_ACT_IDENTITY or MT_ACT_TANH */
  const float* weight[3];  /* DEVICE f32, as mt_policy */
  const float* bias[3];
  float out_scale;         /* finite */
  uint32_t flags;          /* MT_POLICY_SEE_POSE only: it fixes IN */
  const float* obs;    int64_t obs_ld;      /* DEVICE (T, IN, obs_ld) */
  const float* target; int64_t target_ld;   /* DEVICE (T, target_ld) f32: R, e.g. mt_gae's ret_out */
  const float* coef;   int64_t coef_ld;     /* DEVICE (T, coef_ld) f32: required */
  float scale;             /* finite; applied once, at the final conversion */
  float* grad_out;         /* DEVICE f32 (P_v,): always written */
  float* loss_out;         /* DEVICE f32 (1,) or NULL */
  void* workspace;         /* DEVICE, 4-byte aligned; may be NULL when mt_value_grad_workspace() is 0 */
  size_t workspace_bytes;  /* >= mt_value_grad_workspace() */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_value_grad(mt_handle h, const struct mt_value_grad* p);
/* Bytes of workspace mt_value_grad needs on this handle for a value head of that shape and n_steps (0 for n_steps == 0,
 * and for arguments mt_value_grad would refuse). */
MT_API size_t mt_value_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps);

/* PPO's clipped surrogate gradient in one pass over the logs: mt_policy_grad with the coefficient of every sample formed
 * in the kernel from its NEW log-probability (which the kernel holds anyway), the logged old one and the advantage --
 * instead of mt_policy_eval, four elementwise passes over (T, n_envs) and mt_policy_grad's second forward pass -- plus
 * what a PPO loop logs and what a learned exploration width needs.
 *
 * Samples, x, a, mu and the layers are mt_policy_grad's.  With lo = fl32(1 - (double)clip), hi = fl32(1 + (double)clip)
 * formed once on the host, per sample s = (t, i), all in fp32:
 *   A       = weight[t, i] * adv[t, i]                   (A = adv[t, i] without weight)
 *   skipped   when A == 0 or any a_j is unusable (the rule of every tape): x, a and old_logp of such a sample are never
 *             read into the arithmetic, NaN among them included.  Every other sample is USED.
 *   new     = mt_policy_eval's logp, bit for bit           (-0.5f * lp, lp by mt_policy_grad's fmaf chain)
 *   x       = min(max((new - old_logp[t, i]) + log_ratio_shift, -MT_PPO_MAX_LOG_RATIO), MT_PPO_MAX_LOG_RATIO)
 *   ratio   = exp(x)                                       (the hardware's exp2 of the rounded x * log2(e): about
 *                                                           1.2e-7 + 6e-8 |x| relative, the same bits for the same x)
 *   clipped = clip > 0 && ((A > 0 && ratio > hi) || (A < 0 && ratio < lo))
 *   c       = clipped ? 0 : ratio * A
 *   obj     = clipped ? (A > 0 ? hi : lo) * A : c          = min(ratio A, clamp(ratio, lo, hi) A)
 * and
 *   grad_out          = scale * sum_s c_s d logp_s / d theta: EXACTLY mt_policy_grad's grad_out for coef = c (the same
 *                       deltas, images, accumulation order, grid and reduction: bit for bit on the same handle)
 *   loss_out          = scale * sum_s obj_s                 (the surrogate objective; theta += lr * grad ascends it)
 *   kl_out            = scale * sum over used s of ((ratio - 1) - x)       (the k3 estimator of KL(old || new))
 *   sigma_grad_out[j] = scale * sum_s c_s fmaf(e_j, d_j, -1),  e_j = a_j - mu_j, d_j = e_j * inv_var_j: d / d log sigma_j
 *                       of the full Gaussian log-density (its normaliser included)
 *   count_out         = {used, clipped}: int64 counts, exact at any size
 *   ratio_out[t, i], coef_out[t, i] = ratio, c; a skipped sample gets 0 in both.
 * clip == 0 never clips: c = ratio * A, the importance-weighted policy gradient.  log_ratio_shift is
 * sum_j log(sigma_old_j / sigma_j) when sigma changed since old_logp was taken (logp drops the normaliser), else 0.
 * adv, old_logp and weight are device memory and cannot be screened: they are expected to be finite; a NaN or an infinity
 * among the USED samples leaves the sums unspecified.
 * Contract.  mt_policy_grad's: two launches on the handle's stream (one when n_steps == 0, which writes zeros to every
 * output given), no allocation, no host wait, legal under stream capture, no floating-point atomics -- the same arguments
 * give the same bits; the bits do not depend on the ld's.  Everything the host can see is screened: clip must be 0 or in
 * (0, 1), log_ratio_shift and scale finite, every ld >= n_envs, count_out 8-byte aligned, and no output may overlap the
 * weights, an input or another output (the workspace counts as an output).  The workspace holds
 * blocks x (P + 1 + MT_PPO_EXTRA_WORDS) words -- per block: the gradient, the objective, the KL sum, MT_MAX_DOF sigma sums
 * and the two counts -- mt_ppo_grad_workspace() bytes; the second launch adds the rows in ascending block order (the
 * counts as integers) and applies scale once.  Columns [n_envs, ld) of no row are read or written. */
#define MT_PPO_MAX_LOG_RATIO 20.0f
#define MT_PPO_EXTRA_WORDS (MT_MAX_DOF + 3)
struct mt_ppo_grad {       /* as with mt_cem, the type is always written `struct mt_ppo_grad` */
  int32_t struct_size;     /* = sizeof(struct mt_ppo_grad), checked */
  int32_t n_steps;         /* T, 0..65535 */
  int32_t n_layers;        /* L, as mt_policy */
  int32_t width[2];
  int32_t hidden_act;
  int32_t out_act;
  const float* weight[3];  /* DEVICE f32, as mt_policy: the network's matrices */
  const float* bias[3];
  float out_scale;         /* finite */
  float sigma[MT_MAX_DOF]; /* per joint, degrees: finite, > 0 for j < D (entries behind D: finite, >= 0, not read) */
  uint32_t flags;          /* MT_POLICY_SEE_POSE only: it fixes IN */
  const float* obs;      int64_t obs_ld;    /* DEVICE (T, IN, obs_ld) */
  const float* action;   int64_t act_ld;    /* DEVICE (T, D, act_ld) */
  const float* adv;      int64_t adv_ld;    /* DEVICE (T, adv_ld) f32: the advantages */
  const float* old_logp; int64_t old_ld;    /* DEVICE (T, old_ld) f32: mt_policy_eval's logp when the actions were taken */
  const float* sample_weight; int64_t weight_ld; /* DEVICE (T, weight_ld) f32 or NULL (= 1), e.g. mt_gae's weight_out */
  float clip;              /* 0 (no clipping) or in (0, 1) */
  float log_ratio_shift;   /* finite */
  float scale;             /* finite; applied once, at the final conversion */
  float* grad_out;         /* DEVICE f32 (P,): always written */
  float* loss_out;         /* DEVICE f32 (1,) or NULL */
  float* ratio_out;      int64_t ratio_ld;  /* DEVICE (T, ratio_ld) or NULL */
  float* coef_out;       int64_t coef_ld;   /* DEVICE (T, coef_ld) or NULL */
  float* sigma_grad_out;   /* DEVICE f32 (D,) or NULL */
  float* kl_out;           /* DEVICE f32 (1,) or NULL */
  int64_t* count_out;      /* DEVICE int64 (2,) or NULL: used, clipped */
  void* workspace;         /* DEVICE, 4-byte aligned; may be NULL when mt_ppo_grad_workspace() is 0 */
  size_t workspace_bytes;  /* >= mt_ppo_grad_workspace() */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_ppo_grad(mt_handle h, const struct mt_ppo_grad* p);
/* Bytes of workspace mt_ppo_grad needs on this handle for a policy of that shape and n_steps (0 for n_steps == 0, and for
 * arguments mt_ppo_grad would refuse). */
MT_API size_t mt_ppo_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps);

/* Environment.get_observations(), manytor.py:141-153, at the current pose (also
 * zeroes the coordinates of dead targets, :148).  Result in MT_F_OBS. */
MT_API int mt_observe(mt_handle h);
/* Environment.is_done(), manytor.py:155-173, at the current pose. Result in MT_F_DONE. */
MT_API int mt_check_done(mt_handle h);

/* Copy a field out in the reference's env-major shape (see mt_field) to host
 * (is_device = 0, synchronises) or device memory.  dst_bytes must match. */
MT_API int mt_get(mt_handle h, int field, void* dst, int64_t dst_bytes, int is_device);
/* Overwrite GOALS / POINTS / ALIVE(u8 N,K) / TOTAL_REWARD from host env-major
 * arrays (attribute assignment on the reference objects, e.g. manytor.py:243), and -- for restoring a checkpoint --
 * DONE (u8 N; the ballot words are rebuilt), EPISODES (u32 N), LAST_RETURN (f32 N), RETURN_RING (f32 N,R).
 * Floating-point input is screened: NaN / +-inf anywhere, or a joint angle beyond +-32768 degrees, is
 * MT_ERR_INVALID_ARG and nothing is written (the kernels assume finite state).  A pose anywhere inside +-32768
 * degrees is stepped from with the accuracy of one inside +-180. */
MT_API int mt_set(mt_handle h, int field, const void* src, int64_t src_bytes);
/* The episode index every env was given by the last full reset (finished-episode counts and return-ring slots are
 * relative to it): mt_reset / mt_reset_random set it; a checkpoint restore sets it back with this call. */
MT_API int mt_set_episode_base(mt_handle h, uint32_t episode0);
/* Raw resident buffer: pointer to row 0, number of rows, row stride in elements and element dtype.  Writing through the
 * pointer is the caller's business (order it with the handle's stream).  Asking for MT_F_GOALS tells the library that
 * joint angles may change behind its back: from then on it never assumes them to be whole degrees (the table look-up
 * the sampled-action kernels use for the pose a step starts from is replaced by the computed sines / cosines). */
MT_API int mt_device_ptr(mt_handle h, int field, void** ptr, int64_t* rows, int64_t* ld, int* dtype);

/* Inverse kinematics of the pickup frame: which joint angles put the hand on that point?  Not in the reference (it has no
 * solver; its targets are met by sampled actions, test_multi.py:19-21).
 * The driven point p(q) is the origin of the frame the pickup test uses (mt_config.ee_frame, resolved as everywhere: for
 * the built-in tables the frame after all D joints).  MT_ERR_UNSUPPORTED when ee_frame resolves to the origin row: that
 * point does not move.  With joint j at theta_j = q_j + off_j, z_j and o_j the Z axis and the origin of the frame BEFORE
 * joint j (z_0 = (0, 0, 1), o_0 = 0), column j of the position Jacobian is z_j x (p - o_j) per radian for every joint up to
 * the last one the driven frame depends on and exactly 0 for later joints.
 *
 * mt_jacobian: jac_out[(3 j + a) * jac_ld + i] = d p_a / d q_j of env i per DEGREE (the per-radian column times pi / 180),
 * pos_out[a * pos_ld + i] = p_a (optional).  angles is DEVICE (D, angles_ld) f32 degrees, or NULL: the resident pose
 * MT_F_GOALS (MT_ERR_STATE before a reset).  One launch on the handle's stream; nothing resident is written.
 *
 * mt_ik: `iters` damped-least-squares iterations per env in ONE launch.  One iteration, J per radian at the current q:
 *   e = x - p(q);  A = J J^T + damping^2 I_3;  y = A^-1 e;  dq = (180 / pi) J^T y;
 *   m = max_j |dq_j|;  if m > max_step_deg: dq *= max_step_deg / m;  q += dq
 * in fp32 with a fixed operation order: an env's result depends on its own inputs only (not on the batch, its neighbours
 * or the row pitches), and two calls give the same bits.
 * Early stop (tol > 0): an env whose box residual max(|e_x|, |e_y|, |e_z|) -- the pickup test's metric -- is <= tol BEFORE
 * an iteration takes no further step; its angles are, bit for bit, those of a call with that many iterations.
 * Target: x = target[a * target_ld + i], or with target NULL the alive target of env i with the smallest squared Euclidean
 * distance from p at the START pose (the lowest index wins a tie), read from MT_F_POINTS and the alive mask;
 * index_out[i] names it.  An env without an alive target gets index -1, its start angles bit for bit, residual 0, 0 steps.
 * Start: start[j * start_ld + i], or with start NULL the resident pose MT_F_GOALS.
 * An env with a non-finite target coordinate or an unusable start angle (NaN, +-inf, beyond +-32768 degrees) is held the
 * same way with residual NaN; no other env's outputs change.
 * Results: angles_out[j * angles_ld + i] (the layout of MT_F_ACTIONS and of one step of mt_policy.action_log) is the final
 * q -- with MT_IK_WRAP mapped into [-180, 180), the reference's action domain (manytor.py:216); without it continuous
 * from the start pose, the short route for mt_step's interpolation -- residual_out[i] the box residual at the angles
 * written (one more forward pass), iters_out[i] the steps taken.  Any output may be NULL; all NULL without MT_IK_STAGE is
 * refused.  MT_IK_STAGE also writes the angles to MT_F_ACTIONS: the next mt_step executes them, exactly as after
 * mt_set_actions with the same angles.  Nothing else resident is written.
 * Everything the host can see is screened before any launch (MT_ERR_INVALID_ARG; every ld >= n_envs; index_out with an
 * explicit target); MT_ERR_STATE before a reset whenever the call reads or stages resident state (target NULL, start
 * NULL, MT_IK_STAGE).  One launch on the handle's stream, no allocation, no host wait: legal under stream capture. */
#define MT_IK_STAGE 0x1u       /* also write the angles to MT_F_ACTIONS */
#define MT_IK_WRAP  0x2u       /* angles mapped into [-180, 180) */
#define MT_IK_MAX_ITERS 255
struct mt_ik {             /* as with mt_cem, the type is always written `struct mt_ik` */
  int32_t struct_size;     /* = sizeof(struct mt_ik), checked */
  int32_t iters;           /* 1..MT_IK_MAX_ITERS */
  float damping;           /* lambda, finite, > 0, in length units */
  float max_step_deg;      /* finite, > 0: the largest joint move of one iteration */
  float tol;               /* finite, >= 0: box residual at which an env stops; 0 = never stop early */
  uint32_t flags;          /* MT_IK_* */
  const float* target; int64_t target_ld;   /* DEVICE (3, target_ld) x / y / z, or NULL: each env's nearest alive target */
  const float* start;  int64_t start_ld;    /* DEVICE (D, start_ld) degrees, or NULL: MT_F_GOALS */
  float* angles_out;   int64_t angles_ld;   /* DEVICE (D, angles_ld) or NULL */
  float* residual_out;     /* DEVICE f32 (n_envs,) or NULL */
  int32_t* iters_out;      /* DEVICE i32 (n_envs,) or NULL */
  int32_t* index_out;      /* DEVICE i32 (n_envs,) or NULL; nearest-target mode only */
  uint64_t reserved;       /* must be 0 */
};
MT_API int mt_ik(mt_handle h, const struct mt_ik* s);
/* (angles, jac_out and pos_out are DEVICE f32 rows handed over as void*, like mt_sample_plans' block: device memory cannot
 * be screened on the host.  An unusable angle gives that env's own outputs unspecified values and touches nothing else.) */
MT_API int mt_jacobian(mt_handle h, const void* angles, int64_t angles_ld, void* jac_out, int64_t jac_ld, void* pos_out,
                       int64_t pos_ld);

/* ---- multi-GPU: the one exchange of the path ---------------------------------------------------
 * Envs share nothing, so stepping needs no collective.  What is exchanged is what test_multi.py:32 prints: the
 * per-env return, all-gathered over the ranks (one process per GPU) with RCCL over xGMI, straight out of the
 * arena on the handle's stream -- no staging copy, no host round trip.  librccl.so is dlopen'ed on first use, so the
 * library loads and runs on a box without RCCL.
 *   rank 0: mt_comm_unique_id(id)  ->  ship the 128 bytes to the other ranks by any means (the Python host uses the
 *   torch.distributed store)  ->  every rank: mt_comm_init(h, id, rank, world)  [collective, ncclCommInitRank]. */
MT_API int mt_comm_unique_id(void* id_out /* MT_UNIQUE_ID_BYTES */);
MT_API int mt_comm_init(mt_handle h, const void* unique_id, int rank, int world_size);
MT_API int mt_comm_destroy(mt_handle h);
/* All-gather row `row` of a single-precision field (MT_F_TOTAL_REWARD, MT_F_LAST_RETURN: row 0; MT_F_RETURN_RING: a
 * slot) of every rank into dst (device memory, global env order, dst_elems = total number of envs over all ranks;
 * shards may differ in size).  Asynchronous on the handle's stream.  Without mt_comm_init (one GPU) it is a
 * device-to-device copy. */
MT_API int mt_gather_returns(mt_handle h, int field, int row, float* dst, int64_t dst_elems);
/* The same exchange taken off the handle's stream: the row is snapshotted on the handle's stream (so a reset queued
 * next may overwrite it), the all-gather runs on a side stream of the handle, and the call returns at once -- steps and
 * resets queued afterwards overlap with the exchange over xGMI.  mt_gather_returns_wait orders the handle's stream
 * behind the last begun gather; with host_wait != 0 it also blocks the calling thread until dst is complete and, if
 * elapsed_ms is not NULL, reports the device time the exchange took (if mt_sync has already waited for it: the time
 * of that last completed exchange).  dst must not be read, and the communicator not destroyed, before that.  mt_sync
 * also waits for a begun gather.
 * Several gathers may be begun without a wait in between (each with a dst of its own): they run one after the other on the
 * side stream.  The snapshot is double-buffered, and where mt_rollout writes it itself (its last launch, small batches)
 * mt_gather_returns_begin lets the calling thread run at most ONE exchange ahead of the device: if the exchange before the one
 * just begun has not finished yet it waits for it (the device still holds a whole episode of queued work then), so that the
 * next episode needs neither a snapshot launch nor a stream wait between its steps and the gather.  MT_GATHER_THROTTLE=0
 * never waits (the snapshot is then a launch of its own whenever the host is further ahead).
 * On a caller's stream (mt_set_stream), and while that stream is being captured, mt_rollout does not write the snapshot and
 * this call always copies the row in stream order: a write queued on that stream between the two calls (a torch op on a
 * mt_device_ptr view, say) is part of what is gathered. */
MT_API int mt_gather_returns_begin(mt_handle h, int field, int row, float* dst, int64_t dst_elems);
MT_API int mt_gather_returns_wait(mt_handle h, int host_wait, float* elapsed_ms);
/* The same without the snapshot: the exchange on the side stream reads the arena row itself, so nothing is copied on the
 * handle's stream.  Meant for MT_F_LAST_RETURN right after the reset that ended an episode (the reset stores every env's
 * finished return there): that row is written by resets only, and the library orders every later reset / re-arm of its
 * own behind the exchange.  For any other row the caller must not let it change before mt_gather_returns_wait. */
MT_API int mt_gather_returns_begin_inplace(mt_handle h, int field, int row, float* dst, int64_t dst_elems);
/* Total number of envs over all ranks of the communicator (n_envs without one). */
MT_API int mt_comm_total_envs(mt_handle h, int64_t* total);
/* Summary of a return row over ALL ranks without moving the row (what a learner logs per episode):
 * sum / min / max of row `row` of `field` (as for mt_gather_returns), the number of envs, and how many of them have
 * their done flag set.  Reduced on the device (double accumulation, fixed order: the same bits on every rank and from
 * run to run), five numbers per rank exchanged over the communicator (all-gather), combined on the host.
 * Synchronous on the handle's stream; collective when a communicator is attached. */
typedef struct mt_return_stats {
  double sum, min, max;
  int64_t count; /* envs over all ranks */
  int64_t done;  /* of which MT_F_DONE != 0 */
} mt_return_stats;
MT_API int mt_reduce_returns(mt_handle h, int field, int row, mt_return_stats* out);

/* HIP-event timer on the handle's stream (wall-clock of test_multi.py:16-18, device side).  Start and stop join the chains
 * but do not launch a deferred mt_reset_random: the next mt_rollout absorbs it INSIDE the timed region. */
MT_API int mt_timer_start(mt_handle h);
MT_API int mt_timer_stop(mt_handle h, float* elapsed_ms);
/* The same end mark WITHOUT joining the chains and without a host wait: one end event on every stream of the handle
 * that may still carry work (its stream, the chain streams while forked); mt_timer_read waits for them and returns the
 * time from mt_timer_start to the LAST of them -- and to the end of an exchange begun with mt_gather_returns_begin that
 * was still pending at the mark.  bench.py brackets each timed region with the pair to report the region's device
 * timeline next to its wall clock. */
MT_API int mt_timer_stop_async(mt_handle h);
MT_API int mt_timer_read(mt_handle h, float* elapsed_ms);
/* Lap timer: any number of begin/end event pairs recorded on the stream WITHOUT host synchronisation;
 * mt_timer_laps_total synchronises once, returns the summed device time of all laps and clears them.  Lets a
 * benchmark time only its step launches inside a longer region without stalling the GPU at every lap.  A lap begins behind
 * everything queued before it (a deferred reset is launched first); while the chains are forked on the handle's own stream it
 * has one begin event per chain and runs from the earliest of them to the latest end event -- no join for the stopwatch. */
MT_API int mt_timer_lap_begin(mt_handle h);
MT_API int mt_timer_lap_end(mt_handle h);
MT_API int mt_timer_laps_total(mt_handle h, float* total_ms, int* n_laps);
/* The same, one figure per lap in recording order (ms[0 .. *n_laps)); clears the laps.  With capacity smaller than the
 * number of laps it only reports *n_laps and fails, leaving the laps in place. */
MT_API int mt_timer_lap_times(mt_handle h, float* ms, int capacity, int* n_laps);

/* Stateless kinematics helpers = the module functions of the reference.
 * mt_fk_batch: fk(mode, goals), manytor.py:35-53 -> 4x4 row-major per pose; with
 * dof = mode = 1, angles_in_radians = 1 it is dh(a, alfa, d, theta), manytor.py:25-32.
 * mt_r_theta_batch: r_theta(v1, v2), manytor.py:17-22 -> (r_deg, theta_deg).
 * Host pointers in, host pointers out; run on `device`. */
MT_API int mt_fk_batch(int device, const float* dh_table, int dof, int mode, const float* angles, int angles_in_radians,
                int64_t n, float* out_mat16);
/* joints_coordinates at each of the `substeps` poses of the straight joint-space route prev -> action
 * (manytor.py:182-190; what the reference appends to `trajectory` and streams to its viewer): host (n, dof) in,
 * host (n, substeps, dof, 3) out.  Off the step path; meant for the few envs one draws or logs. */
MT_API int mt_route_trace(int device, const float* dh_table, int dof, int substeps, const float* prev,
                          const float* action, int64_t n, float* out);
MT_API int mt_r_theta_batch(int device, const float* v1, const float* v2, int64_t n, float* out_r_theta);
/* Measurement aid ("report against the measured bandwidth"): a streaming kernel with exactly the memory
 * operations of one mt_step_random -- dof + 3 targets + 2 rows read, dof + 2 rewritten in place, 3 targets + 4 rows and
 * one byte row written non-temporally, one env per lane, the arena's row pitch -- and none of its arithmetic, run `reps`
 * times over n_envs envs.  us_per_pass = average device time of a pass, bytes_per_pass = (8 dof + 24 targets + 33) x
 * n_envs.  Built for (dof, targets) = (4, 7), (7, 7), (4, 10); allocates and frees its own buffers. */
MT_API int mt_stream_probe(int device, int dof, int n_targets, int64_t n_envs, int reps, float* us_per_pass,
                           int64_t* bytes_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* MANYTOR_HIP_H */
