// libmanytor_hip.so -- host side of the C ABI declared in include/manytor_hip.h.
//
// Owns the device arena (SoA rows in HBM), the stream, and the launch logic.
// No arithmetic of the step path happens here: everything the reference
// computes in manytor.py:17-53,141-260 runs in the kernels of kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"
#include "table_dispatch.h"

using namespace mt;

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace mt {
int fail(mt_handle h, int code, const std::string& msg) {
  if (h)
    h->err = msg;
  else
    g_last_error = msg;
  return code;
}

int join_chains(mt_handle h) {
  if (!h->forked) return MT_OK;
  h->forked = false;
  for (int c = 1; c < mt_engine::kMaxChains; ++c) {
    if (!h->chain_streams[c] || !h->ev_join[c]) continue;
    MT_HIP(h, hipEventRecord(h->ev_join[c], h->chain_streams[c]));
    MT_HIP(h, hipStreamWaitEvent(h->stream, h->ev_join[c], 0));
  }
  return MT_OK;
}
}  // namespace mt

namespace {

DhConst make_dh(const float* table, int dof) {
  DhConst t{};
  for (int j = 0; j < MT_MAX_DOF; ++j) {
    t.ca[j] = 1.f;
  }
  for (int j = 0; j < dof; ++j) {
    const double a = table[4 * j + 0], alpha = table[4 * j + 1], d = table[4 * j + 2], off = table[4 * j + 3];
    t.a[j] = (float)a;
    t.d[j] = (float)d;
    // snap multiples of pi/2 so that e.g. cos(pi/2) is 0, not 6e-17 (the reference's residue)
    double sa = std::sin(alpha), ca = std::cos(alpha);
    if (std::fabs(sa) < 1e-7) sa = 0.0;
    if (std::fabs(ca) < 1e-7) ca = 0.0;
    t.sa[j] = (float)sa;
    t.ca[j] = (float)ca;
    t.off_deg[j] = (float)(off * 180.0 / M_PI);
  }
  t.fo = dof >= 2 ? dof - 2 : 0;  // the reference's rows (manytor.py:143, :162); mt_create overrides them from mt_config
  t.fe = dof - 1;
  return t;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int ensure_staging(mt_handle h, size_t bytes) {
  if (h->staging_bytes >= bytes) return MT_OK;
  if (h->staging) {
    MT_HIP(h, hipStreamSynchronize(h->stream));
    MT_HIP(h, hipFree(h->staging));
    h->staging = nullptr;
    h->staging_bytes = 0;
  }
  if (hipMalloc(&h->staging, bytes) != hipSuccess) return fail(h, MT_ERR_ALLOC, "hipMalloc(staging) failed");
  h->staging_bytes = bytes;
  return MT_OK;
}

// ---- kernel dispatch ---------------------------------------------------------------------------
// static_kind: 0 = runtime table (RtTable<D>), 1 = Ref4Table, 2 = Dh7Table
template <class Tbl>
bool table_matches(const DhConst& t, int dof) {
  if (dof != Tbl::D) return false;
  for (int j = 0; j < dof; ++j)
    if (t.a[j] != Tbl::a(j) || t.d[j] != Tbl::d(j) || t.sa[j] != Tbl::sa(j) || t.ca[j] != Tbl::ca(j) ||
        t.off_deg[j] != Tbl::off(j))
      return false;
  return true;
}

int match_static(const DhConst& t, int dof) {
  if (table_matches<Ref4Table>(t, dof)) return 1;
  if (table_matches<Dh7Table>(t, dof)) return 2;
  return 0;
}

// ---- the dispatch policy: ONE table of every size threshold the host picks a schedule by ------------------------------
// Every schedule of a kernel gives the same bits (tests/test_gpu_parity.py: test_step_kernel_variants_are_bit_identical,
// test_rollout_in_independent_chains_equals_plain_launches, ...), so this table is about time only.  The numbers come from
// the sweeps named beside them (tools/variant_sweep.py, size_sweep.py, chain_sweep.py, fused_split_sweep.py,
// ab_blocks_per_cu.sh; profiles/r02_variants.md, r03_variants.md, r04_variants.md).  choose_dispatch() below is the only
// reader; the MT_* environment variables override single entries for experiments and tests, and mt_describe_dispatch()
// reports the table, the overrides and what was resolved for a handle.
struct BlockCap {
  int64_t from, below;  // envs of the launch
  int blocks;           // resident blocks per CU
};
struct DispatchPolicy {
  // step_split_kernel: one env over 4 / 2 lanes while the batch is so small that a launch is one wave's dependent chain
  //   <= 49 152 arms: 4.5-5.5 us per step against 5.3-5.9 with prefetch (49 152: 5.47 against 5.70 with 2 lanes);
  //   <= 65 536: 5.8 against 6.0 (4 lanes: 6.3)                                  [profiles/r03_variant_sweep_final.json]
  int64_t step_split4_max = 49152, step_split2_max = 65536;
  // prefetch (PF = 8) for arms other than the reference arm: up to here (long arms lose more to the lower occupancy than
  // they gain); the reference arm takes it at every size (7.1 against 7.8 us at 131 072, 19.9 against 21.0 at 524 288)
  int64_t prefetch_other_max = 131072;
  // rollout_split_kernel (fused rollout): 4 lanes per env up to 32 768 arms, 2 up to 131 072 (3.60 against 4.50 us per step
  // at 98 304 arms, 4.37 against 4.50 at 131 072; one env per lane wins from 196 608 on)   [r03_fused_split_sweep.json]
  int64_t fused_split4_max = 32768, fused_split2_max = 131072;
  // reset_split_kernel: the target draw over 4 lanes per env (11.2 -> 6.9 us at 16 384 arms, 12.1 -> 10.0 at 65 536, a tie
  // at 131 072, slower above)
  int64_t reset_split_max = 65536;
  // mt_rollout replays a cached HIP graph of its launches up to here (-3..6 % per step; nothing above, where the kernels
  // are the time)                                                                        [r02_graph_replay.json]
  int64_t graph_max = 131072;
  // mt_rollout / mt_step as two chains of launches on two streams (us per step incl. the per-episode reset, one chain ->
  // two: 163 840 envs 8.45 -> 7.15, 262 144: 10.5 -> 8.7, 524 288: 21.5 -> 19.8, 1 M: 39.9 -> 36.3, 2 M: 74.6 -> 69.0;
  // nothing at 4 M; at 98 304-131 072 two chains win back to back but lose from an idle device)     [r03_variants.md 2]
  int64_t chains_min = 163840, chains_max = 3145728;
  // a chain is a batch of span envs, but two kernels are in flight, so the lane-split schedules stop paying earlier
  // (2 x 65 536 envs: 6.85 us with one env per lane against 7.0-7.35 with two lanes; 2 x 49 152: 6.8 with two against 6.95)
  int64_t chain_split4_max = 16384, chain_split2_max = 49152, chain_prefetch_other_max = 131072;
  // launches of the prefetch kernel over at least this many envs take LaneOffset<false> (kernels.h FLAT: the HBM-bound
  // regime, 0.7-2.4 % faster there)                                                      [r03_ab_flat_from.txt]
  int64_t flat_from = 393216;
  // resident blocks per CU of a CHAIN launch of the sampled-action PF + TT kernel (74-76 VGPRs: six fit), keyed by the
  // envs of the launch with two chains in mind (us per step of the batch, no cap -> cap: 327 680 arms 12.3 -> 11.6 (3),
  // 393 216: 14.4 -> 13.3 (3), 524 288: 19.1 -> 18.0 (4), 786 432: 27.4 -> 26.1 (4), 1 048 576: 35.2 -> 34.5 (5); nothing
  // at >= 1 179 648 and <= 262 144 arms)                                                 [r03_variants.md 12]
  BlockCap block_caps[3] = {{147456, 229376, 3}, {229376, 458752, 4}, {458752, 589824, 5}};
  // mt_rollout(T) exposes the state after T steps and the outputs of the last one, so on small shards -- where a launch
  // per step is a kernel boundary plus a re-fetch of the whole state past L2 for 4-6 us of work -- it runs
  // `multi_step_k` steps per launch through the rollout kernels (state in registers / LDS between them; every step
  // still writes its obs / reward / done / ee), bit-identical by construction             [r04_variants.md 1]
  //   us per step, 50-step segments from an idle device (tools/rollout_k_sweep.py, profiles/r04_rollout_k_sweep*.json):
  //                 one launch per step (default of round 3)      k = 4     k = 5     k = 8     k = 50
  //      65 536 envs   5.71 (graph replay)                         4.18      3.99      3.74      3.04
  //      98 304        6.48 (graph replay)                         4.96      4.70      4.35
  //     131 072        6.47 (graph replay)                         5.79      5.50      5.10      4.42
  //     163 840        7.43 (two chains of step kernels)           6.59      6.26      5.88
  //     196 608        8.32 (two chains)                           6.74      6.35      5.97
  //     262 144        8.09 (two chains)                           8.03      7.64      7.27
  //   (k = 2 loses at 131 072: a rollout-kernel launch costs 4-6 us before its first step's outputs.)  The multi-step
  //   launches run on the handle's stream alone: in two chains they are faster back to back at 131 072-163 840 envs
  //   (4.78 / 5.88 us) but slower from an idle device over a 20-step segment (5.83 / 6.81) and slower at >= 196 608.
  int64_t multi_step_max = 262144;
  int multi_step_k = 5;
  // the chained launch-per-step form of the large batches starts an episode with ONE step of the rollout kernel that carries
  // the deferred reset as its prologue
  bool fold_reset_into_chains = false;
  // the angle-addition recurrence is run (S - 1) / 2 rotations from each end of a route; beyond this many the per-pose
  // polynomial sincos kernels take over (drift: 12 rotations 3.3e-5 / 6.6e-5 in z on the 4- / 7-joint arm, 31 rotations
  // 8.6e-5 / 1.3e-4, outside the 1e-4 position tolerance)                                [tests/test_gpu_zmin.py]
  int max_recurrence_rotations = 12;
  // sampled step launches of the code-reading prefetch kernels re-derive the pose they start from (the zero pose of a full
  // reset, or the previous launch's action draw: kernels.h PREV) instead of loading it: 4 D of the 208 B an env-step moves,
  // for one more Philox block per env.  Per compile-time table:
  //   reference arm: the rows keep their 62-64 VGPRs and 8 waves per SIMD                [profiles/goal_rederive_ab.txt]
  //   7-joint table: its launches take the prefetch kernel up to 131 072 envs only, where a launch is not HBM-bound, and
  //   the rows go from 62-63 to 68-70 VGPRs (8 -> 7 waves per SIMD): us per step of the one-chain launch-per-step form
  //   (MT_ROLLOUT_K=1 MT_GRAPH=0), 7 alternating passes of 400 steps, loaded -> re-derived: 70 001 envs 7.85 -> 8.21,
  //   131 072 envs 8.27 -> 8.56 (ranges disjoint): off; MT_GOALS_REDERIVE=1 turns it on  [profiles/goal_rederive_dh7.json]
  bool rederive_goals_ref4 = true;
  bool rederive_goals_dh7 = false;
  // ... and, on a multi-chain handle, by the launches of this many of its chains only (the others keep loading).  Every chain
  // re-deriving (MT_GOALS_REDERIVE=1) takes bench.py --full's step lap of 1 M reference arms from 32.3-32.6 to 30.0-30.2 us
  // (three alternating rounds): below the 30.54 us at which its roofline.frac, computed on a fixed 233 model bytes per env-step
  // for 8 TB/s, reaches 1 (measured 1.012-1.018) -- a figure tests/test_bench_contract.py holds at <= 1 -- although the
  // launches then move 196 B.  One chain of two: lap 31.6 us, frac 0.966-0.967, headline +3.2 % instead of +5.9 %.  A stop-gap:
  // raise this to kMaxChains once the model bytes follow the kernels                       [profiles/goal_rederive_ab.txt]
  int rederive_goals_chains = 1;
  // ... and by launches of at most this many envs (= chains_max: beyond it a step is ONE launch of the whole batch).  The same
  // kind of stop-gap: at 4 M arms bench.py compares the step with a stream probe of the 233-byte access shape, and the
  // re-deriving launch, which moves less than the probe, lands on both sides of it (frac_of_achievable 0.96-1.03 in four runs,
  // the parent 0.93-0.97; us per step 181.9 -> 179.0, -1.6 %); test_bench_contract.py holds that figure at <= 1 as well
  int64_t rederive_goals_max_envs = 3145728;
  // rows of more than this many envs get a 1 KiB pad (rows an exact power of two apart alias onto the same channels)
  int64_t ld_pad_above = 16384;
  int ld_pad_floats = 256;
};
static const DispatchPolicy kPolicy{};

// Blocks per CU for a chain launch of the sampled-action prefetch kernel of a compile-time table.  The cap is applied at
// launch time the usual way, with dynamic LDS nobody touches: a block then claims 1 / cap of the CU's 160 KB.
// MT_BLOCKS_PER_CU overrides (0 = none; 1 and 2 cannot be realised inside the default 64 KB dynamic-LDS limit and are
// raised to 3).
static int step_blocks_per_cu(const mt_engine* h, int64_t n_launch) {
  if (h->blocks_per_cu_override >= 0) return h->blocks_per_cu_override;
  if (n_launch >= h->n) return 0;  // chain launches only
  for (const BlockCap& c : kPolicy.block_caps)
    if (n_launch >= c.from && n_launch < c.below) return c.blocks;
  return 0;
}
static size_t lds_pad_for_blocks(int blocks_per_cu, size_t static_lds) {
  if (blocks_per_cu <= 0) return 0;
  const size_t per_block = (size_t)163840 / (size_t)blocks_per_cu - 1024;  // safely inside the bracket of that block count
  return per_block > static_lds ? std::min<size_t>(per_block, 65536) - static_lds : 0;  // <= 64 KB in all: no attribute needed
}

// Envs per chain: equal shares rounded up to whole 256-env blocks; the last chain takes what is left (possibly less).
int64_t chain_span(const mt_engine* h, int chains) {
  const int64_t per = (h->n + chains - 1) / chains;
  return (per + 255) / 256 * 256;
}

static bool env_int(const char* name, long long* v) {  // set AND non-empty (atoi("") would read as 0)
  const char* e = std::getenv(name);
  if (!e || !*e) return false;
  *v = std::atoll(e);
  return true;
}

// Every schedule choice of a handle, from kPolicy, the handle's size / table / flags (h->cfg, h->args.dh must be set) and
// the MT_* overrides.  Called once by mt_create.  The overrides that were seen are kept in h->overrides for
// mt_describe_dispatch.
static void choose_dispatch(mt_handle h) {
  const mt_config* cfg = &h->cfg;
  const DispatchPolicy& P = kPolicy;
  const int64_t n = cfg->n_envs;
  long long v = 0;
  h->overrides.clear();
  // (the value as it was PARSED, never the raw text: mt_describe_dispatch pastes this into a JSON string)
  auto seen = [&](const char* name) { h->overrides += (h->overrides.empty() ? "" : ",") + std::string(name) + "=" + std::to_string(v); };

  h->trig = (cfg->flags & MT_FLAG_HW_TRIG) ? 2 : ((cfg->flags & MT_FLAG_DIRECT_TRIG) ? 1 : 0);
  if (cfg->flags & MT_FLAG_ABLATE_LOOP) h->trig = (cfg->flags & MT_FLAG_ABLATE_OBS) ? 4 : 3;
  else if (cfg->flags & MT_FLAG_ABLATE_OBS) h->trig = 5;   /* OBS alone = arithmetic-only build */
  // Routes with more rotations per half than the recurrence tolerates take the per-pose polynomial sincos (the
  // MT_FLAG_DIRECT_TRIG kernels: no drift, about twice the arithmetic).
  const bool long_route = h->trig == 0 && (cfg->substeps - 1) / 2 > P.max_recurrence_rotations;
  if (long_route) h->trig = 1;
  h->lds_table = (cfg->flags & MT_FLAG_DH_IN_LDS) != 0 && !long_route;  // the LDS-table variant exists for the recurrence only
  // other rows than the reference's last two: the runtime-table kernel with runtime frames (RtTableF), one env per lane
  h->custom_frames = !(h->args.dh.fo == h->D - 2 && h->args.dh.fe == h->D - 1);
  h->static_kind = ((cfg->flags & (MT_FLAG_NO_SPECIALIZE | MT_FLAG_DH_IN_LDS)) || h->custom_frames) ? 0 : match_static(h->args.dh, h->D);

  // ---- one launch per step: which step kernel for which batch (all variants give the same bits) ----
  // (the schedules themselves are filled at the end, once the chain count is known: schedule_for)
  int forced_lanes = 0, forced_prefetch = -1;  // MT_SPLIT (step and rollout kernels alike) / MT_PREFETCH, for every scope
  if (env_int("MT_SPLIT", &v)) {
    forced_lanes = (v == 2 || v == 4) ? (int)v : 1;
    seen("MT_SPLIT");
  }
  if (env_int("MT_PREFETCH", &v)) {
    forced_prefetch = v != 0;
    seen("MT_PREFETCH");
  }
  h->reset_split = n <= P.reset_split_max;
  if (env_int("MT_RESET_SPLIT", &v)) {
    h->reset_split = v != 0;
    seen("MT_RESET_SPLIT");
  }
  h->graph_mode = -1;
  h->graph_max = P.graph_max;
  if (env_int("MT_GRAPH", &v)) {
    h->graph_mode = v != 0 ? 1 : 0;
    seen("MT_GRAPH");
  }
  h->flat_from = P.flat_from;
  if (env_int("MT_FLAT_FROM", &v)) {
    h->flat_from = std::max<long long>(0, v);
    seen("MT_FLAT_FROM");
  }
  h->blocks_per_cu_override = -1;
  if (env_int("MT_BLOCKS_PER_CU", &v)) {
    // 1 and 2 blocks per CU would need more than the default 64 KB of dynamic LDS per block: the smallest cap the pad can
    // realise is 3, and the kernel-name string reports what is really applied
    const int c = (int)std::max<long long>(0, std::min<long long>(8, v));
    h->blocks_per_cu_override = (c == 1 || c == 2) ? 3 : c;
    seen("MT_BLOCKS_PER_CU");
  }
  // End-pose sines / cosines from the whole-degree table (step kernels with TT; profiles/r03_variants.md section 3)
  h->trig_steps = h->static_kind != 0;
  if (env_int("MT_TRIG_TABLE", &v)) {
    h->trig_steps = v != 0 && h->static_kind != 0;
    seen("MT_TRIG_TABLE");
  }

  // ---- mt_rollout / mt_step as independent chains of launches on separate streams (engine_internal.h) ----
  h->chains = (n >= P.chains_min && n <= P.chains_max) ? 2 : 1;
  h->chains_forced = false;
  if (env_int("MT_CHAINS", &v)) {
    h->chains = (int)std::max<long long>(1, std::min<long long>(mt_engine::kMaxChains, v));
    h->chains_forced = true;
    seen("MT_CHAINS");
  }
  if (n < 2 * 256) h->chains = 1;
  h->lazy_chains = true;
  if (env_int("MT_LAZY_CHAINS", &v)) {  // 0: join at the end of every call
    h->lazy_chains = v != 0;
    seen("MT_LAZY_CHAINS");
  }

  // ---- mt_rollout: several steps per launch on small shards (the rollout kernels; default trigonometry only) ----
  h->multi_k = (n <= P.multi_step_max) ? P.multi_step_k : 1;
  if (env_int("MT_ROLLOUT_K", &v)) {
    h->multi_k = (int)std::max<long long>(1, std::min<long long>(64, v));
    seen("MT_ROLLOUT_K");
  }
  // ... which absorb the episode boundary: a deferred full reset as the first launch's prologue, the gather's snapshot as
  // the last launch's epilogue (kernels.h RolloutArgs)
  h->defer_reset = true;
  if (env_int("MT_DEFER_RESET", &v)) {
    h->defer_reset = v != 0;
    seen("MT_DEFER_RESET");
  }
  // ... and, for the chained launch-per-step form of the large batches, as a one-step launch of the rollout kernel in front
  // of each chain's step launches (profiles/r04_variants.md section 4)
  h->defer_reset_chained = P.fold_reset_into_chains;
  if (env_int("MT_DEFER_RESET_CHAINS", &v)) {
    h->defer_reset_chained = v != 0;
    seen("MT_DEFER_RESET_CHAINS");
  }
  h->gather_throttle = true;
  if (env_int("MT_GATHER_THROTTLE", &v)) {  // 0: mt_gather_returns_begin never waits on the host (a snapshot launch instead)
    h->gather_throttle = v != 0;
    seen("MT_GATHER_THROTTLE");
  }
  h->snap_in_rollout = true;
  if (env_int("MT_ROLLOUT_SNAP", &v)) {
    h->snap_in_rollout = v != 0;
    seen("MT_ROLLOUT_SNAP");
  }
  // ... whose launches take the prologue that runs the first step under the state loads (kernels.h RPF; static tables)
  h->rollout_early = true;
  if (env_int("MT_ROLLOUT_EARLY", &v)) {
    h->rollout_early = v != 0;
    seen("MT_ROLLOUT_EARLY");
  }

  // ---- mt_rollout_tape: the two optional choices of rollout_tape_kernel (kernels.h), off unless measured to pay ----
  h->tape_prefetch = false;
  if (env_int("MT_TAPE_PREFETCH", &v)) {
    h->tape_prefetch = v != 0;
    seen("MT_TAPE_PREFETCH");
  }
  h->tape_nt_loads = false;
  if (env_int("MT_TAPE_NT", &v)) {
    h->tape_nt_loads = v != 0;
    seen("MT_TAPE_NT");
  }

  // ---- the ground test's interior poses on dense lanes of the block (kernels.h, GroundQueue); 0: the per-lane loop ----
  h->ground_compact = true;
  if (env_int("MT_GROUND_COMPACT", &v)) {
    h->ground_compact = v != 0;
    seen("MT_GROUND_COMPACT");
  }

  // ---- sampled step launches re-derive the previous pose where the host knows what it is (kernels.h, PREV); 0: always load ----
  h->goals_rederive = h->static_kind == 1 ? P.rederive_goals_ref4 : (h->static_kind == 2 ? P.rederive_goals_dh7 : false);
  h->goals_rederive_chains = P.rederive_goals_chains;
  h->goals_rederive_max_envs = P.rederive_goals_max_envs;
  if (env_int("MT_GOALS_REDERIVE", &v)) {  // 1: both compile-time tables, every chain, launches of any size
    h->goals_rederive = v != 0 && h->static_kind != 0;
    h->goals_rederive_chains = mt_engine::kMaxChains;
    h->goals_rederive_max_envs = INT64_MAX;
    seen("MT_GOALS_REDERIVE");
  }

  if (h->custom_frames) h->lds_table = false;
  // The schedule of launches over `envs` envs, against the thresholds of their scope
  auto schedule_for = [&](int64_t envs, int64_t split4_max, int64_t split2_max, int64_t prefetch_other_max) {
    mt_engine::Schedule s;
    s.step_lanes = envs <= split4_max ? 4 : (envs <= split2_max ? 2 : 1);
    s.prefetch = h->static_kind == 1 || envs <= prefetch_other_max;
    s.rollout_lanes = envs <= P.fused_split4_max ? 4 : (envs <= P.fused_split2_max ? 2 : 1);
    if (forced_lanes) s.step_lanes = s.rollout_lanes = forced_lanes;
    if (forced_prefetch >= 0) s.prefetch = forced_prefetch != 0;
    if (h->custom_frames) s = mt_engine::Schedule{};  // RtTableF kernels: one env per lane, no prefetch
    return s;
  };
  h->sched[mt_engine::kBatch] = schedule_for(n, P.step_split4_max, P.step_split2_max, P.prefetch_other_max);
  // A chain of a multi-chain call is a batch of chain_span() envs: its launches use the schedule for THAT size
  h->sched[mt_engine::kChain] =
      h->chains > 1 ? schedule_for(chain_span(h, h->chains), P.chain_split4_max, P.chain_split2_max, P.chain_prefetch_other_max)
                    : h->sched[mt_engine::kBatch];
}

#define MT_DISPATCH_D(D_, FN, ...)   \
  switch (D_) {                      \
    case 2: FN<2>(__VA_ARGS__); break; \
    case 3: FN<3>(__VA_ARGS__); break; \
    case 4: FN<4>(__VA_ARGS__); break; \
    case 5: FN<5>(__VA_ARGS__); break; \
    case 6: FN<6>(__VA_ARGS__); break; \
    case 7: FN<7>(__VA_ARGS__); break; \
    case 8: FN<8>(__VA_ARGS__); break; \
    default: break;                  \
  }

// ---- what one step launch is: resolved once (plan_step), launched in one place (launch_plan), reported from the same value --
// The template arguments of step_kernel / step_split_kernel (kernels.h) by name; SAMPLE is apart (StepPlan::sample).
struct StepVariant {
  int trig = 0;        // TRIG
  bool lds = false;    // LDS: the DH table in LDS (runtime tables, recurrence only)
  int lanes = 1;       // 1: step_kernel; 2 / 4: step_split_kernel<.., L>
  int pf = 0;          // PF
  bool tt = false;     // TT
  bool flat = false;   // FLAT
  bool fresh = false;  // FRESH
  bool codes = false;  // CODES
  bool gc = false;     // GC: the interior poses of the ground test on dense lanes of the block (kernels.h, GroundQueue)
  int prev = kPrevLoad;  // PREV: the pose the step starts from is loaded / the zero pose / the action draw of the step before
};
constexpr unsigned variant_key(const StepVariant& v) {
  return (unsigned)v.trig | (unsigned)v.lds << 3 | (unsigned)v.lanes << 4 | (unsigned)(v.pf != 0) << 7 | (unsigned)v.tt << 8 |
         (unsigned)v.flat << 9 | (unsigned)v.fresh << 10 | (unsigned)v.codes << 11 | (unsigned)v.gc << 12 | (unsigned)v.prev << 13;
}

// Every instantiation the library holds, per table type.  A row without TT exists for sampled and for staged actions
// (SAMPLE = true / false), a row with TT for sampled actions only.  launch_plan instantiates these rows and nothing else.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wc++20-designator"
constexpr StepVariant kRuntimeVariants[] = {  // RtTable<D>
    {.trig = 0}, {.trig = 1}, {.trig = 2}, {.trig = 3}, {.trig = 4}, {.trig = 5},
    {.lds = true},
    {.lanes = 2}, {.lanes = 4},
    {.pf = kPrefetch}, {.pf = kPrefetch, .flat = true},
    {.gc = true}, {.pf = kPrefetch, .gc = true}, {.pf = kPrefetch, .flat = true, .gc = true},
};
constexpr StepVariant kFramesVariants[] = {{.trig = 0}, {.trig = 1}};  // RtTableF<D>
constexpr StepVariant kStaticVariants[] = {  // Ref4Table, Dh7Table
    {.trig = 0}, {.trig = 1}, {.trig = 2}, {.trig = 3}, {.trig = 4}, {.trig = 5},
    {.lanes = 2}, {.lanes = 4},
    {.lanes = 2, .tt = true}, {.lanes = 4, .tt = true},
    {.pf = kPrefetch}, {.pf = kPrefetch, .flat = true},
    {.pf = 0, .tt = true}, {.pf = kPrefetch, .tt = true}, {.pf = kPrefetch, .tt = true, .flat = true},
    {.pf = kPrefetch, .tt = true, .codes = true}, {.pf = kPrefetch, .tt = true, .flat = true, .codes = true},
    {.pf = 0, .tt = true, .fresh = true}, {.pf = kPrefetch, .tt = true, .fresh = true},
    {.pf = kPrefetch, .tt = true, .flat = true, .fresh = true},
    {.gc = true}, {.pf = kPrefetch, .gc = true}, {.pf = kPrefetch, .flat = true, .gc = true},
    {.pf = 0, .tt = true, .gc = true}, {.pf = kPrefetch, .tt = true, .gc = true}, {.pf = kPrefetch, .tt = true, .flat = true, .gc = true},
    {.pf = kPrefetch, .tt = true, .codes = true, .gc = true}, {.pf = kPrefetch, .tt = true, .flat = true, .codes = true, .gc = true},
    // the code-reading rows again, the previous pose re-derived (PREV)
    {.pf = kPrefetch, .tt = true, .codes = true, .prev = kPrevZero}, {.pf = kPrefetch, .tt = true, .flat = true, .codes = true, .prev = kPrevZero},
    {.pf = kPrefetch, .tt = true, .codes = true, .prev = kPrevDraw}, {.pf = kPrefetch, .tt = true, .flat = true, .codes = true, .prev = kPrevDraw},
    {.pf = kPrefetch, .tt = true, .codes = true, .gc = true, .prev = kPrevZero},
    {.pf = kPrefetch, .tt = true, .flat = true, .codes = true, .gc = true, .prev = kPrevZero},
    {.pf = kPrefetch, .tt = true, .codes = true, .gc = true, .prev = kPrevDraw},
    {.pf = kPrefetch, .tt = true, .flat = true, .codes = true, .gc = true, .prev = kPrevDraw},
};
#pragma clang diagnostic pop

enum class TableKind { kRuntime = 0, kRef4 = 1, kDh7 = 2, kFrames = 3 };  // RtTable<D>, Ref4Table, Dh7Table, RtTableF<D>
struct StepPlan {
  TableKind table = TableKind::kRuntime;
  int D = 0;
  bool sample = false;  // SAMPLE: actions drawn in the kernel (false: staged actions)
  StepVariant v;
  int blocks_per_cu = 0;  // resident-blocks cap (0 = none) ...
  size_t lds_bytes = 0;   // ... and the dynamic LDS that realises it (FRESH: at least the staging columns of the draw)
  dim3 grid;
  bool exists = true;  // false: no such kernel for this handle's schedule (FRESH only)
};

// The block-cooperative ground test (kernels.h, GroundQueue; MT_GROUND_COMPACT) of the one-env-per-lane recurrence kernels
// of a compile-time or runtime table.  Not on the single-env view (threads past the env would read outside its rows), not
// with MT_FLAG_DEBUG_ZMIN (MT_F_ZMIN wants every pose of every env: the per-lane loop), not for the long arms (D >= 6: the
// sequential schedule exists to fit 64 VGPRs, and both ends' state alive at the queue does not -- the runtime-table
// kernels spill, the prefetch kernels go from 62 to 74 VGPRs; profiles/ground_compaction_kernel_resources.md).
static bool ground_compacts(const mt_engine* h, bool whole_rows) {
  return h->ground_compact && whole_rows && h->trig == 0 && !h->lds_table && !h->custom_frames &&
         !(h->cfg.flags & MT_FLAG_DEBUG_ZMIN) && h->D <= 5;
}
template <int D>
static void ground_queue_bytes_d(size_t* out) { *out = sizeof(GroundQueue<RtTable<D>>); }
static size_t ground_queue_bytes(const mt_engine* h) {  // the static LDS the GC kernels of this handle's table add
  if (h->static_kind == 1) return sizeof(GroundQueue<Ref4Table>);
  if (h->static_kind == 2) return sizeof(GroundQueue<Dh7Table>);
  size_t bytes = 0;
  MT_DISPATCH_D(h->D, ground_queue_bytes_d, &bytes);
  return bytes;
}

// THE rules of which step kernel a launch of `n` envs gets -- every variant gives the same bits, so this is about time only:
//   scope  whose schedule: the whole batch, one chain's 256-aligned range of it, or the single-env view (batch schedule).
//          Batch and chain launches cover whole rows, so threads past the end of the range may read on to the end of their
//          block inside the rows (what the TT kernels do before their barrier); the single-env view does not
//   codes  the handle's target codes are valid (engine_internal.h, codes_valid)
//   prev   what the host knows the pose row of these envs to hold, as a PREV of kernels.h (launch_step: goals_prev); taken by
//          the kernels that have the form (the code-reading prefetch kernels), a load for every other
//   fresh  the first step of an episode with the deferred reset as the step kernel's own prologue (kernels.h, FRESH): the
//          sampled-action kernels of the static tables, one env per lane.  exists = false: the caller falls back to one
//          step of the rollout kernel
// Cheap enough to run per launch: no allocation, no strings.
StepPlan plan_step(const mt_engine* h, mt_engine::Scope scope, int64_t n, bool sample, bool codes, bool fresh = false,
                   int prev = kPrevLoad) {
  const mt_engine::Schedule& s = h->sched[scope == mt_engine::kChain ? mt_engine::kChain : mt_engine::kBatch];
  const bool whole_rows = scope != mt_engine::kOneEnv;
  StepPlan p;
  p.table = h->custom_frames ? TableKind::kFrames : (TableKind)h->static_kind;
  p.D = h->D;
  p.sample = sample;
  p.grid = grid_for(n);
  StepVariant& v = p.v;
  if (fresh) {
    const size_t stage = (size_t)2 * h->K * kBlock * sizeof(float), fixed = kTrigEntries * sizeof(SinCos) + 512;
    p.exists = h->trig == 0 && h->trig_steps && s.step_lanes == 1 && !h->lds_table && !h->trace &&
               stage + fixed <= 65536;  // (K > 20: above the default dynamic-LDS limit)
    if (!p.exists) return p;
    p.sample = true;
    v.tt = v.fresh = true;
    v.pf = s.prefetch ? kPrefetch : 0;
    v.flat = v.pf && n >= h->flat_from;
    p.blocks_per_cu = v.pf ? step_blocks_per_cu(h, n) : 0;
    p.lds_bytes = std::max(stage, lds_pad_for_blocks(p.blocks_per_cu, fixed));
    return p;
  }
  if (p.table == TableKind::kFrames) {  // runtime frames: the recurrence, or the polynomial sincos of long routes
    v.trig = h->trig == 1 ? 1 : 0;      // (mt_create: more than 12 rotations per half) and MT_FLAG_DIRECT_TRIG
    return p;
  }
  if (h->lds_table) {  // runtime tables only; the LDS-table kernel is the recurrence whatever the handle's trig says
    v.lds = true;
    return p;
  }
  if (h->trig != 0) {  // no schedules beside the recurrence
    v.trig = h->trig;
    return p;
  }
  // sampled actions of a compile-time table on whole rows: both end poses' sines / cosines from the table (TT)
  v.tt = sample && h->trig_steps && whole_rows;
  if (s.step_lanes > 1) {  // tiny batches: one env over 2 or 4 lanes (kernels.h, step_split_kernel)
    v.lanes = s.step_lanes;
    const int64_t per_block = kBlock / v.lanes;
    p.grid = dim3((unsigned)((n + per_block - 1) / per_block));
    return p;
  }
  v.pf = s.prefetch ? kPrefetch : 0;    // target loads in flight before the kinematics (kernels.h, PF)
  v.flat = v.pf && n >= h->flat_from;   // HBM-bound launches: kernels.h, LaneOffset<false>
  // the prefetch kernels read the targets as their codes while those are valid (kernels.h, CODES: 28 B per env less)
  v.codes = v.pf && v.tt && codes;
  v.prev = v.codes ? prev : kPrevLoad;
  v.gc = ground_compacts(h, whole_rows);
  if (v.pf && v.tt) {  // see step_blocks_per_cu
    p.blocks_per_cu = step_blocks_per_cu(h, n);
    p.lds_bytes = lds_pad_for_blocks(p.blocks_per_cu, kTrigEntries * sizeof(SinCos) + (v.gc ? ground_queue_bytes(h) : 0));
  }
  return p;
}

// The only place that spells the kernels' template argument lists: row I of ROWS, every argument by its name.
template <class Tbl, bool SAMPLE, const auto& ROWS, size_t I>
void launch_variant(const StepPlan& p, hipStream_t stream, const StepArgs& args) {
  constexpr StepVariant V = ROWS[I];
  if constexpr (V.lanes > 1)
    hipLaunchKernelGGL((step_split_kernel<Tbl, SAMPLE, V.lanes, V.tt>), p.grid, dim3(kBlock), p.lds_bytes, stream, args);
  else
    hipLaunchKernelGGL((step_kernel<Tbl, SAMPLE, V.trig, V.lds, V.pf, V.tt, V.flat, V.fresh, V.codes, V.gc, V.prev>), p.grid,
                       dim3(kBlock), p.lds_bytes, stream, args);
}
// ... if row I is the plan's variant (false: it is not)
template <class Tbl, const auto& ROWS, size_t I>
bool launch_row(const StepPlan& p, hipStream_t stream, const StepArgs& args) {
  if (variant_key(p.v) != variant_key(ROWS[I])) return false;
  if constexpr (ROWS[I].gc && Tbl::D >= 6)
    return false;  // never planned (ground_compacts), not instantiated
  else if (p.sample)
    launch_variant<Tbl, true, ROWS, I>(p, stream, args);
  else if constexpr (!ROWS[I].tt)
    launch_variant<Tbl, false, ROWS, I>(p, stream, args);
  else
    return false;  // TT serves sampled actions only
  return true;
}
template <class Tbl, const auto& ROWS, size_t... I>
bool launch_rows(const StepPlan& p, hipStream_t stream, const StepArgs& args, std::index_sequence<I...>) {
  return (launch_row<Tbl, ROWS, I>(p, stream, args) || ...);
}
template <class Tbl, const auto& ROWS>
bool launch_table(const StepPlan& p, hipStream_t stream, const StepArgs& args) {
  return launch_rows<Tbl, ROWS>(p, stream, args, std::make_index_sequence<std::size(ROWS)>{});
}
template <int D>
void launch_plan_d(const StepPlan& p, hipStream_t stream, const StepArgs& args, bool* launched) {
  *launched = p.table == TableKind::kFrames ? launch_table<RtTableF<D>, kFramesVariants>(p, stream, args)
                                            : launch_table<RtTable<D>, kRuntimeVariants>(p, stream, args);
}

// Launches the kernel a plan names.  A plan outside the tables above is a bug in plan_step, not a condition to run past.
void launch_plan(const StepPlan& p, hipStream_t stream, const StepArgs& args) {
  bool launched = false;
  // GC kernels keep the threads past the end of the batch up to the barriers, and those load at their own offsets: the rows
  // must cover the grid (whole-row launches do: ld >= the batch rounded up to blocks; ground_compacts keeps the rest out)
  if (p.v.gc && (int64_t)p.grid.x * kBlock > args.ld) {
    std::fprintf(stderr, "manytor: a ground-compacting step launch of %u blocks over rows of %lld\n", p.grid.x, (long long)args.ld);
    std::abort();
  }
  if (p.table == TableKind::kRef4)
    launched = launch_table<Ref4Table, kStaticVariants>(p, stream, args);
  else if (p.table == TableKind::kDh7)
    launched = launch_table<Dh7Table, kStaticVariants>(p, stream, args);
  else
    MT_DISPATCH_D(p.D, launch_plan_d, p, stream, args, &launched);
  if (!launched) {
    std::fprintf(stderr, "manytor: no step kernel for table %d, D %d, sample %d, variant key 0x%x\n", (int)p.table, p.D,
                 (int)p.sample, variant_key(p.v));
    std::abort();
  }
}

template <int D>
void launch_trace_d(mt_handle h, const StepArgs& args, float* trace, bool sample) {
  if (sample)
    hipLaunchKernelGGL((trace_kernel<D, true>), grid_for(args.n), dim3(kBlock), 0, h->stream, args, trace);
  else
    hipLaunchKernelGGL((trace_kernel<D, false>), grid_for(args.n), dim3(kBlock), 0, h->stream, args, trace);
}

// May the host keep a record of what a step launch leaves in MT_F_GOALS, and trust the one it has?  Not once the row's address
// is out (goals_exposed) or a caller was seen capturing the handle's calls (goals_foreign), not for a launch that is being captured
// (major_base: the handle's own graphs; replays run whatever the row holds).
static bool goals_tracked(const mt_engine* h, const StepArgs& args) {
  return !h->goals_exposed && !h->goals_foreign && !args.major_base;
}

// What a step launch takes the pose it starts from to be: a PREV of kernels.h out of the host's record of the row
// (engine_internal.h: GoalsRow), or -1 -- a load by a launch that leaves no record either.  The draw of step - 1 is named only
// where the record says exactly that: the same seed, the step index right before this launch's.
static int goals_prev(const mt_engine* h, mt_engine::Scope scope, const StepArgs& args, bool traced, bool sample, int chain) {
  if (!sample || traced || scope == mt_engine::kOneEnv || !goals_tracked(h, args)) return -1;
  mt_engine::GoalsRow r = h->goals_row[chain >= 0 ? chain : 0];
  if (chain < 0)  // the whole batch: every chain's range has to be in the same state
    for (int c = 1; c < h->chains; ++c)
      if (h->goals_row[c].kind != r.kind || h->goals_row[c].seed != r.seed || h->goals_row[c].step != r.step) r = mt_engine::GoalsRow{};
  // (kPolicy.rederive_goals_chains, rederive_goals_max_envs)
  if (!h->goals_rederive || chain >= h->goals_rederive_chains || args.n > h->goals_rederive_max_envs) return kPrevLoad;
  if (r.kind == mt_engine::GoalsRow::kZero) return kPrevZero;
  const uint64_t seed = ((uint64_t)args.seed_hi << 32) | args.seed_lo;
  if (r.kind == mt_engine::GoalsRow::kDraw && r.seed == seed && r.step + 1u == args.major && args.major != 0u) return kPrevDraw;
  return kPrevLoad;
}

// One env step of the envs `args` describes (the whole batch, a chain's range, or one env of it: args_for_env), on the
// schedule of `scope`; `trace` is the matching view of the sub-step trace buffer or NULL.
// `chain`: the chain whose range `args` is (scope kChain), -1 for the whole batch or one env of it.
void launch_step(mt_handle h, mt_engine::Scope scope, const StepArgs& args, float* trace, bool sample, int chain = -1) {
  if (trace) MT_DISPATCH_D(h->D, launch_trace_d, h, args, trace, sample);  // first: it needs the previous pose
  const int prev = goals_prev(h, scope, args, trace != nullptr, sample, chain);
  const StepPlan p = plan_step(h, scope, args.n, sample, h->codes_valid, false, prev < 0 ? (int)kPrevLoad : prev);
  launch_plan(p, h->stream, args);
  h->codes_valid = p.v.codes;  // every step kernel may zero targets; only the ones that read codes zero those too
  if (p.v.prev != kPrevLoad) ++h->goals_rederived;
  // a sampled step of the whole range leaves its action draw as the pose (prev >= 0: a launch that runs now, with a step index
  // the host knows); a staged action, one env of the batch, a captured launch or a traced one leave the row unknown
  const mt_engine::GoalsRow row =
      (prev >= 0 && sample && p.v.lanes == 1)
          ? mt_engine::GoalsRow{mt_engine::GoalsRow::kDraw, args.major, ((uint64_t)args.seed_hi << 32) | args.seed_lo}
          : mt_engine::GoalsRow{};
  if (chain >= 0)
    h->goals_row[chain] = row;
  else
    for (mt_engine::GoalsRow& g : h->goals_row) g = row;
}

void launch_step(mt_handle h, bool sample) { launch_step(h, mt_engine::kBatch, h->args, h->trace, sample); }

// The first step of an episode with the deferred reset inside it (plan_step, fresh); false = no such kernel for this
// handle's schedule.  `args` carries reset_seed / reset_episode / radius.
bool launch_step_fresh(mt_handle h, mt_engine::Scope scope, const StepArgs& args, int chain) {
  const StepPlan p = plan_step(h, scope, args.n, true, false, true);
  if (!p.exists) return false;
  launch_plan(p, h->stream, args);
  h->codes_valid = p.v.codes;  // (false: the drawn targets are written as floats only)
  const mt_engine::GoalsRow row = goals_tracked(h, args)  // the pose it leaves is its action draw, as after any sampled step
                                      ? mt_engine::GoalsRow{mt_engine::GoalsRow::kDraw, args.major, ((uint64_t)args.seed_hi << 32) | args.seed_lo}
                                      : mt_engine::GoalsRow{};
  if (chain >= 0)
    h->goals_row[chain] = row;
  else
    for (mt_engine::GoalsRow& g : h->goals_row) g = row;
  return true;
}

// ---- multi-chain rollouts ------------------------------------------------------------------------------------------
StepArgs args_for_range(mt_handle h, const StepArgs& base, int64_t off, int64_t cnt);
int check_launch(mt_handle h, const char* what);
int ensure_chains(mt_handle h, int chains) {
  if (!h->ev_fork) MT_HIP(h, hipEventCreateWithFlags(&h->ev_fork, event_flags(false)));
  for (int c = 1; c < chains; ++c) {
    if (!h->chain_streams[c]) MT_HIP(h, hipStreamCreateWithFlags(&h->chain_streams[c], hipStreamNonBlocking));
    if (!h->ev_join[c]) MT_HIP(h, hipEventCreateWithFlags(&h->ev_join[c], event_flags(false)));
  }
  return MT_OK;
}

// One chain's T steps on the handle's CURRENT stream (h->stream): chain c owns envs [c * span, (c + 1) * span).  The
// step-kernel schedule is the one for the chain's env count (a chain is a batch of `span` envs).  `a0` carries seed /
// major_base; step s is launched with major = major0 + s.  sample = false: staged actions (mt_step), T = 1.
void launch_chain(mt_handle h, const StepArgs& a0, uint32_t major0, int T, int chains, int c, bool sample = true) {
  const int64_t span = chain_span(h, chains), off = (int64_t)c * span;
  if (off >= h->n) return;
  StepArgs as = args_for_range(h, a0, off, std::min(span, h->n - off));
  for (int s = 0; s < T; ++s) {
    as.major = major0 + (uint32_t)s;
    launch_step(h, mt_engine::kChain, as, nullptr, sample, c);
  }
}

// Chain c's FIRST step of an episode, the deferred reset inside it (launch_step_fresh); false: not served.
bool launch_chain_fresh(mt_handle h, const StepArgs& a0, uint32_t major, int chains, int c) {
  const int64_t span = chain_span(h, chains), off = (int64_t)c * span;
  if (off >= h->n) return true;
  StepArgs as = args_for_range(h, a0, off, std::min(span, h->n - off));
  as.major = major;
  return launch_step_fresh(h, mt_engine::kChain, as, c);
}

// Chain c's stream (chain 0 runs on the handle's own stream).
hipStream_t chain_stream(mt_handle h, int c) { return c == 0 ? h->stream : h->chain_streams[c]; }

// Start the chains off the handle's stream: everything queued on it so far is ahead of what the chains will run.
int fork_chains(mt_handle h, int chains) {
  if (h->forked) return MT_OK;
  int rc = ensure_chains(h, chains);
  if (rc) return rc;
  const int64_t span = chain_span(h, chains);
  MT_HIP(h, hipEventRecord(h->ev_fork, h->stream));
  for (int c = 1; c < chains; ++c)
    if ((int64_t)c * span < h->n) MT_HIP(h, hipStreamWaitEvent(h->chain_streams[c], h->ev_fork, 0));
  h->forked = true;
  return MT_OK;
}

// After a per-chain call: on the handle's private stream the chains may stay forked (the next per-chain call continues
// them, any other call joins: MT_ENTER); on a caller's stream the call has to be complete in stream order when it returns.
int settle_chains(mt_handle h) { return (h->lazy_chains && h->stream == h->own_stream) ? MT_OK : join_chains(h); }

// Every row base of `a` moved `off` envs to the right (done_bits, snap and n are the caller's: they differ per view).
void shift_rows(StepArgs& a, int64_t off) {
  a.actions += off;
  a.goals += off;
  a.points += off;
  a.codes += off;
  a.alive += off;
  a.total_reward += off;
  a.obs += off;
  a.reward += off;
  a.done += off;
  a.ee += off;
  a.episodes += off;
  a.last_return += off;
  if (a.ring) a.ring += off;
  if (a.zmin) a.zmin += off;
  a.env_base += off;
}

// The view of ONE env of the batch, n = 1.  The wavefront ballot of such a launch goes to a spare word; the real
// done_bits word is rebuilt afterwards (done_bits_word_kernel).
StepArgs args_for_env(mt_handle h, int64_t env) {
  StepArgs a = h->args;
  shift_rows(a, env);
  a.done_bits = h->spare_bits;
  a.snap = nullptr;
  a.n = 1;
  return a;
}

// The view of a contiguous RANGE of envs [off, off + cnt) of the batch, off a multiple of 256 (whole blocks, whole ballot
// words, 1 KiB-aligned row segments): what one chain of a multi-chain mt_rollout launches on.
StepArgs args_for_range(mt_handle h, const StepArgs& base, int64_t off, int64_t cnt) {
  StepArgs a = base;
  shift_rows(a, off);
  a.done_bits += off / 64;
  if (a.snap) a.snap += off;
  a.n = cnt;
  return a;
}

template <int D, bool RANDOM, bool ONLY_DONE>
void launch_reset_k(mt_handle h, const StepArgs& args) {
  const size_t lds = RANDOM ? (size_t)2 * args.K * kBlock * sizeof(float) : 0;  // staging columns of the drawn target codes
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&reset_kernel<D, RANDOM, ONLY_DONE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((reset_kernel<D, RANDOM, ONLY_DONE>), grid_for(args.n), dim3(kBlock), lds, h->stream, args,
                     h->cfg.radius);
}
template <int D, bool ONLY_DONE>
void launch_reset_split(mt_handle h, const StepArgs& args) {  // whole batch, small: 4 lanes per env for the draw
  constexpr int L = 4;
  const int64_t per_block = kBlock / L;
  const size_t lds = (size_t)2 * args.K * per_block * sizeof(float);
  hipLaunchKernelGGL((reset_split_kernel<D, ONLY_DONE, L>), dim3((unsigned)((args.n + per_block - 1) / per_block)),
                     dim3(kBlock), lds, h->stream, args, h->cfg.radius);
}
template <int D>
void launch_reset_d(mt_handle h, const StepArgs& args, int mode) {  // 0 given points, 1 random, 2 random only-done
  // (the random forms write codes with the targets they draw; a full reset of the whole batch makes them valid: its caller)
  if (mode == 0) h->codes_valid = false;
  if (mode != 0 && h->reset_split && args.n == h->n)
    return mode == 1 ? launch_reset_split<D, false>(h, args) : launch_reset_split<D, true>(h, args);
  if (mode == 0)
    launch_reset_k<D, false, false>(h, args);
  else if (mode == 1)
    launch_reset_k<D, true, false>(h, args);
  else
    launch_reset_k<D, true, true>(h, args);
}

template <int D>
void launch_observe_d(mt_handle h) {
  hipLaunchKernelGGL((observe_kernel<D>), grid_for(h->n), dim3(kBlock), 0, h->stream, h->args);
}
template <int D>
void launch_check_done_d(mt_handle h) {
  hipLaunchKernelGGL((check_done_kernel<D>), grid_for(h->n), dim3(kBlock), 0, h->stream, h->args);
}
template <int D>
void launch_joints_d(mt_handle h, float* out) {
  hipLaunchKernelGGL((joints_kernel<D>), grid_for(h->n), dim3(kBlock), 0, h->stream, h->args, out);
}

// ik_kernel / jacobian_kernel with the handle's table: the compile-time table it matched, else the runtime table with the
// runtime pickup frame.
template <class Tbl>
void launch_ik_t(mt_handle h, const IkArgs& r) {
  hipLaunchKernelGGL((ik_kernel<Tbl>), grid_for(r.n), dim3(kBlock), 0, h->stream, r);
}
template <int D>
void launch_ik_d(mt_handle h, const IkArgs& r) {
  launch_ik_t<RtTableF<D>>(h, r);
}
void launch_ik(mt_handle h, const IkArgs& r) {
  if (h->static_kind == 1) return launch_ik_t<Ref4Table>(h, r);
  if (h->static_kind == 2) return launch_ik_t<Dh7Table>(h, r);
  MT_DISPATCH_D(h->D, launch_ik_d, h, r);
}
template <class Tbl>
void launch_jacobian_t(mt_handle h, const JacobianArgs& r) {
  hipLaunchKernelGGL((jacobian_kernel<Tbl>), grid_for(r.n), dim3(kBlock), 0, h->stream, r);
}
template <int D>
void launch_jacobian_d(mt_handle h, const JacobianArgs& r) {
  launch_jacobian_t<RtTableF<D>>(h, r);
}
void launch_jacobian(mt_handle h, const JacobianArgs& r) {
  if (h->static_kind == 1) return launch_jacobian_t<Ref4Table>(h, r);
  if (h->static_kind == 2) return launch_jacobian_t<Dh7Table>(h, r);
  MT_DISPATCH_D(h->D, launch_jacobian_d, h, r);
}

// The rollout kernels on the envs `a` describes (the whole batch or a chain's 256-aligned range), `split` lanes per env.
// RPF (kernels.h): the prologue that requests everything up front and runs the first step under the loads -- for the short
// launches of mt_rollout's multi-step form, compile-time tables only (the long fused launches keep RPF = 0).
template <class Tbl, int L, int RPF>
void launch_rollout_split_t(mt_handle h, const StepArgs& a, const RolloutArgs& r) {
  const int64_t per_block = kBlock / L;
  const size_t lds = (size_t)3 * h->K * per_block * sizeof(float) + (ActionTrigTable<Tbl>::value ? kTrigEntries * sizeof(SinCos) : 0);
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_split_kernel<Tbl, L, RPF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_split_kernel<Tbl, L, RPF>), dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(kBlock), lds,
                     h->stream, a, r);
}

template <class Tbl, int RPF>
void launch_rollout_t(mt_handle h, const StepArgs& a, int lanes, const RolloutArgs& r) {
  if (lanes == 4) return launch_rollout_split_t<Tbl, 4, RPF>(h, a, r);
  if (lanes == 2) return launch_rollout_split_t<Tbl, 2, RPF>(h, a, r);
  // 21.5 KB at K = 7, 96 KB at K = 32 (of 160 KB), + 3.6 KB for the action sin / cos table of the compile-time tables
  const size_t lds = (size_t)3 * h->K * kBlock * sizeof(float) + (ActionTrigTable<Tbl>::value ? kTrigEntries * sizeof(SinCos) : 0);
  if (lds > 65536)  // above the default dynamic-LDS limit the kernel has to be told
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel<Tbl, RPF>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_kernel<Tbl, RPF>), grid_for(a.n), dim3(kBlock), lds, h->stream, a, r);
}

template <int D>
void launch_rollout_d(mt_handle h, const StepArgs& a, int lanes, const RolloutArgs& r) {
  launch_rollout_t<RtTable<D>, 0>(h, a, lanes, r);
}
// `lanes` per env: the rollout_lanes of the launch's scope (engine_internal.h, Schedule), or 1
void launch_rollout(mt_handle h, const StepArgs& a, int lanes, const RolloutArgs& r, bool early = false) {
  h->codes_valid = false;  // the rollout kernels write targets as floats only
  h->forget_goals();       // ... and leave the pose of their last step
  if (h->static_kind == 1) return early ? launch_rollout_t<Ref4Table, kPrefetch>(h, a, lanes, r) : launch_rollout_t<Ref4Table, 0>(h, a, lanes, r);
  if (h->static_kind == 2) return early ? launch_rollout_t<Dh7Table, kPrefetch>(h, a, lanes, r) : launch_rollout_t<Dh7Table, 0>(h, a, lanes, r);
  MT_DISPATCH_D(h->D, launch_rollout_d, h, a, lanes, r);
}

// rollout_tape_kernel on the whole batch: one env per lane for every table kind and batch size.
template <class Tbl, bool PREFETCH>
void launch_tape_t(mt_handle h, const StepArgs& a, const TapeArgs& r) {
  const size_t lds = (size_t)3 * h->K * kBlock * sizeof(float);  // 21.5 KB at K = 7, 96 KB at K = 32
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_tape_kernel<Tbl, PREFETCH>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_tape_kernel<Tbl, PREFETCH>), grid_for(a.n), dim3(kBlock), lds, h->stream, a, r);
}
template <int D>
void launch_tape_d(mt_handle h, const StepArgs& a, const TapeArgs& r) {
  launch_tape_t<RtTable<D>, false>(h, a, r);
}
// (the next-step prefetch exists for the compile-time tables, where it was measured: tools/tape_rollout_sweep.py)
bool tape_prefetches(const mt_engine* h) { return h->tape_prefetch && h->static_kind != 0; }
void launch_tape(mt_handle h, const StepArgs& a, const TapeArgs& r) {
  const bool pf = tape_prefetches(h);
  if (h->static_kind == 1) return pf ? launch_tape_t<Ref4Table, true>(h, a, r) : launch_tape_t<Ref4Table, false>(h, a, r);
  if (h->static_kind == 2) return pf ? launch_tape_t<Dh7Table, true>(h, a, r) : launch_tape_t<Dh7Table, false>(h, a, r);
  MT_DISPATCH_D(h->D, launch_tape_d, h, a, r);
}

// f(TableTag<Tbl>{}) with the handle's table type: the kernels of the planner calls have no other compile-time axis.
// mt_shoot's commit: rollout_tape_kernel with every env following the plane its evaluation chose (SELECT).  One form, no
// next-step prefetch (it was measured for the plain tape only).
template <class Tbl>
void launch_tape_select_t(mt_handle h, const StepArgs& a, const TapeArgs& r) {
  const size_t lds = (size_t)3 * h->K * kBlock * sizeof(float);
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_tape_kernel<Tbl, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_tape_kernel<Tbl, false, true>), grid_for(a.n), dim3(kBlock), lds, h->stream, a, r);
}
void launch_tape_select(mt_handle h, const StepArgs& a, const TapeArgs& r) {
  with_table(h, [&](auto tag) { launch_tape_select_t<typename decltype(tag)::type>(h, a, r); });
}

// rollout_policy_kernel on the whole batch: the tape kernel's shape; W = the smallest compiled extent of the hidden
// register arrays that holds the policy's widest hidden layer.
template <class Tbl, int W>
void launch_policy_t(mt_handle h, const StepArgs& a, const PolicyArgs& r) {
  const size_t lds = (size_t)3 * h->K * kBlock * sizeof(float);  // 21.5 KB at K = 7, 96 KB at K = 32
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_policy_kernel<Tbl, W>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_policy_kernel<Tbl, W>), grid_for(a.n), dim3(kBlock), lds, h->stream, a, r);
}
void launch_policy(mt_handle h, const StepArgs& a, const PolicyArgs& r, int width) {
  with_table(h, [&](auto tag) {
    using Tbl = typename decltype(tag)::type;
    if (width <= 32) return launch_policy_t<Tbl, 32>(h, a, r);
    launch_policy_t<Tbl, 64>(h, a, r);
  });
}

// shoot_kernel on the whole batch: a block per 64 envs, its four waves share the candidates (kernels.h).
template <class Tbl>
void launch_shoot_t(mt_handle h, const StepArgs& a, const ShootArgs& r) {
  // targets [3K][64] + the four waves' (best return, index) pairs: 7.3 KB at K = 7, 26 KB at K = 32
  const size_t lds = ((size_t)3 * h->K + 2 * kShootWaves) * kShootEnvs * sizeof(float);
  hipLaunchKernelGGL((shoot_kernel<Tbl>), dim3((unsigned)((a.n + kShootEnvs - 1) / kShootEnvs)), dim3(kBlock), lds, h->stream, a, r);
}
void launch_shoot(mt_handle h, const StepArgs& a, const ShootArgs& r) {
  with_table(h, [&](auto tag) { launch_shoot_t<typename decltype(tag)::type>(h, a, r); });
}

// cem_kernel on the whole batch: shoot_kernel's shape plus the [C][64] score tile, the four waves' elite masks and the
// best index (at most 43 KB: K = 32, C = 64).
template <class Tbl>
void launch_cem_t(mt_handle h, const StepArgs& a, const CemArgs& r) {
  const size_t lds = ((size_t)3 * h->K + (size_t)r.C + 2 * kShootWaves + 1) * kShootEnvs * sizeof(float);
  hipLaunchKernelGGL((cem_kernel<Tbl>), dim3((unsigned)((a.n + kShootEnvs - 1) / kShootEnvs)), dim3(kBlock), lds, h->stream, a, r);
}
void launch_cem(mt_handle h, const StepArgs& a, const CemArgs& r) {
  with_table(h, [&](auto tag) { launch_cem_t<typename decltype(tag)::type>(h, a, r); });
}

// mppi_kernel on the whole batch: cem_kernel's shape; LDS holds the target tile, the [C][64] score / weight tile and the
// table of 2T + 1 <= 255 powers of decay (at most 41 KB: K = 32, C = 64).
template <class Tbl>
void launch_mppi_t(mt_handle h, const StepArgs& a, const MppiArgs& r) {
  const size_t lds = (((size_t)3 * h->K + (size_t)r.C) * kShootEnvs + kMppiTable) * sizeof(float);
  hipLaunchKernelGGL((mppi_kernel<Tbl>), dim3((unsigned)((a.n + kShootEnvs - 1) / kShootEnvs)), dim3(kBlock), lds, h->stream, a, r);
}
void launch_mppi(mt_handle h, const StepArgs& a, const MppiArgs& r) {
  with_table(h, [&](auto tag) { launch_mppi_t<typename decltype(tag)::type>(h, a, r); });
}

// sample_plans_kernel: a thread per (env, step, candidate); it needs the number of joints only
template <int D>
void launch_sample_plans_d(mt_handle h, const CemArgs& r, float* plans, int64_t ld, int64_t cand_stride) {
  hipLaunchKernelGGL((sample_plans_kernel<D>), dim3(grid_for(h->n).x, (unsigned)r.T, (unsigned)r.C), dim3(kBlock), 0, h->stream, r, plans,
                     ld, cand_stride, h->args.n, h->args.env_base);
}

// The rollout kernels implement the default trigonometry and the reference's frame rows only.
bool fusable(mt_handle h) { return h->trig == 0 && !h->lds_table && !h->trace && !h->custom_frames; }
// Which of these a handle that is not fusable has: the first that applies.
const char* unfusable_reason(const mt_engine* h) {
  return h->custom_frames                        ? "custom obs_frame / ee_frame"
         : h->trace                              ? "MT_FLAG_TRACE"
         : h->lds_table                          ? "MT_FLAG_DH_IN_LDS"
         : h->trig == 2                          ? "MT_FLAG_HW_TRIG"
         : (h->cfg.flags & MT_FLAG_DIRECT_TRIG) ? "MT_FLAG_DIRECT_TRIG"
         : h->trig == 1                          ? "substeps beyond the recurrence's reach (per-pose trigonometry)"
                                                 : "a profiling flag (MT_FLAG_ABLATE_*)";
}
// The refusal of the calls that exist on the rollout kernels only (mt_rollout_tape and the planners on top of it).
int fail_unfusable(mt_handle h, const char* who) {
  return fail(h, MT_ERR_UNSUPPORTED, std::string(who) + ": not available on a handle with " + unfusable_reason(h));
}

// Does mt_rollout(n_steps >= 2) on this handle run k steps per launch through the rollout kernels right now?
bool rollout_is_multi_step(mt_handle h) { return h->multi_k > 1 && fusable(h); }
// Does it run as chains of one launch per step whose FIRST launch can be the rollout kernel with the reset as its prologue?
bool chained_rollout_absorbs_reset(mt_handle h) {
  const bool graph = h->graph_mode > 0 || (h->graph_mode < 0 && h->n <= h->graph_max);
  return h->defer_reset_chained && !rollout_is_multi_step(h) && h->chains > 1 && h->lazy_chains && !h->trace && !graph && fusable(h);
}


int check_launch(mt_handle h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, MT_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return MT_OK;
}

struct FieldInfo {
  void* ptr;
  int rows;      // SoA rows
  int dtype;     // element dtype of the resident buffer
  size_t esize;  // element size
};

int field_info(mt_handle h, int field, FieldInfo* fi) {
  const StepArgs& a = h->args;
  switch (field) {
    case MT_F_ACTIONS: *fi = {a.actions, h->D, MT_F32, 4}; return MT_OK;
    case MT_F_GOALS: *fi = {a.goals, h->D, MT_F32, 4}; return MT_OK;
    case MT_F_POINTS: *fi = {a.points, 3 * h->K, MT_F32, 4}; return MT_OK;
    case MT_F_ALIVE: *fi = {a.alive, 1, MT_U32, 4}; return MT_OK;
    case MT_F_OBS: *fi = {a.obs, 3 * h->K, MT_F32, 4}; return MT_OK;
    case MT_F_REWARD: *fi = {a.reward, 1, MT_I32, 4}; return MT_OK;
    case MT_F_DONE: *fi = {a.done, 1, MT_U8, 1}; return MT_OK;
    case MT_F_DONE_BITS: *fi = {a.done_bits, 1, MT_U64, 8}; return MT_OK;
    case MT_F_EE: *fi = {a.ee, 3, MT_F32, 4}; return MT_OK;
    case MT_F_TOTAL_REWARD: *fi = {a.total_reward, 1, MT_F32, 4}; return MT_OK;
    case MT_F_EPISODES: *fi = {a.episodes, 1, MT_U32, 4}; return MT_OK;
    case MT_F_LAST_RETURN: *fi = {a.last_return, 1, MT_F32, 4}; return MT_OK;
    case MT_F_RETURN_RING:
      if (!a.ring) return fail(h, MT_ERR_STATE, "MT_F_RETURN_RING: the handle was created with return_ring = 0");
      *fi = {a.ring, (int)a.ring_slots, MT_F32, 4};
      return MT_OK;
    case MT_F_TRACE:
      if (!h->trace) return fail(h, MT_ERR_STATE, "MT_F_TRACE: the handle was created without MT_FLAG_TRACE");
      *fi = {h->trace, 3 * h->cfg.substeps, MT_F32, 4};
      return MT_OK;
    case MT_F_ZMIN:
      if (!a.zmin) return fail(h, MT_ERR_STATE, "MT_F_ZMIN: the handle was created without MT_FLAG_DEBUG_ZMIN");
      *fi = {a.zmin, 1, MT_F32, 4};
      return MT_OK;
    default: return fail(h, MT_ERR_INVALID_ARG, "unknown or non-resident field");
  }
}

}  // namespace

// =================================================================================================
// Host arrays handed to mt_set / mt_reset are screened on the bit pattern before they reach the arena (the kernels are
// built with -ffinite-math-only): `limit` = largest accepted magnitude as a float bit pattern.
static int64_t first_unusable(const float* v, int64_t count, uint32_t limit) {
  for (int64_t i = 0; i < count; ++i) {
    uint32_t bits;
    std::memcpy(&bits, v + i, 4);
    if ((bits & 0x7FFFFFFFu) > limit) return i;
  }
  return -1;
}
// Resets write MT_F_LAST_RETURN: an exchange that is still reading that row in place has to finish first.
static int order_behind_inplace_gather(mt_handle h, hipStream_t stream) {
  if (h->gather_pending && h->gather_inplace) MT_HIP(h, hipStreamWaitEvent(stream, h->ev_g1, 0));
  return MT_OK;
}

// Chains a whole-batch call may run as, right now: the handle's chain count unless the sub-step trace is on or the caller
// is capturing the handle's stream into a graph of their own (they get the plain single-stream sequence).
// per_step_call: mt_step / mt_sample_actions / mt_set_actions -- ONE launch per range and call.  On a caller's stream every
// call has to fork behind the caller's work and join back before it returns, two cross-stream dependencies for one launch:
// measured with a torch policy on the same stream (examples/policy_loop.py, 1 M arms) 144.4 us per loop iteration in two
// chains against 127.3 in one (profiles/r04_policy_loop_chains_on_torch_stream.txt), so there the step stays one launch.
// On the handle's own stream the chains stay forked from call to call and the step is 42 -> 37.5 us at 1 M arms.
static int usable_chains(mt_handle h, bool per_step_call = false) {
  if (h->chains <= 1 || h->trace) return 1;
  if (per_step_call && !(h->lazy_chains && h->stream == h->own_stream)) return 1;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return 1;
  }
  return h->chains;
}

// fn(c, off, cnt) once per chain with h->stream switched to the chain's stream; forks first, settles afterwards.
template <class F>
static int per_chain(mt_handle h, int chains, const char* what, F&& fn) {
  int rc = fork_chains(h, chains);
  if (rc) return rc;
  const int64_t span = chain_span(h, chains);
  hipStream_t root = h->stream;
  for (int c = 0; c < chains; ++c) {
    const int64_t off = (int64_t)c * span;
    if (off >= h->n) continue;
    h->stream = c == 0 ? root : h->chain_streams[c];
    fn(c, off, std::min(span, h->n - off));
  }
  h->stream = root;
  rc = check_launch(h, what);
  if (rc) return rc;
  return settle_chains(h);
}

constexpr uint32_t kMaxAngleBits = 0x47000000u;   // 32768.0f: the bound of unusable_angle (kernels.h)
constexpr uint32_t kMaxFiniteBits = 0x7F7FFFFFu;  // FLT_MAX

// ---- what mt_rollout_tape, mt_shoot, mt_cem and mt_mppi (and mt_sample_plans) share on the host ------------------------
// The commit they all end in: rollout_tape_kernel on the whole batch and the bookkeeping of a call that moves the state.
// The caller has set in `r` what is its own: the tape and the logs (tape_args), dry_run, nt_loads and, with `select`
// (mt_shoot: env i follows the plane r.best[i] of a stack of tapes), best / cand_stride.
static int commit_tape(mt_handle h, TapeArgs& r, uint64_t seed, bool auto_reset, bool select) {
  if (auto_reset) {
    h->args.seed_lo = (uint32_t)seed;  // as mt_reset_done(seed) leaves them
    h->args.seed_hi = (uint32_t)(seed >> 32);
    int rcg = order_behind_inplace_gather(h, h->stream);  // the in-kernel re-arm writes MT_F_LAST_RETURN
    if (rcg) return rcg;
  }
  r.auto_reset = auto_reset ? 1u : 0u;
  r.seed_lo = (uint32_t)seed;
  r.seed_hi = (uint32_t)(seed >> 32);
  r.radius = h->cfg.radius;
  if (select)
    launch_tape_select(h, h->args, r);
  else
    launch_tape(h, h->args, r);
  if (!r.dry_run) {
    h->args.flags &= ~kFlagWholeGoals;  // tape angles are anybody's floats
    h->codes_valid = false;             // the kernel writes targets as floats only
  }
  return check_launch(h, select ? "rollout_tape_kernel<SELECT>" : "rollout_tape_kernel");
}
// T steps of `tape` with the logs and the return row of `s` (a mt_tape, mt_shoot, mt_cem or mt_mppi: the same names)
template <class S>
static TapeArgs tape_args(const S* s, const float* tape, int64_t ld, int T) {
  TapeArgs r{};
  r.tape = tape;
  r.tape_ld = ld;
  r.reward_log = s->reward_log;
  r.done_log = s->done_log;
  r.log_ld = s->log_ld;
  r.return_out = s->return_out;
  r.T = T;
  return r;
}

// struct mt_cem and struct mt_mppi name the candidate stream, the refit and the commit alike; what the messages about
// them differ in: the struct's name, the prefix of its flags, its longest horizon.
struct PlanNames {
  const char *name, *flags;
  int max_steps;
};
constexpr PlanNames kCemNames{"mt_cem", "MT_CEM", 65535}, kMppiNames{"mt_mppi", "MT_MPPI", MT_MPPI_MAX_STEPS};
static_assert(MT_MPPI_AUTO_RESET == MT_CEM_AUTO_RESET && MT_MPPI_KEEP_MEAN == MT_CEM_KEEP_MEAN, "one set of flag bits");
static_assert(MT_MPPI_MAX_STEPS == kMppiMaxSteps, "the header's horizon limit is the kernel's table size");

// The candidate stream's parameters, checked and copied into the kernel's block; `who` goes ahead of every message
// ("mt_sample_plans: ", "mt_cem: ", nothing for mt_mppi).
template <class S, class Args>
static int stream_args(mt_handle h, const S* s, const char* who, const PlanNames& p, Args& e) {
  const std::string w = std::string(who) + p.name;
  MT_REQUIRE(h, s->n_steps >= 0 && s->n_steps <= p.max_steps, w + ".n_steps must be 0.." + std::to_string(p.max_steps));
  MT_REQUIRE(h, s->n_candidates >= 1 && s->n_candidates <= 64, w + ".n_candidates must be 1..64");
  MT_REQUIRE(h, (s->flags & ~(MT_CEM_AUTO_RESET | MT_CEM_KEEP_MEAN)) == 0, w + ".flags: unknown " + p.flags + "_* flag");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&s->lo, 1, kMaxAngleBits) < 0 && first_unusable(&s->hi, 1, kMaxAngleBits) < 0,
             w + ".lo / hi must be finite and within +-32768 degrees");
  MT_REQUIRE(h, s->lo <= s->hi, w + ".lo must be <= hi");
  e.mean = s->mean;
  e.sigma = s->sigma;
  e.ld = s->ld;
  e.T = s->n_steps;
  e.C = s->n_candidates;
  e.draw = s->draw;
  e.keep_mean = (s->flags & MT_CEM_KEEP_MEAN) ? 1u : 0u;
  e.seed_lo = (uint32_t)s->seed;
  e.seed_hi = (uint32_t)(s->seed >> 32);
  e.lo = s->lo;
  e.hi = s->hi;
  return MT_OK;
}
// ... and its rows, which a call with n_steps > 0 needs
template <class S>
static int stream_rows(mt_handle h, const S* s, const char* who, const PlanNames& p) {
  const std::string w = std::string(who) + p.name;
  MT_REQUIRE(h, s->mean != nullptr && s->sigma != nullptr, w + ".mean / sigma is NULL");
  MT_REQUIRE(h, s->ld >= h->n, w + ".ld is smaller than n_envs");
  return MT_OK;
}

// do [p, p + rows * ld) and [q, q + rows2 * ld2) share a byte?  (rows of n floats, the last one not padded)
static bool rows_overlap(const float* p, int64_t rows, int64_t ld, const float* q, int64_t rows2, int64_t ld2, int64_t n) {
  if (!p || !q || rows == 0 || rows2 == 0) return false;
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + (uintptr_t)(((rows - 1) * ld + n) * 4);
  const uintptr_t b0 = (uintptr_t)q, b1 = b0 + (uintptr_t)(((rows2 - 1) * ld2 + n) * 4);
  return a0 < b1 && b0 < a1;
}
static bool weights_fit(const struct mt_cem*, int64_t) { return true; }  // (no such output)
static bool weights_fit(const struct mt_mppi* s, int64_t n) { return !s->weights_out || s->w_ld >= n; }

// The layout rules of what a refit writes (mean_out / sigma_out, returns_out, chosen_out and the commit's logs; which of
// mean_out / sigma_out may be NULL is the entry point's own rule, checked ahead of this), then those outputs into the
// kernel's block.
template <class S, class Args>
static int refit_args(mt_handle h, const S* s, const PlanNames& p, Args& e) {
  const std::string w = std::string(p.name) + ".";
  const int H = s->commit_steps;
  const int64_t n = h->n, rows = (int64_t)s->n_steps * h->D;
  MT_REQUIRE(h, !s->mean_out || s->out_ld >= n, w + "out_ld is smaller than n_envs");
  MT_REQUIRE(h, !s->returns_out || s->ret_ld >= n, w + "ret_ld is smaller than n_envs");
  MT_REQUIRE(h, weights_fit(s, n), w + "w_ld is smaller than n_envs");
  MT_REQUIRE(h, !(H > 0 && s->chosen_out == nullptr), w + "chosen_out is NULL with commit_steps > 0");
  MT_REQUIRE(h, !(H > 0) || s->chosen_ld >= n, w + "chosen_ld is smaller than n_envs");
  MT_REQUIRE(h, !(H > 0 && (s->reward_log || s->done_log)) || s->log_ld >= n, w + "log_ld is smaller than n_envs");
  // the refit may sit EXACTLY on its input (same base, same pitch: every element is then read and written by one thread);
  // any other overlap of an output with mean / sigma or with the other output would let one block read another's writes
  const bool same_m = s->mean_out == s->mean && s->out_ld == s->ld, same_s = s->sigma_out == s->sigma && s->out_ld == s->ld;
  MT_REQUIRE(h, same_m || !rows_overlap(s->mean_out, rows, s->out_ld, s->mean, rows, s->ld, n), w + "mean_out overlaps mean without being mean");
  MT_REQUIRE(h, same_s || !rows_overlap(s->sigma_out, rows, s->out_ld, s->sigma, rows, s->ld, n), w + "sigma_out overlaps sigma without being sigma");
  MT_REQUIRE(h, !rows_overlap(s->mean_out, rows, s->out_ld, s->sigma, rows, s->ld, n), w + "mean_out overlaps sigma");
  MT_REQUIRE(h, !rows_overlap(s->sigma_out, rows, s->out_ld, s->mean, rows, s->ld, n), w + "sigma_out overlaps mean");
  MT_REQUIRE(h, !rows_overlap(s->mean_out, rows, s->out_ld, s->sigma_out, rows, s->out_ld, n), w + "mean_out overlaps sigma_out");
  if (H > 0) {
    const int64_t hr = (int64_t)H * h->D;
    MT_REQUIRE(h, !rows_overlap(s->chosen_out, hr, s->chosen_ld, s->mean, rows, s->ld, n) &&
                      !rows_overlap(s->chosen_out, hr, s->chosen_ld, s->sigma, rows, s->ld, n) &&
                      !rows_overlap(s->chosen_out, hr, s->chosen_ld, s->mean_out, rows, s->out_ld, n) &&
                      !rows_overlap(s->chosen_out, hr, s->chosen_ld, s->sigma_out, rows, s->out_ld, n),
               w + "chosen_out overlaps mean / sigma / mean_out / sigma_out");
  }
  e.mean_out = s->mean_out;
  e.sigma_out = s->sigma_out;
  e.out_ld = s->out_ld;
  e.returns_out = s->returns_out;
  e.ret_ld = s->ret_ld;
  e.best_out = s->best_out;
  e.best_return_out = s->best_return_out;
  e.chosen_out = H > 0 ? s->chosen_out : nullptr;
  e.chosen_ld = s->chosen_ld;
  e.H = H;
  e.sigma_min = s->sigma_min;
  return MT_OK;
}

extern "C" {

int mt_version(void) { return MT_VERSION; }

const char* mt_status_string(int status) {
  switch (status) {
    case MT_OK: return "ok";
    case MT_ERR_INVALID_ARG: return "invalid argument";
    case MT_ERR_HIP: return "HIP runtime error";
    case MT_ERR_NO_DEVICE: return "no usable HIP device";
    case MT_ERR_ALLOC: return "device allocation failed";
    case MT_ERR_STATE: return "invalid call order";
    case MT_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
  }
}

const char* mt_last_error(mt_handle h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int mt_device_count(int* count) {
  MT_REQUIRE(nullptr, count != nullptr, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    (void)hipGetLastError();
    return fail(nullptr, MT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return MT_OK;
}

int mt_create(mt_handle* out, const mt_config* cfg) {
  MT_REQUIRE(nullptr, out != nullptr && cfg != nullptr, "out/cfg is NULL");
  *out = nullptr;
  MT_REQUIRE(nullptr, cfg->struct_size == (int32_t)sizeof(mt_config), "mt_config.struct_size mismatch");
  MT_REQUIRE(nullptr, cfg->n_envs >= 1, "n_envs must be >= 1");
  MT_REQUIRE(nullptr, cfg->n_envs <= ((int64_t)1 << 30) - 256, "n_envs must be < 2^30 per handle (32-bit row offsets)");
  MT_REQUIRE(nullptr, cfg->dof >= 2 && cfg->dof <= MT_MAX_DOF, "dof must be in 2..8");
  MT_REQUIRE(nullptr, cfg->n_targets >= 1 && cfg->n_targets <= MT_MAX_TARGETS, "n_targets must be in 1..32");
  MT_REQUIRE(nullptr, cfg->substeps >= 2, "substeps must be >= 2");
  MT_REQUIRE(nullptr, cfg->pickup_tol >= 0.f && cfg->radius > 0.f, "pickup_tol/radius out of range");
  // the kernels are built with -ffinite-math-only: every float that reaches them is screened on its bit pattern at the door
  MT_REQUIRE(nullptr, first_unusable(&cfg->pickup_tol, 1, kMaxFiniteBits) < 0 && first_unusable(&cfg->radius, 1, kMaxFiniteBits) < 0,
             "pickup_tol / radius must be finite");
  MT_REQUIRE(nullptr, first_unusable(cfg->dh_table, (int64_t)cfg->dof * 4, kMaxFiniteBits) < 0, "dh_table holds a NaN or an infinity");
  MT_REQUIRE(nullptr, cfg->env_id_base >= 0, "env_id_base must be >= 0");
  MT_REQUIRE(nullptr, cfg->return_ring >= 0 && cfg->return_ring <= MT_MAX_RETURN_RING, "return_ring must be in 0..64");
  MT_REQUIRE(nullptr, cfg->reserved == 0, "mt_config.reserved must be 0");
  MT_REQUIRE(nullptr, cfg->obs_frame >= -cfg->dof && cfg->obs_frame < cfg->dof, "obs_frame must be in -dof..dof-1");
  MT_REQUIRE(nullptr, cfg->ee_frame >= -cfg->dof && cfg->ee_frame < cfg->dof, "ee_frame must be in -dof..dof-1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(nullptr, MT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
  }
  MT_REQUIRE(nullptr, cfg->device >= 0 && cfg->device < ndev, "device ordinal out of range");

  mt_engine* h = new (std::nothrow) mt_engine();
  if (!h) return fail(nullptr, MT_ERR_ALLOC, "out of host memory");
  h->cfg = *cfg;
  h->n = cfg->n_envs;
  h->ld = (int64_t)align_up((size_t)cfg->n_envs, 256);
  // Rows that are an exact power of two apart alias onto the same HBM channels, so every row gets a pad.  1 KiB
  // (256 floats): round 1 used 4 KiB, which is fine at 1 M arms but pathological at 262 144 (row stride 1 MiB + 4 KiB:
  // 14.7 us per step against 11.7 with 1 KiB; tools/pad_sweep.py, profiles/r02_variants.md section 6); 1 KiB is within
  // 1 % of the best pad at every size tried.  MT_LD_PAD (floats) overrides it for experiments.
  int64_t pad = (cfg->n_envs > kPolicy.ld_pad_above) ? kPolicy.ld_pad_floats : 0;
  if (const char* env = std::getenv("MT_LD_PAD")) pad = (int64_t)align_up((size_t)std::atoll(env), 64);
  h->ld += pad;
  h->D = cfg->dof;
  h->K = cfg->n_targets;

  auto bail = [&](int code, const std::string& msg) {
    g_last_error = msg;
    if (h->arena) (void)hipFree(h->arena);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return code;
  };
#define MT_HIP_C(call)                                                                       \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) return bail(MT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

  DeviceGuard guard(cfg->device);
  if (guard.error() != hipSuccess) return bail(MT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.error()));
  MT_HIP_C(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  MT_HIP_C(hipEventCreateWithFlags(&h->ev0, event_flags(true)));
  MT_HIP_C(hipEventCreateWithFlags(&h->ev1, event_flags(true)));

  // arena layout: every row block starts on a 1 KiB boundary
  const size_t ld = (size_t)h->ld, D = (size_t)h->D, K = (size_t)h->K;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = align_up(off + bytes, 1024);
    return o;
  };
  const size_t o_act = take(D * ld * 4), o_goal = take(D * ld * 4), o_pts = take(3 * K * ld * 4),
               o_obs = take(3 * K * ld * 4), o_alive = take(ld * 4), o_tot = take(ld * 4), o_rew = take(ld * 4),
               o_done = take(ld), o_bits = take(ld / 64 * 8), o_ee = take(3 * ld * 4), o_epi = take(ld * 4),
               o_last = take(ld * 4), o_ring = take((size_t)cfg->return_ring * ld * 4), o_misc = take(256),
               o_trace = take((cfg->flags & MT_FLAG_TRACE) ? (size_t)cfg->substeps * 3 * ld * 4 : 0),
               o_zmin = take((cfg->flags & MT_FLAG_DEBUG_ZMIN) ? ld * 4 : 0), o_trig = take(kTrigEntries * sizeof(SinCos)),
               o_codes = take(2 * K * ld * 4);
  h->arena_bytes = off;
  // (One experiment with hipExtMallocWithFlags(hipDeviceMallocContiguous) instead -- a physically contiguous arena -- cost 5 %
  // at 1 M arms and was dropped the same day: profiles/r04_variants.md section 3.)
  if (hipMalloc(&h->arena, h->arena_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return bail(MT_ERR_ALLOC, "hipMalloc of the state arena failed (" + std::to_string(h->arena_bytes) + " bytes)");
  }
  MT_HIP_C(hipMemsetAsync(h->arena, 0, h->arena_bytes, h->stream));
  char* base = (char*)h->arena;
  StepArgs& a = h->args;
  a.actions = (float*)(base + o_act);
  a.goals = (float*)(base + o_goal);
  a.points = (float*)(base + o_pts);
  a.codes = (uint32_t*)(base + o_codes);
  a.obs = (float*)(base + o_obs);
  a.alive = (uint32_t*)(base + o_alive);
  a.total_reward = (float*)(base + o_tot);
  a.reward = (int32_t*)(base + o_rew);
  a.done = (uint8_t*)(base + o_done);
  a.done_bits = (unsigned long long*)(base + o_bits);
  a.ee = (float*)(base + o_ee);
  a.episodes = (uint32_t*)(base + o_epi);
  a.last_return = (float*)(base + o_last);
  a.ring = cfg->return_ring ? (float*)(base + o_ring) : nullptr;
  a.ring_slots = (uint32_t)cfg->return_ring;
  a.episode0 = 0;
  a.bad_actions = (uint32_t*)(base + o_misc);                 // word 0 of the misc block
  h->spare_bits = (unsigned long long*)(base + o_misc + 64);  // ballot sink of single-env launches
  h->trace = (cfg->flags & MT_FLAG_TRACE) ? (float*)(base + o_trace) : nullptr;
  a.zmin = (cfg->flags & MT_FLAG_DEBUG_ZMIN) ? (float*)(base + o_zmin) : nullptr;
  a.snap = nullptr;  // set on copies of the arguments only: the last step launch of an mt_rollout (chained form)
  a.trig_table = (const float*)(base + o_trig);
  hipLaunchKernelGGL(fill_trig_table_kernel, dim3(1), dim3(kBlock), 0, h->stream, (float*)(base + o_trig));
  MT_HIP_C(hipGetLastError());
  a.n = h->n;
  a.ld = h->ld;
  a.env_base = cfg->env_id_base;
  a.K = h->K;
  a.S = cfg->substeps;
  a.tol = cfg->pickup_tol;
  a.radius = cfg->radius;
  a.inv_sm1 = 1.0f / (float)(cfg->substeps - 1);
  a.flags = cfg->flags & ~kFlagWholeGoals;  // the internal bit is the host's to set (resets / sampled steps), never the caller's
  a.dh = make_dh(cfg->dh_table, h->D);
  a.dh.fo = (cfg->obs_frame + h->D) % h->D;
  a.dh.fe = (cfg->ee_frame + h->D) % h->D;
  // other rows than the reference's last two: the runtime-table kernel with runtime frames (RtTableF), one env per lane
  choose_dispatch(h);
#undef MT_HIP_C
  *out = h;
  return MT_OK;
}

int mt_destroy(mt_handle h) {
  if (!h) return MT_OK;
  DeviceGuard guard(h->cfg.device);
  (void)hipStreamSynchronize(h->stream);
  mt_gather_release(h);  // drains the side stream before the communicator goes
  mt_comm_release(h);
  for (auto& g : h->graphs)
    for (hipGraphExec_t x : g.exec)
      if (x) (void)hipGraphExecDestroy(x);
  for (int c = 1; c < mt_engine::kMaxChains; ++c) {
    if (h->chain_streams[c]) {
      (void)hipStreamSynchronize(h->chain_streams[c]);
      (void)hipStreamDestroy(h->chain_streams[c]);
    }
    if (h->ev_join[c]) (void)hipEventDestroy(h->ev_join[c]);
    if (h->ev1c[c]) (void)hipEventDestroy(h->ev1c[c]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->graph_step0) (void)hipFree(h->graph_step0);
  if (h->staging) (void)hipFree(h->staging);
  if (h->pinned) (void)hipHostFree(h->pinned);
  if (h->arena) (void)hipFree(h->arena);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  for (hipEvent_t e : h->lap_events) (void)hipEventDestroy(e);  // (the whole pool)
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return MT_OK;
}

// What mt_step_kernel_name and mt_describe_dispatch report: the plans of a sampled-action launch of the whole batch and of
// one chain's span (the same values launch_step resolves; "trig" is the handle's, which the LDS-table and runtime-frame
// kernels do not all implement: plan_step).
static StepPlan batch_plan(const mt_engine* h) { return plan_step(h, mt_engine::kBatch, h->n, true, false); }
static StepPlan chain_plan(const mt_engine* h) { return plan_step(h, mt_engine::kChain, chain_span(h, h->chains), true, false); }
static std::string table_name(const mt_engine* h) {
  const char* tbl = h->static_kind == 1 ? "Ref4Table" : (h->static_kind == 2 ? "Dh7Table" : nullptr);
  return tbl ? tbl : (h->custom_frames ? "RtTableF<" : "RtTable<") + std::to_string(h->D) + ">";
}
// mt_rollout's multi-step launches run per chain only where MT_CHAINS asks for it
static int multi_step_lanes(const mt_engine* h) {
  return h->sched[(h->chains > 1 && h->chains_forced) ? mt_engine::kChain : mt_engine::kBatch].rollout_lanes;
}

const char* mt_step_kernel_name(mt_handle h) {
  if (!h) return "";
  const std::string table = table_name(h);
  const StepVariant v = batch_plan(h).v;
  if (v.lanes > 1)
    h->kernel_name = "step_split_kernel<" + table + ", L=" + std::to_string(v.lanes) + (v.tt ? ", tt=1>" : ">");
  else
    h->kernel_name = "step_kernel<" + table + ", trig=" + std::to_string(h->trig) + ", lds=" + (v.lds ? "true" : "false") +
                     ", pf=" + std::to_string(v.pf) + (v.tt ? ", tt=1" : "") + (v.flat ? ", flat=1>" : ">");
  const bool multi_one_chain = h->multi_k > 1 && fusable(h) && !h->chains_forced;  // mt_rollout does not use the chains then
  if (h->chains > 1 && !multi_one_chain) {  // what mt_rollout launches instead: the schedule for a chain's env count, on row views
    const StepPlan c = chain_plan(h);
    h->kernel_name += " [mt_rollout: " + std::to_string(h->chains) + " chains of " + std::to_string(chain_span(h, h->chains)) +
                      " envs, " + (c.v.lanes > 1 ? "L=" + std::to_string(c.v.lanes)
                                                 : "pf=" + std::to_string(c.v.pf) + (c.v.flat ? ", flat=1" : "")) +
                      (c.blocks_per_cu > 0 ? ", " + std::to_string(c.blocks_per_cu) + " blocks/CU" : std::string()) + "]";
  }
  if (h->multi_k > 1 && fusable(h)) {  // what mt_rollout launches on small shards instead of one step kernel per step
    const int sp = multi_step_lanes(h);
    h->kernel_name += " [mt_rollout: " + std::to_string(h->multi_k) + " steps per launch, " +
                      (sp > 1 ? "rollout_split_kernel L=" + std::to_string(sp) : std::string("rollout_kernel")) + "]";
  }
  return h->kernel_name.c_str();
}

const char* mt_describe_dispatch(mt_handle h) {
  if (!h) return "";
  const DispatchPolicy& P = kPolicy;
  auto num = [](long long v) { return std::to_string(v); };
  auto b = [](bool v) { return std::string(v ? "true" : "false"); };
  const int64_t span = chain_span(h, h->chains);
  const std::string table = table_name(h);
  const StepPlan sb = batch_plan(h), sc = chain_plan(h);
  const bool multi = h->multi_k > 1 && fusable(h);
  const bool graph = h->graph_mode > 0 || (h->graph_mode < 0 && h->n <= h->graph_max);
  const bool rederive_on = h->goals_rederive && !h->goals_exposed && !h->goals_foreign && !h->points_exposed && !h->trace;
  auto rederives = [&](const StepPlan& p) {  // (sb: a launch of the whole batch; sc: of a chain's span)
    return rederive_on && p.v.lanes == 1 && p.v.pf != 0 && p.v.tt && (&p == &sb ? h->n : span) <= h->goals_rederive_max_envs;
  };
  std::string caps = "[";
  for (const BlockCap& c : P.block_caps) caps += std::string(caps.size() > 1 ? "," : "") + "[" + num(c.from) + "," + num(c.below) + "," + num(c.blocks) + "]";
  caps += "]";
  std::string& d = h->describe;
  d = "{\"n_envs\":" + num(h->n) + ",\"ld\":" + num(h->ld) + ",\"dof\":" + num(h->D) + ",\"targets\":" + num(h->K) +
      ",\"table\":\"" + table + "\",\"trig\":" + num(h->trig) + ",\"lds_table\":" + b(h->lds_table) + ",\"custom_frames\":" + b(h->custom_frames) +
      // one launch per step: mt_step / mt_step_random on a one-chain handle
      ",\"step\":{\"lanes_per_env\":" + num(sb.v.lanes) + ",\"prefetch\":" + b(sb.v.pf != 0) +
      ",\"trig_table\":" + b(sb.v.tt) + ",\"flat\":" + b(sb.v.flat) + "}" +
      // per-chain calls: mt_rollout, mt_step, mt_sample_actions, mt_set_actions(device), mt_reset_random
      ",\"chains\":{\"count\":" + num(h->chains) + ",\"span\":" + num(h->chains > 1 ? span : h->n) + ",\"lazy\":" + b(h->lazy_chains) +
      ",\"lanes_per_env\":" + num(sc.v.lanes) + ",\"prefetch\":" + b(sc.v.pf != 0) + ",\"flat\":" + b(sc.v.flat) +
      ",\"blocks_per_cu\":" + num(h->chains > 1 ? sc.blocks_per_cu : 0) + "}" +
      ",\"rollout\":{\"form\":\"" + (multi ? "multi_step" : (h->chains > 1 ? "chained_steps" : (graph ? "graph_replay" : "launch_per_step"))) +
      "\",\"steps_per_launch\":" + num(multi ? h->multi_k : 1) + ",\"graph\":" + b(!multi && graph) +
      ",\"lanes_per_env\":" + num(multi ? multi_step_lanes(h) : (h->chains > 1 ? sc : sb).v.lanes) +
      ",\"chains\":" + num(multi && !h->chains_forced ? 1 : h->chains) +
      ",\"absorbs_reset\":" + b(h->defer_reset && (multi || chained_rollout_absorbs_reset(h))) + ",\"writes_snapshot\":" + b(h->snap_in_rollout && (multi || (h->chains > 1 && !graph && !h->trace))) + "}" +
      ",\"fused\":{\"usable\":" + b(fusable(h)) + ",\"lanes_per_env\":" + num(h->sched[mt_engine::kBatch].rollout_lanes) + "}" +
      // mt_rollout_tape: one form for every batch size (the lane-split and two-chain forms do not exist for it)
      ",\"tape\":{\"usable\":" + b(fusable(h)) + ",\"lanes_per_env\":1,\"chains\":1,\"prefetch\":" + b(tape_prefetches(h)) +
      ",\"nt_loads\":" + b(h->tape_nt_loads) + "}" +
      // mt_shoot: a block scores all candidates of 64 envs, one wave per candidate at a time
      ",\"shoot\":{\"usable\":" + b(fusable(h)) + ",\"envs_per_block\":" + num(kShootEnvs) + ",\"waves_per_block\":" + num(kShootWaves) + "}" +
      // mt_cem: shoot's shape, the candidates drawn in the kernel
      ",\"cem\":{\"usable\":" + b(fusable(h)) + ",\"envs_per_block\":" + num(kShootEnvs) + ",\"waves_per_block\":" + num(kShootWaves) +
      ",\"max_candidates\":64}" +
      // mt_mppi: cem's shape, every candidate weighted by a power of decay
      ",\"mppi\":{\"usable\":" + b(fusable(h)) + ",\"envs_per_block\":" + num(kShootEnvs) + ",\"waves_per_block\":" + num(kShootWaves) +
      ",\"max_candidates\":64,\"max_steps\":" + num(kMppiMaxSteps) + "}" +
      // mt_rollout_policy: the tape kernel's shape; hidden vectors in register arrays of one of two compiled extents
      ",\"policy_rollout\":{\"usable\":" + b(fusable(h)) + ",\"lanes_per_env\":1,\"hidden_extents\":[32,64]}" +
      ",\"reset\":{\"lanes_per_env\":" + num(h->reset_split ? 4 : 1) + "}" +
      // the ground test's interior poses on dense lanes of the block: the step launches that take it (the single-env view,
      // the rollout, tape and shoot kernels never do)
      ",\"ground_compact\":{\"enabled\":" + b(h->ground_compact) + ",\"step\":" + b(sb.v.gc) + ",\"chains\":" + b(sc.v.gc) + "}" +
      // the pose a sampled step starts from re-derived (zero pose / the previous launch's action draw) instead of loaded: by
      // the code-reading launches, while the host knows the row (engine_internal.h, GoalsRow).  "rederive": mt_rollout's
      // step launches do; "step" / "chains": a launch over the whole batch / over a chain's span can
      ",\"goals\":{\"rederive\":" + b(!multi && !graph && rederives(h->chains > 1 ? sc : sb)) + ",\"enabled\":" + b(h->goals_rederive) +
      ",\"step\":" + b(rederives(sb)) + ",\"chains\":" + b(rederives(sc)) +
      ",\"chains_rederiving\":" + num(rederives(sc) ? std::min(h->chains, h->goals_rederive_chains) : 0) +
      ",\"launches_rederived\":" + num((long long)h->goals_rederived) + "}" +
      ",\"overrides\":\"" + h->overrides + "\"" +
      ",\"policy\":{\"step_split4_max\":" + num(P.step_split4_max) + ",\"step_split2_max\":" + num(P.step_split2_max) +
      ",\"prefetch_other_max\":" + num(P.prefetch_other_max) + ",\"fused_split4_max\":" + num(P.fused_split4_max) +
      ",\"fused_split2_max\":" + num(P.fused_split2_max) + ",\"reset_split_max\":" + num(P.reset_split_max) +
      ",\"graph_max\":" + num(P.graph_max) + ",\"chains_min\":" + num(P.chains_min) + ",\"chains_max\":" + num(P.chains_max) +
      ",\"chain_split4_max\":" + num(P.chain_split4_max) + ",\"chain_split2_max\":" + num(P.chain_split2_max) +
      ",\"chain_prefetch_other_max\":" + num(P.chain_prefetch_other_max) + ",\"flat_from\":" + num(P.flat_from) +
      ",\"block_caps\":" + caps + ",\"multi_step_max\":" + num(P.multi_step_max) + ",\"multi_step_k\":" + num(P.multi_step_k) +
      ",\"max_recurrence_rotations\":" + num(P.max_recurrence_rotations) + ",\"ld_pad_above\":" + num(P.ld_pad_above) +
      ",\"ld_pad_floats\":" + num(P.ld_pad_floats) + ",\"rederive_goals_ref4\":" + b(P.rederive_goals_ref4) +
      ",\"rederive_goals_dh7\":" + b(P.rederive_goals_dh7) + ",\"rederive_goals_chains\":" + num(P.rederive_goals_chains) +
      ",\"rederive_goals_max_envs\":" + num(P.rederive_goals_max_envs) + "}" +
      ",\"arena_bytes\":" + num((long long)h->arena_bytes) + "}";
  return d.c_str();
}

int mt_set_stream(mt_handle h, void* hip_stream) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ENTER(h);
  MT_HIP(h, hipStreamSynchronize(h->stream));   // everything queued so far is finished before the ordering changes
  h->stream = (hipStream_t)hip_stream;          // NULL is a stream too: the legacy default stream
  // (on a caller's stream the library's calls can be captured into the caller's graphs: mt::note_capture watches for that)
  return MT_OK;
}

int mt_use_own_stream(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ENTER(h);
  MT_HIP(h, hipStreamSynchronize(h->stream));
  h->stream = h->own_stream;
  return MT_OK;
}

int mt_sync(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ENTER_KEEP(h);  // (also: the NULL stream names the CURRENT device's default stream)
  MT_HIP(h, hipStreamSynchronize(h->stream));
  if (h->gather_pending) {  // a gather begun on the side stream is part of "everything queued on this handle"
    MT_HIP(h, hipStreamSynchronize(h->side_stream));
    MT_HIP(h, hipEventElapsedTime(&h->last_gather_ms, h->ev_g0, h->ev_g1));
    h->gather_pending = false;
    h->snap_free_known[0] = h->snap_free_known[1] = true;  // every exchange has finished
  }
  return MT_OK;
}

// ---- reset ------------------------------------------------------------------------------------
int mt_reset(mt_handle h, const float* points, int layout, int is_device) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, points != nullptr, "points is NULL (use mt_reset_random for device-drawn targets)");
  MT_REQUIRE(h, layout == MT_ENV_MAJOR || layout == MT_SOA, "bad layout");
  if (!is_device && layout == MT_ENV_MAJOR) {
    const int64_t bad = first_unusable(points, h->n * 3 * h->K, kMaxFiniteBits);
    if (bad >= 0) return fail(h, MT_ERR_INVALID_ARG, "mt_reset: points element " + std::to_string(bad) + " is NaN or infinite");
  }
  if (!is_device && layout == MT_SOA)
    for (int r = 0; r < 3 * h->K; ++r) {  // the n live columns of every row (the pad is the caller's garbage)
      const int64_t bad = first_unusable(points + (int64_t)r * h->ld, h->n, kMaxFiniteBits);
      if (bad >= 0)
        return fail(h, MT_ERR_INVALID_ARG, "mt_reset: points row " + std::to_string(r) + " element " + std::to_string(bad) + " is NaN or infinite");
    }
  // (targets handed over in DEVICE memory cannot be screened here: reset_kernel drops an unusable one -- dead from the
  // start, coordinates zeroed -- and counts it, see mt_bad_action_count)
  MT_ENTER(h);
  const int rows = 3 * h->K;
  if (layout == MT_SOA) {
    const size_t bytes = (size_t)rows * h->ld * 4;
    MT_HIP(h, hipMemcpyAsync(h->args.points, points, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                             h->stream));
  } else {
    const size_t bytes = (size_t)rows * h->n * 4;
    const float* src = points;
    if (!is_device) {
      int rc = ensure_staging(h, bytes);
      if (rc) return rc;
      MT_HIP(h, hipMemcpyAsync(h->staging, points, bytes, hipMemcpyHostToDevice, h->stream));
      src = (const float*)h->staging;
    }
    hipLaunchKernelGGL((env_major_to_soa<float>), grid_for(h->n), dim3(kBlock), 0, h->stream, src, rows, h->n,
                       h->args.points, h->ld);
    int rc = check_launch(h, "env_major_to_soa");
    if (rc) return rc;
  }
  {
    int rcg = order_behind_inplace_gather(h, h->stream);
    if (rcg) return rcg;
  }
  h->args.major = 0;  // caller-supplied targets start episode 0 of every env
  h->args.episode0 = 0;
  if (!h->goals_exposed) h->args.flags |= kFlagWholeGoals;  // every env is at the zero pose after this launch
  MT_DISPATCH_D(h->D, launch_reset_d, h, h->args, 0);
  int rc = check_launch(h, "reset_kernel");
  if (rc) return rc;
  h->goals_are(mt_engine::GoalsRow::kZero);
  if (!is_device) MT_HIP(h, hipStreamSynchronize(h->stream));  // the caller may free `points` on return
  h->is_reset = true;
  return MT_OK;
}

// mode 1: full random reset; 2: re-arm finished envs only.  The launches themselves (no deferral).
static int launch_reset_random(mt_handle h, uint64_t seed, uint32_t episode, int mode) {
  // A full random reset of a multi-chain handle is issued per chain, behind that chain's own last step, and leaves the
  // chains forked: one range's reset runs beside the other range's last step instead of behind a join.
  // (only WHILE they are forked: behind a joined call -- the multi-step mt_rollout of small shards, a getter -- the reset
  // is one launch on the handle's stream, and whoever forks next forks behind it)
  const bool per_chain = mode == 1 && h->chains > 1 && h->lazy_chains && h->forked;
  if (!per_chain) {
    int rc = join_chains(h);
    if (rc) return rc;
  }
  h->args.seed_lo = (uint32_t)seed;
  h->args.seed_hi = (uint32_t)(seed >> 32);
  h->args.major = episode;
  if (mode == 1) {
    h->args.episode0 = episode;  // full reset: finished-episode counts restart from here
    if (!h->goals_exposed) h->args.flags |= kFlagWholeGoals;  // every env is at the zero pose after this launch
  }
  h->forget_goals();  // (a re-arm zeroes the pose of the finished envs only; a full reset says "zero" once it is launched)
  if (per_chain) {
    int rc = fork_chains(h, h->chains);
    if (rc) return rc;
    const int64_t span = chain_span(h, h->chains);
    hipStream_t root = h->stream;
    for (int c = 0; c < h->chains && rc == MT_OK; ++c) {
      const int64_t off = (int64_t)c * span;
      if (off >= h->n) continue;
      const StepArgs ar = args_for_range(h, h->args, off, std::min(span, h->n - off));
      h->stream = c == 0 ? root : h->chain_streams[c];
      rc = order_behind_inplace_gather(h, h->stream);
      if (rc == MT_OK) MT_DISPATCH_D(h->D, launch_reset_d, h, ar, 1);
    }
    h->stream = root;
    if (rc == MT_OK) rc = check_launch(h, "reset_kernel (per chain)");
    if (rc) return rc;
    h->codes_valid = !h->points_exposed;  // every chain's range drew its targets: codes and floats
    h->goals_are(mt_engine::GoalsRow::kZero);  // ... and sits at the zero pose
    h->is_reset = true;
    return settle_chains(h);
  }
  int rc = order_behind_inplace_gather(h, h->stream);
  if (rc) return rc;
  MT_DISPATCH_D(h->D, launch_reset_d, h, h->args, mode);
  rc = check_launch(h, "reset_kernel");
  if (rc) return rc;
  if (mode == 1) {
    h->codes_valid = !h->points_exposed;  // (a re-arm keeps them as they were: it rewrites what it draws)
    h->goals_are(mt_engine::GoalsRow::kZero);
  }
  h->is_reset = true;
  return MT_OK;
}

}  // extern "C" (interrupted: the next function has C++ linkage, engine_internal.h)

namespace mt {
int flush_pending_reset(mt_handle h) {
  if (!h->reset_pending) return MT_OK;
  h->reset_pending = false;
  return launch_reset_random(h, h->pend_seed, h->pend_episode, 1);
}
}  // namespace mt

extern "C" {

static int reset_random_impl(mt_handle h, uint64_t seed, uint32_t episode, int mode) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ON_DEVICE(h, h->cfg.device);
  h->snap_valid = false;
  note_capture(h);
  int rc = flush_pending_reset(h);  // an earlier deferred reset comes first (its last_return is what this one overwrites)
  if (rc) return rc;
  // A full reset of a handle whose mt_rollout runs k steps per launch is DEFERRED into the first launch of the next
  // mt_rollout (RolloutArgs::reset_first: the same state, bit for bit, without the reset's launch and without re-fetching what
  // it would have written: an episode end of a 131 072-env shard goes from 20 to 6 us on the device, tools/episode_end_cost.py).
  // Any other entry point launches it first (MT_ENTER).  Not while the chains are forked (the per-chain reset above), and
  // only on the handle's OWN stream: there the contract already is "mt_sync before anything else looks at the state" (and
  // mt_sync launches it); on a caller's stream the contract is stream order, and whatever the caller queues next without
  // calling the library -- a replay of a graph captured from mt_step, a torch kernel on a view it holds -- has to find
  // the reset done.
  if (mode == 1 && h->defer_reset && h->stream == h->own_stream &&
      ((rollout_is_multi_step(h) && !h->forked) || chained_rollout_absorbs_reset(h))) {
    h->args.seed_lo = (uint32_t)seed;
    h->args.seed_hi = (uint32_t)(seed >> 32);
    h->args.major = episode;
    h->args.episode0 = episode;
    if (!h->goals_exposed) h->args.flags |= kFlagWholeGoals;
    h->forget_goals();  // until the reset has run: as the prologue of a step launch (launch_step_fresh) or when it is flushed
    h->reset_pending = true;
    h->pend_seed = seed;
    h->pend_episode = episode;
    h->is_reset = true;
    return MT_OK;
  }
  return launch_reset_random(h, seed, episode, mode);
}

int mt_reset_random(mt_handle h, uint64_t seed, uint32_t episode) { return reset_random_impl(h, seed, episode, 1); }

int mt_reset_done(mt_handle h, uint64_t seed) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_reset_done before the first reset");
  return reset_random_impl(h, seed, 0, 2);
}

// ---- actions ----------------------------------------------------------------------------------
int mt_set_actions(mt_handle h, const void* actions, int dtype, int layout, int is_device) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, actions != nullptr, "actions is NULL");
  MT_REQUIRE(h, layout == MT_ENV_MAJOR || layout == MT_SOA, "bad layout");
  MT_REQUIRE(h, dtype == MT_F32 || dtype == MT_F64 || dtype == MT_I32 || dtype == MT_I64, "bad action dtype");
  const size_t es = (dtype == MT_F32 || dtype == MT_I32) ? 4 : 8;
  // Device sources of a multi-chain handle are staged per chain -- each range's rows on its chain's stream, right ahead of
  // that range's mt_step -- so that a policy loop (mt_set_actions(device) / mt_step, ...) keeps the chains forked.
  const int chains = is_device ? usable_chains(h, true) : 1;
  if (chains > 1) {
    MT_ON_DEVICE(h, h->cfg.device);
    const int D = h->D;
    const int64_t ld = h->ld;
    hipError_t copy_err = hipSuccess;
    int rc = per_chain(h, chains, "set_actions (per chain)", [&](int, int64_t off, int64_t cnt) {
      const dim3 g = grid_for(cnt), b(kBlock);
      float* dst = h->args.actions + off;
      if (layout == MT_SOA && dtype == MT_F32) {
        hipError_t e = hipMemcpy2DAsync(dst, (size_t)ld * 4, (const float*)actions + off, (size_t)ld * 4, (size_t)cnt * 4, (size_t)D,
                                        hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) copy_err = e;
      } else if (layout == MT_ENV_MAJOR) {
        const char* src = (const char*)actions + (size_t)off * D * es;
        switch (dtype) {
          case MT_F32: hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)src, D, cnt, dst, ld); break;
          case MT_F64: hipLaunchKernelGGL((env_major_to_soa<double>), g, b, 0, h->stream, (const double*)src, D, cnt, dst, ld); break;
          case MT_I32: hipLaunchKernelGGL((env_major_to_soa<int32_t>), g, b, 0, h->stream, (const int32_t*)src, D, cnt, dst, ld); break;
          default: hipLaunchKernelGGL((env_major_to_soa<int64_t>), g, b, 0, h->stream, (const int64_t*)src, D, cnt, dst, ld); break;
        }
      } else {
        const char* src = (const char*)actions + (size_t)off * es;
        switch (dtype) {
          case MT_F64: hipLaunchKernelGGL((soa_to_soa_f32<double>), g, b, 0, h->stream, (const double*)src, D, cnt, ld, dst); break;
          case MT_I32: hipLaunchKernelGGL((soa_to_soa_f32<int32_t>), g, b, 0, h->stream, (const int32_t*)src, D, cnt, ld, dst); break;
          default: hipLaunchKernelGGL((soa_to_soa_f32<int64_t>), g, b, 0, h->stream, (const int64_t*)src, D, cnt, ld, dst); break;
        }
      }
    });
    if (rc) return rc;
    if (copy_err != hipSuccess) return fail(h, MT_ERR_HIP, std::string("hipMemcpy2DAsync (actions): ") + hipGetErrorString(copy_err));
    return MT_OK;
  }
  MT_ENTER(h);
  const int64_t cols = (layout == MT_SOA) ? h->ld : h->n;
  const size_t bytes = (size_t)h->D * cols * es;
  const void* src = actions;
  if (layout == MT_SOA && dtype == MT_F32) {
    MT_HIP(h, hipMemcpyAsync(h->args.actions, actions, bytes,
                             is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!is_device) MT_HIP(h, hipStreamSynchronize(h->stream));
    return MT_OK;
  }
  if (!is_device) {
    int rc = ensure_staging(h, bytes);
    if (rc) return rc;
    MT_HIP(h, hipMemcpyAsync(h->staging, actions, bytes, hipMemcpyHostToDevice, h->stream));
    src = h->staging;
  }
  const dim3 g = grid_for(h->n), b(kBlock);
  if (layout == MT_ENV_MAJOR) {
    switch (dtype) {
      case MT_F32: hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)src, h->D, h->n, h->args.actions, h->ld); break;
      case MT_F64: hipLaunchKernelGGL((env_major_to_soa<double>), g, b, 0, h->stream, (const double*)src, h->D, h->n, h->args.actions, h->ld); break;
      case MT_I32: hipLaunchKernelGGL((env_major_to_soa<int32_t>), g, b, 0, h->stream, (const int32_t*)src, h->D, h->n, h->args.actions, h->ld); break;
      default: hipLaunchKernelGGL((env_major_to_soa<int64_t>), g, b, 0, h->stream, (const int64_t*)src, h->D, h->n, h->args.actions, h->ld); break;
    }
  } else {
    switch (dtype) {
      case MT_F64: hipLaunchKernelGGL((soa_to_soa_f32<double>), g, b, 0, h->stream, (const double*)src, h->D, h->n, h->ld, h->args.actions); break;
      case MT_I32: hipLaunchKernelGGL((soa_to_soa_f32<int32_t>), g, b, 0, h->stream, (const int32_t*)src, h->D, h->n, h->ld, h->args.actions); break;
      default: hipLaunchKernelGGL((soa_to_soa_f32<int64_t>), g, b, 0, h->stream, (const int64_t*)src, h->D, h->n, h->ld, h->args.actions); break;
    }
  }
  int rc = check_launch(h, "set_actions");
  if (rc) return rc;
  if (!is_device) MT_HIP(h, hipStreamSynchronize(h->stream));
  return MT_OK;
}

int mt_sample_actions(mt_handle h, uint64_t seed, uint32_t step_idx) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const int chains = usable_chains(h, true);
  if (chains > 1) {  // per chain: each range's actions are written on its chain's stream, ahead of that range's mt_step
    MT_ON_DEVICE(h, h->cfg.device);
    return per_chain(h, chains, "sample_actions_kernel (per chain)", [&](int, int64_t off, int64_t cnt) {
      hipLaunchKernelGGL(sample_actions_kernel, grid_for(cnt), dim3(kBlock), 0, h->stream, h->args.actions + off, cnt, h->ld, h->D,
                         h->args.env_base + off, seed, step_idx);
    });
  }
  MT_ENTER(h);
  hipLaunchKernelGGL(sample_actions_kernel, grid_for(h->n), dim3(kBlock), 0, h->stream, h->args.actions, h->n, h->ld,
                     h->D, h->args.env_base, seed, step_idx);
  return check_launch(h, "sample_actions_kernel");
}

// ---- step -------------------------------------------------------------------------------------
int mt_step(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_step before mt_reset / mt_reset_random");
  // The policy-in-the-loop step: on a multi-chain handle each half of the env range is one launch on its own stream, as in
  // mt_rollout (a step of env i depends only on env i: same bits, one half's kernel boundary behind the other's kernel).
  // On the handle's own stream the chains stay forked across mt_set_actions(device) / mt_sample_actions / mt_step calls;
  // on a caller's stream (a torch policy on the same stream) the step is one launch (see usable_chains).
  const int chains = usable_chains(h, true);
  if (chains > 1) {
    MT_ON_DEVICE(h, h->cfg.device);
    h->snap_valid = false;
    note_capture(h);
    {
      int rcf = flush_pending_reset(h);
      if (rcf) return rcf;
    }
    const StepArgs a = h->args;
    int rc = per_chain(h, chains, "step_kernel (per chain)", [&](int c, int64_t, int64_t) { launch_chain(h, a, a.major, 1, chains, c, false); });
    h->args.flags &= ~kFlagWholeGoals;  // staged actions are anybody's floats
    return rc;
  }
  MT_ENTER(h);
  launch_step(h, false);
  h->args.flags &= ~kFlagWholeGoals;  // staged actions are anybody's floats
  return check_launch(h, "step_kernel");
}

int mt_step_host(mt_handle h, const void* actions, int dtype, float* obs, int32_t* reward, uint8_t* done) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, actions && obs && reward && done, "NULL argument");
  MT_REQUIRE(h, dtype == MT_F32 || dtype == MT_F64 || dtype == MT_I32 || dtype == MT_I64, "bad action dtype");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_step_host before mt_reset / mt_reset_random");
  MT_ENTER(h);
  const size_t n = (size_t)h->n, es = (dtype == MT_F32 || dtype == MT_I32) ? 4 : 8;
  const size_t in_b = n * h->D * es, obs_b = n * 3 * h->K * 4, rew_b = n * 4, done_b = n;
  const size_t out_b = obs_b + rew_b + done_b, total = align_up(in_b, 256) + out_b;
  if (h->pinned_bytes < total) {
    if (h->pinned) {
      MT_HIP(h, hipStreamSynchronize(h->stream));
      (void)hipHostFree(h->pinned);
      h->pinned = nullptr;
      h->pinned_bytes = 0;
    }
    if (hipHostMalloc(&h->pinned, total, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, MT_ERR_ALLOC, "hipHostMalloc failed");
    }
    h->pinned_bytes = total;
  }
  int rc = ensure_staging(h, total);
  if (rc) return rc;
  char* hp = (char*)h->pinned;
  char* dp = (char*)h->staging;
  char* hp_out = hp + align_up(in_b, 256);
  char* dp_out = dp + align_up(in_b, 256);
  std::memcpy(hp, actions, in_b);
  MT_HIP(h, hipMemcpyAsync(dp, hp, in_b, hipMemcpyHostToDevice, h->stream));
  const dim3 g = grid_for(h->n), b(kBlock);
  switch (dtype) {
    case MT_F32: hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)dp, h->D, h->n, h->args.actions, h->ld); break;
    case MT_F64: hipLaunchKernelGGL((env_major_to_soa<double>), g, b, 0, h->stream, (const double*)dp, h->D, h->n, h->args.actions, h->ld); break;
    case MT_I32: hipLaunchKernelGGL((env_major_to_soa<int32_t>), g, b, 0, h->stream, (const int32_t*)dp, h->D, h->n, h->args.actions, h->ld); break;
    default: hipLaunchKernelGGL((env_major_to_soa<int64_t>), g, b, 0, h->stream, (const int64_t*)dp, h->D, h->n, h->args.actions, h->ld); break;
  }
  launch_step(h, false);
  h->args.flags &= ~kFlagWholeGoals;
  hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, h->args.obs, h->ld, 3 * h->K, h->n, (float*)dp_out);
  rc = check_launch(h, "mt_step_host");
  if (rc) return rc;
  MT_HIP(h, hipMemcpyAsync(dp_out + obs_b, h->args.reward, rew_b, hipMemcpyDeviceToDevice, h->stream));
  MT_HIP(h, hipMemcpyAsync(dp_out + obs_b + rew_b, h->args.done, done_b, hipMemcpyDeviceToDevice, h->stream));
  MT_HIP(h, hipMemcpyAsync(hp_out, dp_out, out_b, hipMemcpyDeviceToHost, h->stream));
  MT_HIP(h, hipStreamSynchronize(h->stream));  // the only host wait of the call
  std::memcpy(obs, hp_out, obs_b);
  std::memcpy(reward, hp_out + obs_b, rew_b);
  std::memcpy(done, hp_out + obs_b + rew_b, done_b);
  return MT_OK;
}

int mt_step_random(mt_handle h, uint64_t seed, uint32_t step_idx) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_step_random before mt_reset / mt_reset_random");
  MT_ENTER_KEEP(h);  // (launch_step keeps the record of MT_F_GOALS)
  h->args.seed_lo = (uint32_t)seed;
  h->args.seed_hi = (uint32_t)(seed >> 32);
  h->args.major = step_idx;
  launch_step(h, true);
  return check_launch(h, "step_kernel");
}

// ---- one env of the batch (multienv.environment[i].step / .reset, manytor.py:82,118) ----------------------------
static int rebuild_done_word(mt_handle h, int64_t env) {
  hipLaunchKernelGGL(done_bits_word_kernel, dim3(1), dim3(64), 0, h->stream, h->args.done, h->n, env >> 6,
                     h->args.done_bits);
  return check_launch(h, "done_bits_word_kernel");
}

int mt_env_step(mt_handle h, int64_t env, const float* action, float* obs, int32_t* reward, uint8_t* done) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, action && obs && reward && done, "NULL argument");
  MT_REQUIRE(h, env >= 0 && env < h->n, "env index out of range");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_env_step before mt_reset / mt_reset_random");
  MT_ENTER(h);
  const StepArgs a = args_for_env(h, env);
  const size_t pitch = (size_t)h->ld * 4;
  // column `env` of the D action rows <- D host floats
  MT_HIP(h, hipMemcpy2DAsync(a.actions, pitch, action, 4, 4, (size_t)h->D, hipMemcpyHostToDevice, h->stream));
  launch_step(h, mt_engine::kOneEnv, a, h->trace ? h->trace + env : nullptr, false);
  h->args.flags &= ~kFlagWholeGoals;
  int rc = check_launch(h, "step_kernel (one env)");
  if (rc) return rc;
  rc = rebuild_done_word(h, env);
  if (rc) return rc;
  MT_HIP(h, hipMemcpy2DAsync(obs, 4, a.obs, pitch, 4, (size_t)(3 * h->K), hipMemcpyDeviceToHost, h->stream));
  MT_HIP(h, hipMemcpyAsync(reward, a.reward, 4, hipMemcpyDeviceToHost, h->stream));
  MT_HIP(h, hipMemcpyAsync(done, a.done, 1, hipMemcpyDeviceToHost, h->stream));
  MT_HIP(h, hipStreamSynchronize(h->stream));
  return MT_OK;
}

int mt_env_reset(mt_handle h, int64_t env, const float* points, uint64_t seed, uint32_t episode) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, env >= 0 && env < h->n, "env index out of range");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_env_reset before the first reset of the batch");
  if (points && first_unusable(points, 3 * (int64_t)h->K, kMaxFiniteBits) >= 0)
    return fail(h, MT_ERR_INVALID_ARG, "mt_env_reset: a target coordinate is NaN or infinite");
  MT_ENTER(h);
  StepArgs a = args_for_env(h, env);
  if (points)  // (K, 3) host floats: flat index 3k + axis = row index
    MT_HIP(h, hipMemcpy2DAsync(a.points, (size_t)h->ld * 4, points, 4, 4, (size_t)(3 * h->K), hipMemcpyHostToDevice,
                               h->stream));
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.major = episode;
  {
    int rcg = order_behind_inplace_gather(h, h->stream);
    if (rcg) return rcg;
  }
  MT_DISPATCH_D(h->D, launch_reset_d, h, a, points ? 0 : 1);
  int rc = check_launch(h, "reset_kernel (one env)");
  if (rc) return rc;
  rc = rebuild_done_word(h, env);
  if (rc) return rc;
  MT_HIP(h, hipStreamSynchronize(h->stream));  // the caller may free `points` on return
  return MT_OK;
}

int mt_bad_action_count(mt_handle h, uint64_t* count) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, count != nullptr, "count is NULL");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  uint32_t c = 0;
  MT_HIP(h, hipMemcpyAsync(&c, h->args.bad_actions, 4, hipMemcpyDeviceToHost, h->stream));
  MT_HIP(h, hipStreamSynchronize(h->stream));
  *count = c;
  return MT_OK;
}

// mt_rollout on small batches is bound by the kernel boundary, not by the kernels (profiles/r02_variants.md section 3):
// the T launches of a segment are captured once into a HIP graph (stream capture of the very same launches; each node's
// step index = its offset + a device word) and replayed -- 5-15 % less per step up to 131 072 arms, nothing above.
static bool rollout_uses_graph(mt_handle h, int n_steps) {
  if (h->graph_mode == 0 || h->trace || n_steps < 4) return false;
  if (h->graph_mode < 0 && h->n > h->graph_max) return false;

  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(h->stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return false;  // the caller is capturing this stream into a graph of their own: plain launches
  }
  return true;
}

// The cached graph(s) of a T-step segment: one graph per chain (chain c's T launches), to be replayed on chain c's stream.
static int rollout_graph(mt_handle h, int T, uint64_t seed, int chains, const mt_engine::RolloutGraph** out) {
  // one word per chain: chain c's nodes read word c, which is rewritten on chain c's OWN stream right before its replay
  if (!h->graph_step0) MT_HIP(h, hipMalloc(&h->graph_step0, sizeof(uint32_t) * mt_engine::kMaxChains));
  StepArgs a = h->args;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.major = 0;
  a.episode0 = 0;  // not read by the step kernels
  a.major_base = h->graph_step0;
  for (auto& g : h->graphs)
    if (g.T == T && g.chains == chains && std::memcmp(&g.args, &a, sizeof a) == 0) {
      *out = &g;
      return MT_OK;
    }
  // captured on the handle's private stream whatever stream the handle currently launches on (the caller's may be the
  // null stream, which cannot capture); the instantiated graphs are launched on the current one / the chain streams
  mt_engine::RolloutGraph rg{};
  rg.T = T;
  rg.chains = chains;
  rg.args = a;
  hipStream_t launch_stream = h->stream;
  auto drop = [&]() {
    for (int c = 0; c < chains; ++c)
      if (rg.exec[c]) (void)hipGraphExecDestroy(rg.exec[c]);
  };
  for (int c = 0; c < chains; ++c) {
    if (c > 0 && (int64_t)c * chain_span(h, chains) >= h->n) break;
    hipGraph_t graph = nullptr;
    MT_HIP(h, hipStreamBeginCapture(h->own_stream, hipStreamCaptureModeThreadLocal));
    h->stream = h->own_stream;
    if (chains > 1) {
      StepArgs ac = a;
      ac.major_base = h->graph_step0 + c;
      launch_chain(h, ac, 0u, T, chains, c);
    } else {
      for (int s = 0; s < T; ++s) {
        StepArgs as = a;
        as.major = (uint32_t)s;
        launch_step(h, mt_engine::kBatch, as, nullptr, true);
      }
    }
    h->stream = launch_stream;
    hipError_t e = hipStreamEndCapture(h->own_stream, &graph);
    if (e != hipSuccess || !graph) {
      (void)hipGetLastError();
      drop();
      return fail(h, MT_ERR_HIP, std::string("mt_rollout: stream capture failed: ") + hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&rg.exec[c], graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) {
      rg.exec[c] = nullptr;
      drop();
      return fail(h, MT_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    }
  }
  if (h->graphs.size() >= 8) {  // a handful of segment lengths at most; drop the oldest beyond that
    // its per-chain graphs may still be executing on the chain streams (lazily forked chains): fold them back and drain
    // every stream a replay can be on before the executables go
    int rcj = join_chains(h);
    if (rcj) return rcj;
    MT_HIP(h, hipStreamSynchronize(h->stream));
    for (int c = 1; c < mt_engine::kMaxChains; ++c)
      if (h->chain_streams[c]) MT_HIP(h, hipStreamSynchronize(h->chain_streams[c]));
    for (hipGraphExec_t x : h->graphs.front().exec)
      if (x) (void)hipGraphExecDestroy(x);
    h->graphs.erase(h->graphs.begin());
  }
  h->graphs.push_back(rg);
  *out = &h->graphs.back();
  return MT_OK;
}

int mt_rollout(mt_handle h, int n_steps, uint64_t seed, uint32_t step_idx0) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, n_steps >= 0, "n_steps must be >= 0");
  if (n_steps > 0 && !h->is_reset) return fail(h, MT_ERR_STATE, "mt_rollout before mt_reset / mt_reset_random");
  if (n_steps == 0) return MT_OK;
  MT_ON_DEVICE(h, h->cfg.device);  // per-chain call: joins only where it has to (below)
  note_capture(h);
  // several independent chains of launches (env ranges on separate streams) where that pays; a caller who is capturing
  // the handle's stream gets the plain single-stream sequence
  // (a call that finds a deferred reset takes the form that absorbs it even for a single step)
  int chains = (n_steps >= 2 || h->reset_pending) ? usable_chains(h) : 1;
  h->snap_valid = false;  // the returns are about to change
  const bool multi = (n_steps >= 2 || h->reset_pending) && rollout_is_multi_step(h);
  const bool chained_fresh = h->reset_pending && !multi && chains > 1 && chained_rollout_absorbs_reset(h) && !rollout_uses_graph(h, n_steps);
  if (n_steps < 2 && !multi && !chained_fresh) chains = 1;
  if (h->reset_pending && !multi && !chained_fresh) {  // a deferred reset and a form that cannot absorb it: launch it now
    int rc = flush_pending_reset(h);
    if (rc) return rc;
  }
  // Small shards: k steps per launch through the rollout kernels (kPolicy.multi_step_*).  The call exposes the state after
  // n_steps steps and the outputs of the last one either way; every step still writes its outputs.  One chain (see
  // kPolicy) unless MT_CHAINS asks for more.  The episode boundary rides along: a deferred full reset becomes the prologue
  // of the first launch, and the last launch also stores the returns to the overlapped gather's snapshot row.
  if (multi) {
    if (!h->chains_forced) chains = 1;
    StepArgs a = h->args;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    const bool fresh = h->reset_pending;
    h->reset_pending = false;
    // the snapshot row of the next exchange (double-buffered: engine_internal.h) may be written once the exchange that last
    // read it is known to have finished: asked, never waited for (mt_gather_returns_begin keeps the host informed)
    bool snap = h->snap_in_rollout && h->snap != nullptr && snapshot_trusted(h);  // (own stream only: engine_internal.h)
    const int snap_p = h->snap_next;
    if (snap && !h->snap_free_known[snap_p]) {
      if (hipEventQuery(h->ev_gdone[snap_p]) == hipSuccess) {
        h->snap_free_known[snap_p] = true;
      } else {
        (void)hipGetLastError();
        snap = false;
      }
    }
    auto args_of = [&](int s0) {
      RolloutArgs r{std::min(h->multi_k, n_steps - s0), step_idx0 + (uint32_t)s0, 0u, h->cfg.radius, 0u, 0u, 0u, 0u, nullptr};
      if (fresh && s0 == 0) {
        r.reset_first = 1u;
        r.reset_episode = h->pend_episode;
        r.reset_seed_lo = (uint32_t)h->pend_seed;
        r.reset_seed_hi = (uint32_t)(h->pend_seed >> 32);
      }
      if (snap && s0 + h->multi_k >= n_steps) r.snap = h->snap_row(snap_p);
      return r;
    };
    int rc = MT_OK;
    if (fresh) {  // the in-kernel reset writes MT_F_LAST_RETURN: behind an exchange that still reads that row in place
      rc = order_behind_inplace_gather(h, h->stream);
      if (rc) return rc;
    }
    if (chains > 1) {
      rc = fork_chains(h, chains);
      if (rc) return rc;
      const int64_t span = chain_span(h, chains);
      hipStream_t root = h->stream;
      for (int s0 = 0; s0 < n_steps; s0 += h->multi_k) {
        for (int c = 0; c < chains; ++c) {
          const int64_t off = (int64_t)c * span;
          if (off >= h->n) continue;
          h->stream = c == 0 ? root : h->chain_streams[c];
          RolloutArgs r = args_of(s0);
          if (r.snap) r.snap += off;
          if (fresh && s0 == 0 && c > 0 && rc == MT_OK) rc = order_behind_inplace_gather(h, h->stream);
          if (rc == MT_OK) launch_rollout(h, args_for_range(h, a, off, std::min(span, h->n - off)), h->sched[mt_engine::kChain].rollout_lanes, r, h->rollout_early);
        }
      }
      h->stream = root;
      if (rc == MT_OK) rc = check_launch(h, "rollout_kernel (mt_rollout, per chain)");
      if (rc) return rc;
      rc = settle_chains(h);
    } else {
      rc = join_chains(h);
      if (rc) return rc;
      for (int s0 = 0; s0 < n_steps; s0 += h->multi_k) launch_rollout(h, a, h->sched[mt_engine::kBatch].rollout_lanes, args_of(s0), h->rollout_early);
      rc = check_launch(h, "rollout_kernel (mt_rollout)");
    }
    if (rc) return rc;
    h->snap_valid = snap;
    h->args.seed_lo = (uint32_t)seed;
    h->args.seed_hi = (uint32_t)(seed >> 32);
    h->args.major = step_idx0 + (uint32_t)(n_steps - 1);
    return MT_OK;
  }
  bool graph = rollout_uses_graph(h, n_steps);
  if (graph && h->graph_mode < 0) {
    // capture + instantiation cost about a dozen plain segments: only for a segment length that comes back
    bool cached = false, seen = false;
    for (auto& g : h->graphs) cached |= g.T == n_steps;
    for (int t : h->graph_seen) seen |= t == n_steps;
    if (!cached && !seen) {
      if (h->graph_seen.size() >= 32) h->graph_seen.erase(h->graph_seen.begin());
      h->graph_seen.push_back(n_steps);
      graph = false;
    }
  }
  if (chains == 1) {  // single-stream forms: the chains (if a per-chain reset left them forked) come back first
    int rc = join_chains(h);
    if (rc) return rc;
  }
  if (graph) {
    const mt_engine::RolloutGraph* rg = nullptr;
    h->codes_valid = false;  // captured launches are replayed whatever the codes' state: the float kernels
    h->forget_goals();       // ... and whatever the pose row's: they load it, and leave no record
    int rc = rollout_graph(h, n_steps, seed, chains, &rg);
    if (rc) return rc;
    if (chains > 1) {
      rc = fork_chains(h, chains);
      if (rc) return rc;
      const int64_t span = chain_span(h, chains);
      for (int c = 0; c < chains; ++c) {
        if ((int64_t)c * span >= h->n) continue;
        // chain c's step-index word is set on chain c's stream, behind its previous replay and ahead of this one
        MT_HIP(h, hipMemsetD32Async((hipDeviceptr_t)(h->graph_step0 + c), (int)step_idx0, 1, chain_stream(h, c)));
        MT_HIP(h, hipGraphLaunch(rg->exec[c], chain_stream(h, c)));
      }
      rc = settle_chains(h);
      if (rc) return rc;
    } else {
      MT_HIP(h, hipMemsetD32Async((hipDeviceptr_t)h->graph_step0, (int)step_idx0, 1, h->stream));
      MT_HIP(h, hipGraphLaunch(rg->exec[0], h->stream));
    }
  } else if (chains > 1) {
    StepArgs a = h->args;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    int rc = fork_chains(h, chains);  // no-op when a per-chain reset (or the previous segment) left them forked
    if (rc) return rc;
    // chains enqueued round-robin step by step, so that no stream runs dry while the host is busy with another one
    hipStream_t root = h->stream;
    const int64_t span = chain_span(h, chains);
    h->reset_pending = false;
    // the last step launch of every chain also stores its returns to the overlapped gather's next snapshot row (double-
    // buffered: engine_internal.h), once the exchange that last read that row is known to have finished
    StepArgs a_last = a;
    {
      const int sp = h->snap_next;
      bool snap = h->snap_in_rollout && h->snap != nullptr && !h->trace && snapshot_trusted(h);
      if (snap && !h->snap_free_known[sp]) {
        if (hipEventQuery(h->ev_gdone[sp]) == hipSuccess) {
          h->snap_free_known[sp] = true;
        } else {
          (void)hipGetLastError();
          snap = false;
        }
      }
      if (snap) a_last.snap = h->snap_row(sp);
    }
    bool fresh_by_rollout_kernel = false;
    for (int st = 0; st < n_steps; ++st)
      for (int c = 0; c < chains; ++c) {
        h->stream = c == 0 ? root : h->chain_streams[c];
        const int64_t off = (int64_t)c * span;
        if (chained_fresh && st == 0 && off < h->n) {
          // the episode's first step carries the deferred reset as its prologue (the state of reset_kernel + step_kernel, bit
          // for bit: no reset launch, no stores of what the step overwrites, no re-fetch of what the reset would have
          // written): the step kernel's own FRESH form where the schedule has one, else ONE step of the rollout kernel
          if (rc == MT_OK) rc = order_behind_inplace_gather(h, h->stream);  // (the in-kernel reset writes MT_F_LAST_RETURN)
          if (rc != MT_OK) continue;
          StepArgs af = (n_steps == 1) ? a_last : a;
          af.reset_seed_lo = (uint32_t)h->pend_seed;
          af.reset_seed_hi = (uint32_t)(h->pend_seed >> 32);
          af.reset_episode = h->pend_episode;
          af.radius = h->cfg.radius;
          if (launch_chain_fresh(h, af, step_idx0, chains, c)) continue;
          fresh_by_rollout_kernel = true;
          const RolloutArgs r{1, step_idx0, 0u, h->cfg.radius, 1u, h->pend_episode, (uint32_t)h->pend_seed, (uint32_t)(h->pend_seed >> 32), nullptr};
          launch_rollout(h, args_for_range(h, a, off, std::min(span, h->n - off)), 1, r, h->rollout_early);
          continue;
        }
        if (rc == MT_OK) launch_chain(h, st == n_steps - 1 ? a_last : a, step_idx0 + (uint32_t)st, 1, chains, c);
      }
    h->stream = root;
    if (rc == MT_OK) rc = check_launch(h, "step_kernel (chained)");
    if (rc) return rc;
    rc = settle_chains(h);
    if (rc) return rc;
    h->snap_valid = a_last.snap != nullptr && !(fresh_by_rollout_kernel && n_steps == 1);
  } else {
    for (int s = 0; s < n_steps; ++s) {
      int rc = mt_step_random(h, seed, step_idx0 + (uint32_t)s);
      if (rc) return rc;
    }
    return MT_OK;
  }
  h->args.seed_lo = (uint32_t)seed;
  h->args.seed_hi = (uint32_t)(seed >> 32);
  h->args.major = step_idx0 + (uint32_t)(n_steps - 1);
  return MT_OK;
}

int mt_rollout_fused(mt_handle h, int n_steps, uint64_t seed, uint32_t step_idx0, int auto_reset) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, n_steps >= 0, "n_steps must be >= 0");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_rollout_fused before mt_reset / mt_reset_random");
  if (n_steps == 0) return MT_OK;
  // The fused kernel implements the default trigonometry only; the measured alternatives run the same thing as a
  // sequence of launches.
  if (!fusable(h)) {
    for (int s = 0; s < n_steps; ++s) {
      int rc = mt_step_random(h, seed, step_idx0 + (uint32_t)s);
      if (rc) return rc;
      if (auto_reset) {
        rc = mt_reset_done(h, seed);
        if (rc) return rc;
      }
    }
    return MT_OK;
  }
  MT_ENTER(h);
  h->args.seed_lo = (uint32_t)seed;
  h->args.seed_hi = (uint32_t)(seed >> 32);
  if (auto_reset) {  // the in-kernel re-arm writes MT_F_LAST_RETURN
    int rcg = order_behind_inplace_gather(h, h->stream);
    if (rcg) return rcg;
  }
  RolloutArgs r{n_steps, step_idx0, auto_reset ? 1u : 0u, h->cfg.radius, 0u, 0u, 0u, 0u, nullptr};
  launch_rollout(h, h->args, h->sched[mt_engine::kBatch].rollout_lanes, r);
  return check_launch(h, "rollout_kernel");
}

int mt_rollout_tape(mt_handle h, const mt_tape* tape) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, tape != nullptr, "tape is NULL");
  MT_REQUIRE(h, tape->struct_size == (int32_t)sizeof(mt_tape), "mt_tape.struct_size does not match this library");
  MT_REQUIRE(h, tape->reserved == 0, "mt_tape.reserved must be 0");
  MT_REQUIRE(h, (tape->flags & ~(MT_TAPE_AUTO_RESET | MT_TAPE_DRY_RUN)) == 0, "unknown MT_TAPE_* flag");
  const bool auto_reset = (tape->flags & MT_TAPE_AUTO_RESET) != 0, dry = (tape->flags & MT_TAPE_DRY_RUN) != 0;
  MT_REQUIRE(h, !(auto_reset && dry), "MT_TAPE_DRY_RUN | MT_TAPE_AUTO_RESET: the re-arm writes the return ring");
  MT_REQUIRE(h, tape->n_steps >= 0, "n_steps must be >= 0");
  if (!fusable(h)) return fail_unfusable(h, "mt_rollout_tape");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_rollout_tape before mt_reset / mt_reset_random");
  if (tape->n_steps == 0) return MT_OK;
  MT_REQUIRE(h, tape->actions != nullptr, "mt_tape.actions is NULL");
  MT_REQUIRE(h, tape->ld >= h->n, "mt_tape.ld is smaller than n_envs");
  MT_REQUIRE(h, !(tape->reward_log || tape->done_log) || tape->log_ld >= h->n, "mt_tape.log_ld is smaller than n_envs");
  MT_ENTER(h);
  TapeArgs r = tape_args(tape, tape->actions, tape->ld, tape->n_steps);
  r.dry_run = dry ? 1u : 0u;
  r.nt_loads = h->tape_nt_loads ? 1u : 0u;
  return commit_tape(h, r, tape->seed, auto_reset, false);
}

// mt_rollout_policy, and mt_rollout_population with member 0's rows as the weights, in two halves: everything the host can
// refuse (`nm` is the struct the messages name, `who` the entry point), which launches nothing and changes nothing, and
// the launch.  A call with n_steps == 0 passes the screen and is the caller's no-op.
struct PolicyScreen {
  int widest = 0;
  bool noisy = false;
};
static int rollout_policy_screen(mt_handle h, const struct mt_policy* p, const std::string& nm, const char* who, PolicyScreen* out) {
  MT_REQUIRE(h, (p->flags & ~(MT_POLICY_AUTO_RESET | MT_POLICY_DRY_RUN | MT_POLICY_SEE_POSE)) == 0, nm + ".flags: unknown MT_POLICY_* flag");
  const bool auto_reset = (p->flags & MT_POLICY_AUTO_RESET) != 0, dry = (p->flags & MT_POLICY_DRY_RUN) != 0;
  MT_REQUIRE(h, !(auto_reset && dry), nm + ".flags: MT_POLICY_DRY_RUN | MT_POLICY_AUTO_RESET: the re-arm writes the return ring");
  MT_REQUIRE(h, p->n_steps >= 0 && p->n_steps <= 65535, nm + ".n_steps must be 0..65535");
  const int L = p->n_layers;
  MT_REQUIRE(h, L >= 1 && L <= MT_POLICY_MAX_LAYERS, nm + ".n_layers must be 1.." + std::to_string(MT_POLICY_MAX_LAYERS));
  int widest = 0;
  for (int l = 0; l + 1 < L; ++l) {
    MT_REQUIRE(h, p->width[l] >= 1 && p->width[l] <= MT_POLICY_MAX_WIDTH,
               nm + ".width[" + std::to_string(l) + "] must be 1.." + std::to_string(MT_POLICY_MAX_WIDTH));
    widest = std::max(widest, (int)p->width[l]);
  }
  MT_REQUIRE(h, L == 1 || p->hidden_act == MT_ACT_TANH || p->hidden_act == MT_ACT_RELU, nm + ".hidden_act must be MT_ACT_TANH or MT_ACT_RELU");
  MT_REQUIRE(h, p->out_act == MT_ACT_TANH || p->out_act == MT_ACT_IDENTITY, nm + ".out_act must be MT_ACT_TANH or MT_ACT_IDENTITY");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&p->lo, 1, kMaxAngleBits) < 0 && first_unusable(&p->hi, 1, kMaxAngleBits) < 0,
             nm + ".lo / hi must be finite and within +-32768 degrees");
  MT_REQUIRE(h, p->lo <= p->hi, nm + ".lo must be <= hi");
  MT_REQUIRE(h, first_unusable(&p->out_scale, 1, kMaxFiniteBits) < 0, nm + ".out_scale must be finite");
  bool noisy = false;
  for (int j = 0; j < MT_MAX_DOF; ++j) {
    MT_REQUIRE(h, first_unusable(&p->sigma[j], 1, kMaxFiniteBits) < 0 && p->sigma[j] >= 0.f,
               nm + ".sigma[" + std::to_string(j) + "] must be finite and >= 0");
    noisy |= j < h->D && p->sigma[j] > 0.f;
  }
  if (!fusable(h)) return fail_unfusable(h, who);
  if (!h->is_reset) return fail(h, MT_ERR_STATE, std::string(who) + " before mt_reset / mt_reset_random");
  if (p->n_steps == 0) return MT_OK;
  for (int l = 0; l < L; ++l)
    MT_REQUIRE(h, p->weight[l] != nullptr && p->bias[l] != nullptr, nm + ".weight / bias [" + std::to_string(l) + "] is NULL");
  MT_REQUIRE(h, !p->action_log || p->act_ld >= h->n, nm + ".act_ld is smaller than n_envs");
  MT_REQUIRE(h, !p->obs_log || p->obs_ld >= h->n, nm + ".obs_ld is smaller than n_envs");
  MT_REQUIRE(h, !(p->reward_log || p->done_log) || p->log_ld >= h->n, nm + ".log_ld is smaller than n_envs");
  out->widest = widest;
  out->noisy = noisy;
  return MT_OK;
}
// ... the launch (the caller has entered the handle: MT_ENTER): block b reads the weights of member b / blocks_per_member,
// member_pitch floats behind member 0's
// `ac` (mt_rollout_actor_critic): what the launch writes besides, its PolicyArgs part filled in here; `ac_widest` the
// critic's widest hidden layer
static int rollout_policy_run(mt_handle h, const struct mt_policy* p, const PolicyScreen& sc, uint32_t blocks_per_member, int64_t member_pitch,
                              ActorCriticArgs* ac = nullptr, int ac_widest = 0) {
  const bool auto_reset = (p->flags & MT_POLICY_AUTO_RESET) != 0, dry = (p->flags & MT_POLICY_DRY_RUN) != 0;
  const int L = p->n_layers, widest = sc.widest;
  const bool noisy = sc.noisy;
  PolicyArgs r{};
  const bool see_pose = (p->flags & MT_POLICY_SEE_POSE) != 0;
  int n_in = 3 * h->K + (see_pose ? h->D : 0);
  for (int l = 0; l < L; ++l) {
    r.w[l] = p->weight[l];
    r.b[l] = p->bias[l];
    r.n_in[l] = n_in;
    r.n_out[l] = n_in = (l + 1 < L) ? p->width[l] : h->D;
  }
  r.L = L;
  r.T = p->n_steps;
  r.hidden_act = p->hidden_act;
  r.out_act = p->out_act;
  r.out_scale = p->out_scale;
  r.lo = p->lo;
  r.hi = p->hi;
  std::memcpy(r.sigma, p->sigma, sizeof(r.sigma));
  r.draw = p->draw;
  r.noisy = noisy ? 1u : 0u;
  r.see_pose = see_pose ? 1u : 0u;
  r.action_log = p->action_log;
  r.act_ld = p->act_ld;
  r.obs_log = p->obs_log;
  r.obs_ld = p->obs_ld;
  r.reward_log = p->reward_log;
  r.done_log = p->done_log;
  r.log_ld = p->log_ld;
  r.return_out = p->return_out;
  r.auto_reset = auto_reset ? 1u : 0u;
  r.dry_run = dry ? 1u : 0u;
  r.seed_lo = (uint32_t)p->seed;
  r.seed_hi = (uint32_t)(p->seed >> 32);
  r.radius = h->cfg.radius;
  r.blocks_per_member = blocks_per_member;
  r.member_pitch = member_pitch;
  if (auto_reset) {  // what commit_tape does ahead of a re-arming launch
    h->args.seed_lo = (uint32_t)p->seed;
    h->args.seed_hi = (uint32_t)(p->seed >> 32);
    int rcg = order_behind_inplace_gather(h, h->stream);
    if (rcg) return rcg;
  }
  if (ac) {
    static_cast<PolicyArgs&>(*ac) = r;
    launch_actor_critic(h, h->args, *ac, std::max(widest, ac_widest));
  } else {
    launch_policy(h, h->args, r, widest);
  }
  if (!dry) {
    h->args.flags &= ~kFlagWholeGoals;  // a policy's angles are anybody's floats
    h->codes_valid = false;             // the kernel writes targets as floats only
  }
  return check_launch(h, "rollout_policy_kernel");
}

int mt_rollout_policy(mt_handle h, const struct mt_policy* p) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, p != nullptr, "policy is NULL");
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_policy), "mt_policy.struct_size does not match this library");
  MT_REQUIRE(h, p->reserved == 0, "mt_policy.reserved must be 0");
  PolicyScreen sc;
  int rc = rollout_policy_screen(h, p, "mt_policy", "mt_rollout_policy", &sc);
  if (rc || p->n_steps == 0) return rc;
  MT_ENTER(h);
  return rollout_policy_run(h, p, sc, 1u, 0);
}

// ---- mt_es_sample, mt_rollout_population, mt_es ------------------------------------------------------------------------
// The population's shape against the handle's: M even, G = n / M a multiple of the rollout block.
static int population_shape(mt_handle h, int32_t M, const std::string& nm, int64_t* G) {
  MT_REQUIRE(h, M >= 2 && M <= MT_ES_MAX_MEMBERS && M % 2 == 0,
             nm + ".n_members must be even (antithetic pairs), 2.." + std::to_string(MT_ES_MAX_MEMBERS));
  MT_REQUIRE(h, h->n % M == 0, nm + ".n_members must divide n_envs: member m owns the G = n_envs / n_members envs [mG, (m+1)G)");
  *G = h->n / M;
  MT_REQUIRE(h, *G % kBlock == 0, nm + ": G = n_envs / n_members must be a multiple of " + std::to_string(kBlock) +
                                      ", the rollout block: a block reads one member's weights");
  return MT_OK;
}
// struct mt_population as the struct mt_policy of its member 0 (`q`), with the shape rules and P, the length of theta
static int population_policy(mt_handle h, const struct mt_population* p, const std::string& nm, struct mt_policy* q, int64_t* P, int64_t* G) {
  int rc = population_shape(h, p->n_members, nm, G);
  if (rc) return rc;
  const int L = p->n_layers;
  MT_REQUIRE(h, L >= 1 && L <= MT_POLICY_MAX_LAYERS, nm + ".n_layers must be 1.." + std::to_string(MT_POLICY_MAX_LAYERS));
  for (int l = 0; l + 1 < L; ++l)
    MT_REQUIRE(h, p->width[l] >= 1 && p->width[l] <= MT_POLICY_MAX_WIDTH,
               nm + ".width[" + std::to_string(l) + "] must be 1.." + std::to_string(MT_POLICY_MAX_WIDTH));
  MT_REQUIRE(h, (p->flags & ~(MT_POLICY_AUTO_RESET | MT_POLICY_DRY_RUN | MT_POLICY_SEE_POSE)) == 0, nm + ".flags: unknown MT_POLICY_* flag");
  *q = mt_policy{};
  int64_t off = 0;
  int n_in = 3 * h->K + ((p->flags & MT_POLICY_SEE_POSE) ? h->D : 0);
  for (int l = 0; l < L; ++l) {  // W_l (out, in) | b_l (out,)
    const int n_out = (l + 1 < L) ? p->width[l] : h->D;
    q->weight[l] = p->pop ? p->pop + off : nullptr;
    off += (int64_t)n_out * n_in;
    q->bias[l] = p->pop ? p->pop + off : nullptr;
    off += n_out;
    n_in = n_out;
  }
  *P = off;
  MT_REQUIRE(h, p->pitch >= off, nm + ".pitch is smaller than P = " + std::to_string(off) + ", the policy's parameter count");
  MT_REQUIRE(h, !p->fitness_out || p->return_out, nm + ".fitness_out needs return_out");
  q->struct_size = (int32_t)sizeof(struct mt_policy);
  q->n_steps = p->n_steps;
  q->n_layers = L;
  q->width[0] = p->width[0];
  q->width[1] = p->width[1];
  q->hidden_act = p->hidden_act;
  q->out_act = p->out_act;
  q->out_scale = p->out_scale;
  q->lo = p->lo;
  q->hi = p->hi;
  q->flags = p->flags;
  q->action_log = p->action_log;
  q->act_ld = p->act_ld;
  q->obs_log = p->obs_log;
  q->obs_ld = p->obs_ld;
  q->reward_log = p->reward_log;
  q->done_log = p->done_log;
  q->log_ld = p->log_ld;
  q->return_out = p->return_out;
  q->seed = p->seed;
  return MT_OK;
}
static float inv_members_envs(int64_t G) { return (float)(1.0 / (double)G); }  // the fp32 nearest to 1 / G
static bool floats_overlap(const float* p, int64_t np, const float* q, int64_t nq) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + (uintptr_t)np * 4, b0 = (uintptr_t)q, b1 = b0 + (uintptr_t)nq * 4;
  return p && q && a0 < b1 && b0 < a1;
}
static void launch_es_sums(mt_handle h, const EsArgs& e) {  // a block per member
  hipLaunchKernelGGL(es_sums_kernel, dim3((unsigned)e.M), dim3(kBlock), 0, h->stream, e);
}
static_assert(MT_ES_MAX_MEMBERS == kEsMaxMembers, "the header's member limit is what es_update_kernel's LDS holds");

int mt_es_sample(mt_handle h, const struct mt_es_sample* s) {
  MT_REQUIRE(h, s != nullptr, "es_sample is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_es_sample), "mt_es_sample.struct_size does not match this library");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s->reserved == 0, "mt_es_sample.reserved must be 0");
  const int M = s->n_members;
  MT_REQUIRE(h, M >= 2 && M <= MT_ES_MAX_MEMBERS && M % 2 == 0,
             "mt_es_sample.n_members must be even (antithetic pairs), 2.." + std::to_string(MT_ES_MAX_MEMBERS));
  MT_REQUIRE(h, s->n_params >= 1 && s->n_params <= ((int64_t)1 << 31), "mt_es_sample.n_params must be 1..2^31");
  MT_REQUIRE(h, s->pitch >= s->n_params, "mt_es_sample.pitch is smaller than n_params");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&s->sigma, 1, kMaxFiniteBits) < 0 && s->sigma > 0.f, "mt_es_sample.sigma must be finite and > 0");
  MT_REQUIRE(h, s->theta != nullptr && s->pop != nullptr, "mt_es_sample.theta / pop is NULL");
  MT_REQUIRE(h, !floats_overlap(s->theta, s->n_params, s->pop, (int64_t)(M - 1) * s->pitch + s->n_params), "mt_es_sample.pop overlaps theta");
  MT_ENTER(h);
  EsArgs e{};
  e.theta = const_cast<float*>(s->theta);  // (read only by this kernel)
  e.pop = s->pop;
  e.P = s->n_params;
  e.pitch = s->pitch;
  e.M = M;
  e.sigma = s->sigma;
  e.draw = s->draw;
  e.seed_lo = (uint32_t)s->seed;
  e.seed_hi = (uint32_t)(s->seed >> 32);
  hipLaunchKernelGGL(es_sample_kernel, dim3(grid_for(e.P).x, (unsigned)(M / 2)), dim3(kBlock), 0, h->stream, e);
  return check_launch(h, "es_sample_kernel");
}

int mt_rollout_population(mt_handle h, const struct mt_population* p) {
  MT_REQUIRE(h, p != nullptr, "population is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_population), "mt_population.struct_size does not match this library");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, p->reserved == 0, "mt_population.reserved must be 0");
  struct mt_policy q;
  int64_t P = 0, G = 0;
  int rc = population_policy(h, p, "mt_population", &q, &P, &G);
  if (rc) return rc;
  PolicyScreen sc;
  rc = rollout_policy_screen(h, &q, "mt_population", "mt_rollout_population", &sc);
  if (rc || p->n_steps == 0) return rc;
  MT_ENTER(h);
  rc = rollout_policy_run(h, &q, sc, (uint32_t)(G / kBlock), p->pitch);
  if (rc || !p->fitness_out) return rc;
  EsArgs e{};
  e.M = p->n_members;
  e.returns = p->return_out;
  e.G = G;
  e.inv_g = inv_members_envs(G);
  e.fitness = p->fitness_out;
  launch_es_sums(h, e);
  return check_launch(h, "es_sums_kernel");
}

int mt_es(mt_handle h, const struct mt_es* s) {
  MT_REQUIRE(h, s != nullptr, "es is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_es), "mt_es.struct_size does not match this library");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s->reserved == 0, "mt_es.reserved must be 0");
  MT_REQUIRE(h, s->pop.struct_size == (int32_t)sizeof(struct mt_population), "mt_es.pop.struct_size does not match this library");
  MT_REQUIRE(h, s->pop.reserved == 0, "mt_es.pop.reserved must be 0");
  MT_REQUIRE(h, (s->flags & ~(MT_ES_INPLACE | MT_ES_UPDATE_ONLY)) == 0, "mt_es.flags: unknown MT_ES_* flag");
  MT_REQUIRE(h, s->shaping == MT_ES_SHAPE_RANK || s->shaping == MT_ES_SHAPE_RAW, "mt_es.shaping must be MT_ES_SHAPE_RANK or MT_ES_SHAPE_RAW");
  const bool inplace = (s->flags & MT_ES_INPLACE) != 0, update_only = (s->flags & MT_ES_UPDATE_ONLY) != 0;
  const bool raw = s->shaping == MT_ES_SHAPE_RAW;
  MT_REQUIRE(h, first_unusable(&s->sigma, 1, kMaxFiniteBits) < 0 && s->sigma > 0.f, "mt_es.sigma must be finite and > 0");
  MT_REQUIRE(h, !inplace || first_unusable(&s->lr, 1, kMaxFiniteBits) < 0, "mt_es.lr must be finite");
  struct mt_policy q;
  int64_t P = 0, G = 0;
  int rc = population_policy(h, &s->pop, "mt_es.pop", &q, &P, &G);
  if (rc) return rc;
  PolicyScreen sc;
  rc = rollout_policy_screen(h, &q, "mt_es.pop", "mt_es", &sc);
  if (rc || s->pop.n_steps == 0) return rc;
  const int M = s->pop.n_members, T = s->pop.n_steps;
  MT_REQUIRE(h, s->theta != nullptr && s->grad_out != nullptr && s->coeff_out != nullptr, "mt_es.theta / grad_out / coeff_out is NULL");
  MT_REQUIRE(h, s->pop.return_out != nullptr, "mt_es.pop.return_out is NULL: the update reads the return row");
  const int64_t pop_floats = (int64_t)(M - 1) * s->pop.pitch + P;
  MT_REQUIRE(h, !floats_overlap(s->theta, P, s->grad_out, P), "mt_es.grad_out overlaps theta");
  MT_REQUIRE(h, !floats_overlap(s->theta, P, s->pop.pop, pop_floats) && !floats_overlap(s->grad_out, P, s->pop.pop, pop_floats),
             "mt_es.pop.pop overlaps theta / grad_out");
  // |coeff| <= 2 c_max, |bytesum - 510| <= 510, M / 2 pairs: A_i stays within int64
  const double c_max = raw ? (double)G * 127.0 * (double)T : 2.0 * (double)(M - 1);
  MT_REQUIRE(h, (double)M * c_max * 510.0 < 4.0e18, "mt_es: n_members * G * n_steps is too large for the update's int64 sums");
  MT_ENTER(h);
  EsArgs e{};
  e.theta = s->theta;
  e.pop = const_cast<float*>(s->pop.pop);
  e.P = P;
  e.pitch = s->pop.pitch;
  e.M = M;
  e.sigma = s->sigma;
  e.draw = s->draw;
  e.seed_lo = (uint32_t)s->pop.seed;
  e.seed_hi = (uint32_t)(s->pop.seed >> 32);
  e.returns = s->pop.return_out;
  e.G = G;
  e.inv_g = inv_members_envs(G);
  // the fp32 nearest to KZ / (M sigma 2 (M - 1)) or KZ / (M sigma G), in double from the fp32 KZ and the fp32 sigma
  e.scale = (float)((double)kPlanNoiseScale / ((double)M * (double)s->sigma * (raw ? (double)G : 2.0 * (double)(M - 1))));
  e.lr = s->lr;
  e.raw = raw ? 1u : 0u;
  e.inplace = inplace ? 1u : 0u;
  e.coeff = reinterpret_cast<long long*>(s->coeff_out);
  e.sums = e.coeff + M / 2;
  e.fitness = s->pop.fitness_out;
  e.best = s->best_out;
  e.grad = s->grad_out;
  if (!update_only) {
    hipLaunchKernelGGL(es_sample_kernel, dim3(grid_for(P).x, (unsigned)(M / 2)), dim3(kBlock), 0, h->stream, e);
    rc = check_launch(h, "es_sample_kernel");
    if (rc) return rc;
    rc = rollout_policy_run(h, &q, sc, (uint32_t)(G / kBlock), s->pop.pitch);
    if (rc) return rc;
  }
  launch_es_sums(h, e);
  rc = check_launch(h, "es_sums_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(es_update_kernel, grid_for(P), dim3(kBlock), (size_t)(M + M / 2) * sizeof(long long), h->stream, e);
  return check_launch(h, "es_update_kernel");
}

// ---- mt_policy_grad, mt_reward_to_go, mt_policy_eval, mt_gae, mt_value_grad ----------------------------------------------
// The shape of a policy on this handle: per-layer fan-in / fan-out, the layers' offsets in the flat vector, and P.
// n_last: the outputs of the last layer, 0 = the handle's D (a value head has 1).
struct PolicyLayout {
  int32_t n_in[3], n_out[3];
  int64_t off[3], P;
  int widest;
};
static bool policy_layout(const mt_engine* h, int L, const int32_t width[2], uint32_t flags, PolicyLayout* s, int n_last = 0) {
  if (L < 1 || L > MT_POLICY_MAX_LAYERS || (flags & ~(uint32_t)MT_POLICY_SEE_POSE)) return false;
  int n_in = 3 * h->K + ((flags & MT_POLICY_SEE_POSE) ? h->D : 0);
  s->P = 0;
  s->widest = 0;
  for (int l = 0; l < L; ++l) {
    if (l + 1 < L && (width[l] < 1 || width[l] > MT_POLICY_MAX_WIDTH)) return false;
    const int n_out = (l + 1 < L) ? width[l] : n_last ? n_last : h->D;
    if (l + 1 < L) s->widest = std::max(s->widest, n_out);
    s->n_in[l] = n_in;
    s->n_out[l] = n_out;
    s->off[l] = s->P;
    s->P += (int64_t)n_out * n_in + n_out;
    n_in = n_out;
  }
  return true;
}
// policy_grad_kernel's grid: a block per tile of kBlock envs of one step, at most two blocks per compute unit
static int64_t policy_grad_blocks(mt_handle h, int T) {
  if (h->cu_count <= 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;
    }
    h->cu_count = cus;
  }
  const int64_t tiles = (int64_t)T * ((h->n + kBlock - 1) / kBlock);
  return std::min<int64_t>(tiles, 2 * (int64_t)h->cu_count);
}
static size_t policy_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps, int n_last) {
  PolicyLayout s;
  const int32_t none[2] = {0, 0};
  if (!h || n_steps <= 0 || n_steps > 65535 || !policy_layout(h, n_layers, width ? width : none, flags, &s, n_last)) return 0;
  return (size_t)policy_grad_blocks(h, n_steps) * (size_t)(s.P + 1) * sizeof(float);
}
size_t mt_policy_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps) {
  return policy_grad_workspace(h, n_layers, width, flags, n_steps, 0);
}
static bool bytes_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a0 = (uintptr_t)p, a1 = a0 + np, b0 = (uintptr_t)q, b1 = b0 + nq;
  return p && q && np && nq && a0 < b1 && b0 < a1;
}

// What mt_policy_grad, mt_value_grad and mt_policy_eval state about the network alike (`w` is the struct the messages name).
struct PolicyNet {
  int32_t n_steps, n_layers;
  const int32_t* width;
  int32_t hidden_act, out_act;
  const float* const* weight;
  const float* const* bias;
  float out_scale;
  uint32_t flags;
  const float* obs;
  int64_t obs_ld;
  uint64_t reserved;
};
// (the three structs name these fields alike; a macro, as this is an extern "C" block)
#define MT_POLICY_NET(p)                                                                                                   \
  PolicyNet {                                                                                                              \
    (p)->n_steps, (p)->n_layers, (p)->width, (p)->hidden_act, (p)->out_act, (p)->weight, (p)->bias, (p)->out_scale, (p)->flags, \
        (p)->obs, (p)->obs_ld, (p)->reserved                                                                               \
  }
// ... the scalars of it, which need no handle
static int policy_net_screen(mt_handle h, const PolicyNet& p, const std::string& w) {
  MT_REQUIRE(h, p.reserved == 0, w + ".reserved must be 0");
  MT_REQUIRE(h, (p.flags & ~(uint32_t)MT_POLICY_SEE_POSE) == 0, w + ".flags: only MT_POLICY_SEE_POSE is read");
  MT_REQUIRE(h, p.n_steps >= 0 && p.n_steps <= 65535, w + ".n_steps must be 0..65535");
  const int L = p.n_layers;
  MT_REQUIRE(h, L >= 1 && L <= MT_POLICY_MAX_LAYERS, w + ".n_layers must be 1.." + std::to_string(MT_POLICY_MAX_LAYERS));
  for (int l = 0; l + 1 < L; ++l)
    MT_REQUIRE(h, p.width[l] >= 1 && p.width[l] <= MT_POLICY_MAX_WIDTH,
               w + ".width[" + std::to_string(l) + "] must be 1.." + std::to_string(MT_POLICY_MAX_WIDTH));
  MT_REQUIRE(h, L == 1 || p.hidden_act == MT_ACT_TANH || p.hidden_act == MT_ACT_RELU, w + ".hidden_act must be MT_ACT_TANH or MT_ACT_RELU");
  MT_REQUIRE(h, p.out_act == MT_ACT_TANH || p.out_act == MT_ACT_IDENTITY, w + ".out_act must be MT_ACT_TANH or MT_ACT_IDENTITY");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&p.out_scale, 1, kMaxFiniteBits) < 0, w + ".out_scale must be finite");
  return MT_OK;
}
// ... sigma ahead of the handle: entries whose use depends on the handle's D may still be 0 (`n_known` of them are known
// to be read: every handle has at least one joint)
static int policy_sigma_screen(mt_handle h, const float* sigma, int n_known, const std::string& w) {
  for (int j = 0; j < MT_MAX_DOF; ++j)
    MT_REQUIRE(h, first_unusable(&sigma[j], 1, kMaxFiniteBits) < 0 && (j < n_known ? sigma[j] > 0.f : sigma[j] >= 0.f),
               w + ".sigma[" + std::to_string(j) + "] must be finite and > 0");
  return MT_OK;
}
// A buffer a call reads or writes, for the aliasing rules: `bytes` from `p` on (0: not given).
struct Span {
  const void* p;
  size_t bytes;
  const char* name;
};
static size_t rows_bytes(int64_t rows, int64_t ld, int64_t n, size_t elem = 4) { return (size_t)((rows - 1) * ld + n) * elem; }
// Every output against the weights, against every input and against the outputs behind it.
static int policy_overlap_screen(mt_handle h, const PolicyNet& p, const PolicyLayout& s, const Span* out, int n_out, const Span* in, int n_in,
                                 const std::string& w) {
  for (int a = 0; a < n_out; ++a) {
    const std::string msg = w + "." + out[a].name + " overlaps ";
    for (int l = 0; l < p.n_layers; ++l)
      MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, p.weight[l], (size_t)s.n_out[l] * s.n_in[l] * 4) &&
                        !bytes_overlap(out[a].p, out[a].bytes, p.bias[l], (size_t)s.n_out[l] * 4),
                 msg + "weight / bias [" + std::to_string(l) + "]");
    for (int b = 0; b < n_in; ++b) MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes), msg + in[b].name);
    for (int b = a + 1; b < n_out; ++b) MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes), msg + out[b].name);
  }
  return MT_OK;
}

// mt_policy_grad and mt_value_grad behind their own struct_size checks: the value head's gradient is the policy's with one
// output (n_last = 1), sigma = 1 (sigma NULL) and the target in the action's place (`act` names it in the messages).
struct PolicyGradCall {
  PolicyNet net;
  const float* sigma;  // MT_MAX_DOF of them, or NULL: 1
  int n_last;          // outputs of the last layer; 0 = the handle's D
  const float* action;
  int64_t act_ld;
  const char* act;     // "action" / "target"
  const char* act_ld_name;
  const float* coef;
  int64_t coef_ld;
  float scale;
  float* grad_out;
  float* loss_out;
  void* workspace;
  size_t workspace_bytes;
};
static int policy_grad_call(mt_handle h, const PolicyGradCall& c, const std::string& w) {
  const PolicyNet& p = c.net;
  // what needs no handle: the scalars
  int rc = policy_net_screen(h, p, w);
  if (rc) return rc;
  MT_REQUIRE(h, first_unusable(&c.scale, 1, kMaxFiniteBits) < 0, w + ".scale must be finite");
  if (c.sigma && (rc = policy_sigma_screen(h, c.sigma, 1, w))) return rc;
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const int L = p.n_layers;
  const int D = c.n_last ? c.n_last : h->D;  // the outputs of the last layer
  if (c.sigma)
    for (int j = 0; j < D; ++j) MT_REQUIRE(h, c.sigma[j] > 0.f, w + ".sigma[" + std::to_string(j) + "] must be finite and > 0");
  PolicyLayout s;
  MT_REQUIRE(h, policy_layout(h, L, p.width, p.flags, &s, c.n_last), w + ": not a policy shape");
  const int T = p.n_steps;
  const int64_t n = h->n, P = s.P;
  const int IN = s.n_in[0];
  // policy_grad_kernel streams x as K triples and, with see_pose, r.D single words behind them: with r.D = h->D that is
  // x as mt_rollout_policy lays it out; with another output count the same IN words are regrouped (the fmaf chain of an
  // output runs over x in ascending order either way), which needs IN = 3 K' or 3 K' + r.D
  const int x_singles = D == h->D ? ((p.flags & MT_POLICY_SEE_POSE) ? D : 0) : IN % 3;
  if (x_singles != 0 && x_singles != D)
    return fail(h, MT_ERR_UNSUPPORTED, w + ": MT_POLICY_SEE_POSE with " + std::to_string(h->D) + " joints (supported: 3, 4, 6, 7)");
  MT_REQUIRE(h, c.grad_out != nullptr, w + ".grad_out is NULL");
  const size_t need = T ? (size_t)policy_grad_blocks(h, T) * (size_t)(P + 1) * sizeof(float) : 0;
  if (T) {
    for (int l = 0; l < L; ++l)
      MT_REQUIRE(h, p.weight[l] != nullptr && p.bias[l] != nullptr, w + ".weight / bias [" + std::to_string(l) + "] is NULL");
    MT_REQUIRE(h, p.obs != nullptr && c.action != nullptr && c.coef != nullptr, w + ".obs / " + c.act + " / coef is NULL");
    MT_REQUIRE(h, p.obs_ld >= n, w + ".obs_ld is smaller than n_envs");
    MT_REQUIRE(h, c.act_ld >= n, w + "." + c.act_ld_name + " is smaller than n_envs");
    MT_REQUIRE(h, c.coef_ld >= n, w + ".coef_ld is smaller than n_envs");
    MT_REQUIRE(h, c.workspace != nullptr && ((uintptr_t)c.workspace & 3u) == 0, w + ".workspace is NULL or not 4-byte aligned");
    MT_REQUIRE(h, c.workspace_bytes >= need, w + ".workspace_bytes is smaller than " + w + "_workspace() = " + std::to_string(need));
    // the outputs against the inputs and against each other
    const Span out[3] = {{c.grad_out, (size_t)P * 4, "grad_out"}, {c.loss_out, c.loss_out ? (size_t)4 : 0, "loss_out"}, {c.workspace, need, "workspace"}};
    const Span in[3] = {{p.obs, rows_bytes((int64_t)T * IN, p.obs_ld, n), "obs"},
                        {c.action, rows_bytes((int64_t)T * D, c.act_ld, n), c.act},
                        {c.coef, rows_bytes(T, c.coef_ld, n), "coef"}};
    if ((rc = policy_overlap_screen(h, p, s, out, 3, in, 3, w))) return rc;
  }
  MT_ENTER(h);
  PolicyGradArgs r{};
  for (int l = 0; l < L; ++l) {
    r.w[l] = p.weight[l];
    r.b[l] = p.bias[l];
    r.n_in[l] = s.n_in[l];
    r.n_out[l] = s.n_out[l];
    r.off[l] = s.off[l];
  }
  r.L = L;
  r.T = T;
  r.K = (IN - x_singles) / 3;
  r.D = D;
  r.hidden_act = p.hidden_act;
  r.out_act = p.out_act;
  r.out_scale = p.out_scale;
  for (int j = 0; j < D; ++j) r.inv_var[j] = c.sigma ? (float)(1.0 / ((double)c.sigma[j] * (double)c.sigma[j])) : 1.f;
  r.see_pose = x_singles ? 1u : 0u;
  r.obs = p.obs;
  r.obs_ld = p.obs_ld;
  r.action = c.action;
  r.act_ld = c.act_ld;
  r.coef = c.coef;
  r.coef_ld = c.coef_ld;
  r.n = n;
  r.tiles_per_step = (n + kBlock - 1) / kBlock;
  r.tiles = (int64_t)T * r.tiles_per_step;
  r.P = P;
  r.partials = static_cast<float*>(c.workspace);
  r.blocks = T ? (int32_t)policy_grad_blocks(h, T) : 0;
  r.scale = c.scale;
  r.grad = c.grad_out;
  r.loss = c.loss_out;
  if (T) {
    // the smallest compiled (extent, chunks of x) that holds the policy: kernels.h PolicyGradShape
    if (s.widest <= 32)
      hipLaunchKernelGGL((policy_grad_kernel<32, 4>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    else if (IN <= 64)
      hipLaunchKernelGGL((policy_grad_kernel<64, 1>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    else
      hipLaunchKernelGGL((policy_grad_kernel<64, 2>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    if ((rc = check_launch(h, "policy_grad_kernel"))) return rc;
  }
  hipLaunchKernelGGL(policy_grad_reduce_kernel, grid_for(P + 1), dim3(kBlock), 0, h->stream, r);
  return check_launch(h, "policy_grad_reduce_kernel");
}

int mt_policy_grad(mt_handle h, const struct mt_policy_grad* p) {
  MT_REQUIRE(h, p != nullptr, "policy_grad is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_policy_grad), "mt_policy_grad.struct_size does not match this library");
  const PolicyGradCall c{MT_POLICY_NET(p), p->sigma, 0, p->action, p->act_ld, "action", "act_ld", p->coef, p->coef_ld, p->scale,
                         p->grad_out, p->loss_out, p->workspace, p->workspace_bytes};
  return policy_grad_call(h, c, "mt_policy_grad");
}

size_t mt_value_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps) {
  return policy_grad_workspace(h, n_layers, width, flags, n_steps, 1);
}
int mt_value_grad(mt_handle h, const struct mt_value_grad* p) {
  MT_REQUIRE(h, p != nullptr, "value_grad is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_value_grad), "mt_value_grad.struct_size does not match this library");
  const PolicyGradCall c{MT_POLICY_NET(p), nullptr, 1, p->target, p->target_ld, "target", "target_ld", p->coef, p->coef_ld, p->scale,
                         p->grad_out, p->loss_out, p->workspace, p->workspace_bytes};
  return policy_grad_call(h, c, "mt_value_grad");
}

// mt_ppo_grad: mt_policy_grad's screens, grid and first-pass kernel (in its PPO mode), rows of kPpoExtras more words
static size_t ppo_grad_row_bytes(const PolicyLayout& s) { return (size_t)(s.P + 1 + kPpoExtras) * sizeof(float); }
size_t mt_ppo_grad_workspace(mt_handle h, int n_layers, const int32_t width[2], uint32_t flags, int n_steps) {
  PolicyLayout s;
  const int32_t none[2] = {0, 0};
  if (!h || n_steps <= 0 || n_steps > 65535 || !policy_layout(h, n_layers, width ? width : none, flags, &s)) return 0;
  return (size_t)policy_grad_blocks(h, n_steps) * ppo_grad_row_bytes(s);
}
int mt_ppo_grad(mt_handle h, const struct mt_ppo_grad* p) {
  MT_REQUIRE(h, p != nullptr, "ppo_grad is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_ppo_grad), "mt_ppo_grad.struct_size does not match this library");
  const std::string w = "mt_ppo_grad";
  const PolicyNet net = MT_POLICY_NET(p);
  // what needs no handle: the scalars
  int rc = policy_net_screen(h, net, w);
  if (rc) return rc;
  MT_REQUIRE(h, first_unusable(&p->scale, 1, kMaxFiniteBits) < 0, w + ".scale must be finite");
  MT_REQUIRE(h, first_unusable(&p->clip, 1, kMaxFiniteBits) < 0 && (p->clip == 0.f || (p->clip > 0.f && p->clip < 1.f)),
             w + ".clip must be 0 (no clipping) or in (0, 1)");
  MT_REQUIRE(h, first_unusable(&p->log_ratio_shift, 1, kMaxFiniteBits) < 0, w + ".log_ratio_shift must be finite");
  if ((rc = policy_sigma_screen(h, p->sigma, 1, w))) return rc;
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const int L = p->n_layers, T = p->n_steps, D = h->D;
  for (int j = 0; j < D; ++j) MT_REQUIRE(h, p->sigma[j] > 0.f, w + ".sigma[" + std::to_string(j) + "] must be finite and > 0");
  PolicyLayout s;
  MT_REQUIRE(h, policy_layout(h, L, p->width, p->flags, &s), w + ": not a policy shape");
  const int64_t n = h->n, P = s.P;
  const int IN = s.n_in[0];
  MT_REQUIRE(h, p->grad_out != nullptr, w + ".grad_out is NULL");
  MT_REQUIRE(h, ((uintptr_t)p->count_out & 7u) == 0, w + ".count_out is not 8-byte aligned");
  const size_t need = T ? (size_t)policy_grad_blocks(h, T) * ppo_grad_row_bytes(s) : 0;
  if (T) {
    for (int l = 0; l < L; ++l)
      MT_REQUIRE(h, p->weight[l] != nullptr && p->bias[l] != nullptr, w + ".weight / bias [" + std::to_string(l) + "] is NULL");
    MT_REQUIRE(h, p->obs != nullptr && p->action != nullptr && p->adv != nullptr && p->old_logp != nullptr,
               w + ".obs / action / adv / old_logp is NULL");
    MT_REQUIRE(h, p->obs_ld >= n, w + ".obs_ld is smaller than n_envs");
    MT_REQUIRE(h, p->act_ld >= n, w + ".act_ld is smaller than n_envs");
    MT_REQUIRE(h, p->adv_ld >= n, w + ".adv_ld is smaller than n_envs");
    MT_REQUIRE(h, p->old_ld >= n, w + ".old_ld is smaller than n_envs");
    MT_REQUIRE(h, p->sample_weight == nullptr || p->weight_ld >= n, w + ".weight_ld is smaller than n_envs");
    MT_REQUIRE(h, p->ratio_out == nullptr || p->ratio_ld >= n, w + ".ratio_ld is smaller than n_envs");
    MT_REQUIRE(h, p->coef_out == nullptr || p->coef_ld >= n, w + ".coef_ld is smaller than n_envs");
    MT_REQUIRE(h, p->workspace != nullptr && ((uintptr_t)p->workspace & 3u) == 0, w + ".workspace is NULL or not 4-byte aligned");
    MT_REQUIRE(h, p->workspace_bytes >= need, w + ".workspace_bytes is smaller than " + w + "_workspace() = " + std::to_string(need));
  }
  {  // the outputs against the weights, the inputs and each other (what n_steps == 0 leaves unread has no bytes)
    const auto rows = [&](const void* q, int64_t r, int64_t ld) { return (q && T) ? rows_bytes(r, ld, n) : (size_t)0; };
    const Span out[8] = {{p->grad_out, (size_t)P * 4, "grad_out"},
                         {p->loss_out, p->loss_out ? (size_t)4 : 0, "loss_out"},
                         {p->sigma_grad_out, p->sigma_grad_out ? (size_t)D * 4 : 0, "sigma_grad_out"},
                         {p->kl_out, p->kl_out ? (size_t)4 : 0, "kl_out"},
                         {p->count_out, p->count_out ? (size_t)16 : 0, "count_out"},
                         {p->ratio_out, rows(p->ratio_out, T, p->ratio_ld), "ratio_out"},
                         {p->coef_out, rows(p->coef_out, T, p->coef_ld), "coef_out"},
                         {p->workspace, need, "workspace"}};
    const Span in[5] = {{p->obs, rows(p->obs, (int64_t)T * IN, p->obs_ld), "obs"},
                        {p->action, rows(p->action, (int64_t)T * D, p->act_ld), "action"},
                        {p->adv, rows(p->adv, T, p->adv_ld), "adv"},
                        {p->old_logp, rows(p->old_logp, T, p->old_ld), "old_logp"},
                        {p->sample_weight, rows(p->sample_weight, T, p->weight_ld), "sample_weight"}};
    PolicyNet weights = net;
    if (!T) weights.n_layers = 0;  // (not read, and free to be NULL)
    if ((rc = policy_overlap_screen(h, weights, s, out, 8, in, 5, w))) return rc;
  }
  MT_ENTER(h);
  PpoGradArgs r{};
  for (int l = 0; l < L; ++l) {
    r.w[l] = p->weight[l];
    r.b[l] = p->bias[l];
    r.n_in[l] = s.n_in[l];
    r.n_out[l] = s.n_out[l];
    r.off[l] = s.off[l];
  }
  r.L = L;
  r.T = T;
  r.K = h->K;
  r.D = D;
  r.hidden_act = p->hidden_act;
  r.out_act = p->out_act;
  r.out_scale = p->out_scale;
  for (int j = 0; j < D; ++j) r.inv_var[j] = (float)(1.0 / ((double)p->sigma[j] * (double)p->sigma[j]));
  r.see_pose = (p->flags & MT_POLICY_SEE_POSE) ? 1u : 0u;
  r.obs = p->obs;
  r.obs_ld = p->obs_ld;
  r.action = p->action;
  r.act_ld = p->act_ld;
  r.coef = p->adv;
  r.coef_ld = p->adv_ld;
  r.n = n;
  r.tiles_per_step = (n + kBlock - 1) / kBlock;
  r.tiles = (int64_t)T * r.tiles_per_step;
  r.P = P;
  r.partials = static_cast<float*>(p->workspace);
  r.blocks = T ? (int32_t)policy_grad_blocks(h, T) : 0;
  r.scale = p->scale;
  r.grad = p->grad_out;
  r.loss = p->loss_out;
  r.old_logp = p->old_logp;
  r.old_ld = p->old_ld;
  r.weight = p->sample_weight;
  r.weight_ld = p->weight_ld;
  r.lo = (float)(1.0 - (double)p->clip);
  r.hi = (float)(1.0 + (double)p->clip);
  r.shift = p->log_ratio_shift;
  r.clipping = p->clip > 0.f ? 1u : 0u;
  r.ratio = p->ratio_out;
  r.ratio_ld = p->ratio_ld;
  r.coef_out = p->coef_out;
  r.coefo_ld = p->coef_ld;
  r.sigma_grad = p->sigma_grad_out;
  r.kl = p->kl_out;
  r.count = reinterpret_cast<long long*>(p->count_out);
  if (T) {
    // the (extent, chunks of x) mt_policy_grad picks
    if (s.widest <= 32)
      hipLaunchKernelGGL((policy_grad_kernel<32, 4, 1>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    else if (IN <= 64)
      hipLaunchKernelGGL((policy_grad_kernel<64, 1, 1>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    else
      hipLaunchKernelGGL((policy_grad_kernel<64, 2, 1>), dim3((unsigned)r.blocks), dim3(kBlock), 0, h->stream, r);
    if ((rc = check_launch(h, "policy_grad_kernel"))) return rc;
  }
  hipLaunchKernelGGL(ppo_grad_reduce_kernel, grid_for(P + 1 + kPpoExtras), dim3(kBlock), 0, h->stream, r);
  return check_launch(h, "ppo_grad_reduce_kernel");
}

int mt_policy_eval(mt_handle h, const struct mt_policy_eval* p) {
  MT_REQUIRE(h, p != nullptr, "policy_eval is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_policy_eval), "mt_policy_eval.struct_size does not match this library");
  const std::string w = "mt_policy_eval";
  const PolicyNet net = MT_POLICY_NET(p);
  int rc = policy_net_screen(h, net, w);
  if (rc) return rc;
  MT_REQUIRE(h, p->n_out >= 0 && p->n_out <= MT_MAX_DOF, w + ".n_out must be 0 (the handle's D) or 1.." + std::to_string(MT_MAX_DOF));
  MT_REQUIRE(h, p->mean_out != nullptr || p->logp_out != nullptr, w + ": mean_out and logp_out are both NULL");
  MT_REQUIRE(h, p->logp_out == nullptr || p->action != nullptr, w + ".logp_out needs action");
  if (p->logp_out && (rc = policy_sigma_screen(h, p->sigma, p->n_out ? p->n_out : 1, w))) return rc;
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const int L = p->n_layers, T = p->n_steps, NO = p->n_out ? p->n_out : h->D;
  if (p->logp_out)
    for (int j = 0; j < NO; ++j) MT_REQUIRE(h, p->sigma[j] > 0.f, w + ".sigma[" + std::to_string(j) + "] must be finite and > 0");
  PolicyLayout s;
  MT_REQUIRE(h, policy_layout(h, L, p->width, p->flags, &s, NO), w + ": not a policy shape");
  if (T == 0) return MT_OK;
  const int64_t n = h->n;
  const int IN = s.n_in[0];
  for (int l = 0; l < L; ++l)
    MT_REQUIRE(h, p->weight[l] != nullptr && p->bias[l] != nullptr, w + ".weight / bias [" + std::to_string(l) + "] is NULL");
  MT_REQUIRE(h, p->obs != nullptr, w + ".obs is NULL");
  MT_REQUIRE(h, p->obs_ld >= n, w + ".obs_ld is smaller than n_envs");
  MT_REQUIRE(h, p->mean_out == nullptr || p->mean_ld >= n, w + ".mean_ld is smaller than n_envs");
  MT_REQUIRE(h, p->logp_out == nullptr || p->act_ld >= n, w + ".act_ld is smaller than n_envs");
  MT_REQUIRE(h, p->logp_out == nullptr || p->logp_ld >= n, w + ".logp_ld is smaller than n_envs");
  const bool lp = p->logp_out != nullptr;  // (without it the actions are not read)
  const Span out[2] = {{p->mean_out, p->mean_out ? rows_bytes((int64_t)T * NO, p->mean_ld, n) : 0, "mean_out"},
                       {p->logp_out, lp ? rows_bytes(T, p->logp_ld, n) : 0, "logp_out"}};
  const Span in[2] = {{p->obs, rows_bytes((int64_t)T * IN, p->obs_ld, n), "obs"},
                      {p->action, lp ? rows_bytes((int64_t)T * NO, p->act_ld, n) : 0, "action"}};
  if ((rc = policy_overlap_screen(h, net, s, out, 2, in, 2, w))) return rc;
  MT_ENTER(h);
  PolicyEvalArgs r{};
  for (int l = 0; l < L; ++l) {
    r.w[l] = p->weight[l];
    r.b[l] = p->bias[l];
    r.n_in[l] = s.n_in[l];
    r.n_out[l] = s.n_out[l];
  }
  r.L = L;
  r.K = h->K;
  r.n_pose = IN - 3 * h->K;
  r.NO = NO;
  r.hidden_act = p->hidden_act;
  r.out_act = p->out_act;
  r.out_scale = p->out_scale;
  if (lp)
    for (int j = 0; j < NO; ++j) r.inv_var[j] = (float)(1.0 / ((double)p->sigma[j] * (double)p->sigma[j]));
  r.obs = p->obs;
  r.obs_ld = p->obs_ld;
  r.action = lp ? p->action : nullptr;
  r.act_ld = p->act_ld;
  r.mean = p->mean_out;
  r.mean_ld = p->mean_ld;
  r.logp = p->logp_out;
  r.logp_ld = p->logp_ld;
  r.n = n;
  // a block per tile of kBlock envs (x) of one step (y); the extent as mt_policy_grad picks it
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock), (unsigned)T);
  if (s.widest <= 32)
    hipLaunchKernelGGL((policy_eval_kernel<32>), grid, dim3(kBlock), 0, h->stream, r);
  else
    hipLaunchKernelGGL((policy_eval_kernel<64>), grid, dim3(kBlock), 0, h->stream, r);
  return check_launch(h, "policy_eval_kernel");
}

// mt_rollout_policy's launch with logp and a critic's values written beside its logs: the policy's screen and launch path
// (rollout_policy_screen, rollout_policy_run), the critic's shape through policy_layout with one output.
int mt_rollout_actor_critic(mt_handle h, const struct mt_actor_critic* p) {
  MT_REQUIRE(h, p != nullptr, "actor_critic is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, p->struct_size == (int32_t)sizeof(struct mt_actor_critic), "mt_actor_critic.struct_size does not match this library");
  MT_REQUIRE(h, p->policy.struct_size == (int32_t)sizeof(struct mt_policy), "mt_actor_critic.policy.struct_size does not match this library");
  const std::string w = "mt_actor_critic";
  MT_REQUIRE(h, p->reserved == 0, w + ".reserved must be 0");
  MT_REQUIRE(h, p->policy.reserved == 0, w + ".policy.reserved must be 0");
  const int CL = p->critic_layers;
  MT_REQUIRE(h, CL >= 0 && CL <= MT_POLICY_MAX_LAYERS, w + ".critic_layers must be 0 (no critic) or 1.." + std::to_string(MT_POLICY_MAX_LAYERS));
  int c_widest = 0;
  for (int l = 0; l + 1 < CL; ++l) {
    MT_REQUIRE(h, p->critic_width[l] >= 1 && p->critic_width[l] <= MT_POLICY_MAX_WIDTH,
               w + ".critic_width[" + std::to_string(l) + "] must be 1.." + std::to_string(MT_POLICY_MAX_WIDTH));
    c_widest = std::max(c_widest, (int)p->critic_width[l]);
  }
  if (CL) {
    MT_REQUIRE(h, CL == 1 || p->critic_hidden_act == MT_ACT_TANH || p->critic_hidden_act == MT_ACT_RELU,
               w + ".critic_hidden_act must be MT_ACT_TANH or MT_ACT_RELU");
    MT_REQUIRE(h, p->critic_out_act == MT_ACT_TANH || p->critic_out_act == MT_ACT_IDENTITY,
               w + ".critic_out_act must be MT_ACT_TANH or MT_ACT_IDENTITY");
    MT_REQUIRE(h, first_unusable(&p->critic_out_scale, 1, kMaxFiniteBits) < 0, w + ".critic_out_scale must be finite");
  }
  MT_REQUIRE(h, CL || !p->value_log, w + ".value_log needs a critic (critic_layers is 0)");
  MT_REQUIRE(h, CL || !p->last_value_out, w + ".last_value_out needs a critic (critic_layers is 0)");
  MT_REQUIRE(h, CL || p->logp_log, w + ": no critic and no logp_log: that call is mt_rollout_policy");
  int rc;
  if (p->logp_log && (rc = policy_sigma_screen(h, p->policy.sigma, 1, w + ".policy"))) return rc;
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const struct mt_policy* q = &p->policy;
  PolicyScreen sc;
  rc = rollout_policy_screen(h, q, w + ".policy", "mt_rollout_actor_critic", &sc);
  if (rc || q->n_steps == 0) return rc;
  if (p->logp_log)
    for (int j = 0; j < h->D; ++j)
      MT_REQUIRE(h, q->sigma[j] > 0.f, w + ".policy.sigma[" + std::to_string(j) + "] must be finite and > 0 with logp_log");
  const int T = q->n_steps, D = h->D;
  const int64_t n = h->n;
  const uint32_t see_pose = q->flags & MT_POLICY_SEE_POSE;
  PolicyLayout ps, cs{};
  MT_REQUIRE(h, policy_layout(h, q->n_layers, q->width, see_pose, &ps), w + ".policy: not a policy shape");
  const int IN = ps.n_in[0];
  if (CL) {
    MT_REQUIRE(h, policy_layout(h, CL, p->critic_width, see_pose, &cs, 1), w + ": not a critic shape");
    for (int l = 0; l < CL; ++l)
      MT_REQUIRE(h, p->critic_weight[l] != nullptr && p->critic_bias[l] != nullptr, w + ".critic_weight / critic_bias [" + std::to_string(l) + "] is NULL");
    // the lanes' x columns share the block's LDS with the target tile
    if (actor_critic_lds(h, IN, true) > (size_t)MT_ACTOR_CRITIC_MAX_LDS)
      return fail(h, MT_ERR_UNSUPPORTED,
                  "mt_rollout_actor_critic: a critic needs 3 K + IN <= " + std::to_string(MT_ACTOR_CRITIC_MAX_LDS / (kBlock * 4)) +
                      " (the targets and x of a block in LDS); this handle has 3 K + IN = " + std::to_string(3 * h->K + IN));
  }
  MT_REQUIRE(h, !p->logp_log || p->logp_ld >= n, w + ".logp_ld is smaller than n_envs");
  MT_REQUIRE(h, !p->value_log || p->value_ld >= n, w + ".value_ld is smaller than n_envs");
  const Span out[3] = {{p->logp_log, p->logp_log ? rows_bytes(T, p->logp_ld, n) : 0, "logp_log"},
                       {p->value_log, p->value_log ? rows_bytes(T, p->value_ld, n) : 0, "value_log"},
                       {p->last_value_out, p->last_value_out ? (size_t)n * 4 : 0, "last_value_out"}};
  const Span logs[5] = {{q->action_log, q->action_log ? rows_bytes((int64_t)T * D, q->act_ld, n) : 0, "policy.action_log"},
                        {q->obs_log, q->obs_log ? rows_bytes((int64_t)T * IN, q->obs_ld, n) : 0, "policy.obs_log"},
                        {q->reward_log, q->reward_log ? rows_bytes(T, q->log_ld, n, 1) : 0, "policy.reward_log"},
                        {q->done_log, q->done_log ? rows_bytes(T, q->log_ld, n, 1) : 0, "policy.done_log"},
                        {q->return_out, q->return_out ? (size_t)n * 4 : 0, "policy.return_out"}};
  PolicyNet pnet{};
  pnet.n_layers = q->n_layers;
  pnet.weight = q->weight;
  pnet.bias = q->bias;
  if ((rc = policy_overlap_screen(h, pnet, ps, out, 3, logs, 5, w))) return rc;
  for (int a = 0; a < 3 && CL; ++a)
    for (int l = 0; l < CL; ++l)
      MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, p->critic_weight[l], (size_t)cs.n_out[l] * cs.n_in[l] * 4) &&
                        !bytes_overlap(out[a].p, out[a].bytes, p->critic_bias[l], (size_t)cs.n_out[l] * 4),
                 w + "." + out[a].name + " overlaps critic_weight / critic_bias [" + std::to_string(l) + "]");
  MT_ENTER(h);
  ActorCriticArgs r{};
  for (int l = 0; l < CL; ++l) {
    r.cw[l] = p->critic_weight[l];
    r.cb[l] = p->critic_bias[l];
    r.c_n_in[l] = cs.n_in[l];
    r.c_n_out[l] = cs.n_out[l];
  }
  r.CL = CL;
  r.c_hidden_act = p->critic_hidden_act;
  r.c_out_act = p->critic_out_act;
  r.c_out_scale = p->critic_out_scale;
  if (p->logp_log)
    for (int j = 0; j < D; ++j) r.inv_var[j] = (float)(1.0 / ((double)q->sigma[j] * (double)q->sigma[j]));
  r.logp_log = p->logp_log;
  r.logp_ld = p->logp_ld;
  r.value_log = p->value_log;
  r.value_ld = p->value_ld;
  r.last_value = p->last_value_out;
  return rollout_policy_run(h, q, sc, 1u, 0, &r, c_widest);
}

int mt_gae(mt_handle h, const struct mt_gae* s) {
  MT_REQUIRE(h, s != nullptr, "gae is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_gae), "mt_gae.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_gae.reserved must be 0");
  MT_REQUIRE(h, (s->flags & ~(uint32_t)MT_GAE_MASK_AFTER_DONE) == 0, "mt_gae.flags: unknown MT_GAE_* flag");
  MT_REQUIRE(h, s->n_steps >= 0 && s->n_steps <= 65535, "mt_gae.n_steps must be 0..65535");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&s->gamma, 1, kMaxFiniteBits) < 0 && s->gamma >= 0.f && s->gamma <= 1.f, "mt_gae.gamma must be in [0, 1]");
  MT_REQUIRE(h, first_unusable(&s->lambda, 1, kMaxFiniteBits) < 0 && s->lambda >= 0.f && s->lambda <= 1.f, "mt_gae.lambda must be in [0, 1]");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (s->n_steps == 0) return MT_OK;
  const int64_t n = h->n, T = s->n_steps;
  MT_REQUIRE(h, s->reward_log != nullptr && s->done_log != nullptr && s->value != nullptr, "mt_gae.reward_log / done_log / value is NULL");
  MT_REQUIRE(h, s->adv_out != nullptr, "mt_gae.adv_out is NULL");
  MT_REQUIRE(h, s->log_ld >= n, "mt_gae.log_ld is smaller than n_envs");
  MT_REQUIRE(h, s->value_ld >= n, "mt_gae.value_ld is smaller than n_envs");
  MT_REQUIRE(h, s->adv_ld >= n, "mt_gae.adv_ld is smaller than n_envs");
  MT_REQUIRE(h, s->ret_out == nullptr || s->ret_ld >= n, "mt_gae.ret_ld is smaller than n_envs");
  MT_REQUIRE(h, s->weight_out == nullptr || s->weight_ld >= n, "mt_gae.weight_ld is smaller than n_envs");
  const Span out[3] = {{s->adv_out, rows_bytes(T, s->adv_ld, n), "adv_out"},
                       {s->ret_out, s->ret_out ? rows_bytes(T, s->ret_ld, n) : 0, "ret_out"},
                       {s->weight_out, s->weight_out ? rows_bytes(T, s->weight_ld, n) : 0, "weight_out"}};
  const Span in[4] = {{s->reward_log, rows_bytes(T, s->log_ld, n, 1), "reward_log"},
                      {s->done_log, rows_bytes(T, s->log_ld, n, 1), "done_log"},
                      {s->value, rows_bytes(T, s->value_ld, n), "value"},
                      {s->last_value, s->last_value ? (size_t)n * 4 : 0, "last_value"}};
  for (int a = 0; a < 3; ++a) {
    const std::string msg = std::string("mt_gae.") + out[a].name + " overlaps ";
    for (int b = 0; b < 4; ++b) MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes), msg + in[b].name);
    for (int b = a + 1; b < 3; ++b) MT_REQUIRE(h, !bytes_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes), msg + out[b].name);
  }
  MT_ENTER(h);
  GaeArgs r{};
  r.reward = s->reward_log;
  r.done = s->done_log;
  r.log_ld = s->log_ld;
  r.value = s->value;
  r.value_ld = s->value_ld;
  r.last_value = s->last_value;
  r.gamma = s->gamma;
  r.gl = s->gamma * s->lambda;  // one fp32 product (-ffp-contract=off)
  r.adv = s->adv_out;
  r.adv_ld = s->adv_ld;
  r.ret = s->ret_out;
  r.ret_ld = s->ret_ld;
  r.weight = s->weight_out;
  r.weight_ld = s->weight_ld;
  r.n = n;
  r.T = s->n_steps;
  r.mask_after_done = (s->flags & MT_GAE_MASK_AFTER_DONE) ? 1u : 0u;
  hipLaunchKernelGGL(gae_kernel, grid_for(n), dim3(kBlock), 0, h->stream, r);
  return check_launch(h, "gae_kernel");
}

int mt_reward_to_go(mt_handle h, const struct mt_reward_to_go* s) {
  MT_REQUIRE(h, s != nullptr, "reward_to_go is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_reward_to_go), "mt_reward_to_go.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_reward_to_go.reserved must be 0");
  MT_REQUIRE(h, (s->flags & ~(uint32_t)MT_RTG_MASK_AFTER_DONE) == 0, "mt_reward_to_go.flags: unknown MT_RTG_* flag");
  MT_REQUIRE(h, s->n_steps >= 0 && s->n_steps <= 65535, "mt_reward_to_go.n_steps must be 0..65535");
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&s->gamma, 1, kMaxFiniteBits) < 0 && s->gamma >= 0.f && s->gamma <= 1.f, "mt_reward_to_go.gamma must be in [0, 1]");
  MT_REQUIRE(h, first_unusable(&s->baseline, 1, kMaxFiniteBits) < 0, "mt_reward_to_go.baseline must be finite");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (s->n_steps == 0) return MT_OK;
  MT_REQUIRE(h, s->reward_log != nullptr && s->done_log != nullptr && s->out != nullptr, "mt_reward_to_go.reward_log / done_log / out is NULL");
  MT_REQUIRE(h, s->log_ld >= h->n, "mt_reward_to_go.log_ld is smaller than n_envs");
  MT_REQUIRE(h, s->out_ld >= h->n, "mt_reward_to_go.out_ld is smaller than n_envs");
  const size_t log_bytes = (size_t)(((int64_t)s->n_steps - 1) * s->log_ld + h->n);
  const size_t out_bytes = (size_t)(((int64_t)s->n_steps - 1) * s->out_ld + h->n) * 4;
  MT_REQUIRE(h, !bytes_overlap(s->out, out_bytes, s->reward_log, log_bytes) && !bytes_overlap(s->out, out_bytes, s->done_log, log_bytes),
             "mt_reward_to_go.out overlaps reward_log / done_log");
  MT_ENTER(h);
  RewardToGoArgs r{};
  r.reward = s->reward_log;
  r.done = s->done_log;
  r.log_ld = s->log_ld;
  r.out = s->out;
  r.out_ld = s->out_ld;
  r.n = h->n;
  r.T = s->n_steps;
  r.gamma = s->gamma;
  r.baseline = s->baseline;
  r.mask_after_done = (s->flags & MT_RTG_MASK_AFTER_DONE) ? 1u : 0u;
  hipLaunchKernelGGL(reward_to_go_kernel, grid_for(h->n), dim3(kBlock), 0, h->stream, r);
  return check_launch(h, "reward_to_go_kernel");
}

int mt_shoot(mt_handle h, const struct mt_shoot* s) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s != nullptr, "shoot is NULL");
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_shoot), "mt_shoot.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_shoot.reserved must be 0");
  MT_REQUIRE(h, (s->flags & ~MT_SHOOT_AUTO_RESET) == 0, "mt_shoot.flags: unknown MT_SHOOT_* flag");
  const bool auto_reset = (s->flags & MT_SHOOT_AUTO_RESET) != 0;
  MT_REQUIRE(h, s->n_steps >= 0, "mt_shoot.n_steps must be >= 0");
  MT_REQUIRE(h, s->n_candidates >= 1 && s->n_candidates <= 64, "mt_shoot.n_candidates must be 1..64");
  MT_REQUIRE(h, s->commit_steps >= 0 && s->commit_steps <= s->n_steps, "mt_shoot.commit_steps must be 0..n_steps");
  MT_REQUIRE(h, !(auto_reset && s->commit_steps == 0), "MT_SHOOT_AUTO_RESET with mt_shoot.commit_steps == 0: an evaluation re-arms nothing");
  if (!fusable(h)) return fail_unfusable(h, "mt_shoot");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_shoot before mt_reset / mt_reset_random");
  if (s->n_steps == 0) return MT_OK;
  const int H = s->commit_steps;
  MT_REQUIRE(h, s->actions != nullptr, "mt_shoot.actions is NULL");
  MT_REQUIRE(h, s->ld >= h->n, "mt_shoot.ld is smaller than n_envs");
  MT_REQUIRE(h, s->cand_stride >= (int64_t)s->n_steps * h->D * s->ld, "mt_shoot.cand_stride is smaller than n_steps * dof * ld");
  MT_REQUIRE(h, !s->returns_out || s->ret_ld >= h->n, "mt_shoot.ret_ld is smaller than n_envs");
  MT_REQUIRE(h, !(H > 0 && s->best_out == nullptr), "mt_shoot.best_out is NULL with commit_steps > 0");
  MT_REQUIRE(h, !(H > 0 && (s->reward_log || s->done_log)) || s->log_ld >= h->n, "mt_shoot.log_ld is smaller than n_envs");
  MT_ENTER(h);
  ShootArgs e{};
  e.plans = s->actions;
  e.ld = s->ld;
  e.cand_stride = s->cand_stride;
  e.returns_out = s->returns_out;
  e.ret_ld = s->ret_ld;
  e.best_out = s->best_out;
  e.best_return_out = s->best_return_out;
  e.T = s->n_steps;
  e.C = s->n_candidates;
  launch_shoot(h, h->args, e);  // reads the state, writes the caller's rows only
  int rc = check_launch(h, "shoot_kernel");
  if (rc || H == 0) return rc;
  // the commit: steps 0..H-1 of the plane each env's evaluation chose (nt_loads stays 0: the evaluation has just read these rows)
  TapeArgs r = tape_args(s, s->actions, s->ld, H);
  r.best = s->best_out;
  r.cand_stride = s->cand_stride;
  return commit_tape(h, r, s->seed, auto_reset, true);
}

int mt_sample_plans(mt_handle h, const struct mt_cem* s, void* plans_out, int64_t ld, int64_t cand_stride) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s != nullptr, "mt_sample_plans: cem is NULL");
  CemArgs e{};
  int rc = stream_args(h, s, "mt_sample_plans: ", kCemNames, e);
  if (rc) return rc;
  if (s->n_steps == 0) return MT_OK;
  rc = stream_rows(h, s, "mt_sample_plans: ", kCemNames);
  if (rc) return rc;
  MT_REQUIRE(h, plans_out != nullptr, "mt_sample_plans: plans_out is NULL");
  MT_REQUIRE(h, ld >= h->n, "mt_sample_plans: ld is smaller than n_envs");
  MT_REQUIRE(h, cand_stride >= (int64_t)s->n_steps * h->D * ld, "mt_sample_plans: cand_stride is smaller than n_steps * dof * ld");
  MT_ENTER(h);
  MT_DISPATCH_D(h->D, launch_sample_plans_d, h, e, static_cast<float*>(plans_out), ld, cand_stride);
  return check_launch(h, "sample_plans_kernel");
}

int mt_cem(mt_handle h, const struct mt_cem* s) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s != nullptr, "cem is NULL");
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_cem), "mt_cem.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_cem.reserved must be 0");
  CemArgs e{};
  int rc = stream_args(h, s, "mt_cem: ", kCemNames, e);
  if (rc) return rc;
  const bool auto_reset = (s->flags & MT_CEM_AUTO_RESET) != 0;
  const int T = s->n_steps, H = s->commit_steps;
  MT_REQUIRE(h, s->n_elites >= 1 && s->n_elites <= s->n_candidates, "mt_cem.n_elites must be 1..n_candidates");
  MT_REQUIRE(h, H >= 0 && H <= T, "mt_cem.commit_steps must be 0..n_steps");
  MT_REQUIRE(h, !(auto_reset && H == 0), "MT_CEM_AUTO_RESET with mt_cem.commit_steps == 0: an evaluation re-arms nothing");
  MT_REQUIRE(h, first_unusable(&s->sigma_min, 1, kMaxFiniteBits) < 0 && s->sigma_min >= 0.f, "mt_cem.sigma_min must be finite and >= 0");
  if (!fusable(h)) return fail_unfusable(h, "mt_cem");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_cem before mt_reset / mt_reset_random");
  if (T == 0) return MT_OK;
  rc = stream_rows(h, s, "", kCemNames);
  if (rc) return rc;
  MT_REQUIRE(h, (s->mean_out == nullptr) == (s->sigma_out == nullptr), "mt_cem.mean_out and sigma_out: both or neither");
  rc = refit_args(h, s, kCemNames, e);
  if (rc) return rc;
  MT_ENTER(h);
  e.elite_mask = reinterpret_cast<unsigned long long*>(s->elite_mask_out);
  e.E = s->n_elites;
  e.inv_e = 1.0f / (float)s->n_elites;  // the fp32 nearest to 1 / E
  launch_cem(h, h->args, e);            // reads the state, writes the caller's rows only
  rc = check_launch(h, "cem_kernel");
  if (rc || H == 0) return rc;
  // the commit: mt_rollout_tape(n_steps = H, actions = chosen_out), host bookkeeping included
  TapeArgs r = tape_args(s, s->chosen_out, s->chosen_ld, H);
  r.nt_loads = h->tape_nt_loads ? 1u : 0u;
  return commit_tape(h, r, s->seed, auto_reset, false);
}

int mt_mppi(mt_handle h, const struct mt_mppi* s) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, s != nullptr, "mppi is NULL");
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_mppi), "mt_mppi.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_mppi.reserved must be 0");
  MppiArgs e{};
  int rc = stream_args(h, s, "", kMppiNames, e);
  if (rc) return rc;
  const bool auto_reset = (s->flags & MT_MPPI_AUTO_RESET) != 0;
  const int T = s->n_steps, H = s->commit_steps;
  MT_REQUIRE(h, H >= 0 && H <= T, "mt_mppi.commit_steps must be 0..n_steps");
  MT_REQUIRE(h, !(auto_reset && H == 0), "MT_MPPI_AUTO_RESET with mt_mppi.commit_steps == 0: an evaluation re-arms nothing");
  MT_REQUIRE(h, first_unusable(&s->sigma_min, 1, kMaxFiniteBits) < 0 && s->sigma_min >= 0.f, "mt_mppi.sigma_min must be finite and >= 0");
  // 0x3F800000 = 1.0f: a NaN, an inf or anything beyond 1 fails the first test, a negative value (not -0) the second
  MT_REQUIRE(h, first_unusable(&s->decay, 1, 0x3F800000u) < 0 && s->decay >= 0.f, "mt_mppi.decay must be finite and within 0..1");
  if (!fusable(h)) return fail_unfusable(h, "mt_mppi");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_mppi before mt_reset / mt_reset_random");
  if (T == 0) return MT_OK;
  rc = stream_rows(h, s, "", kMppiNames);
  if (rc) return rc;
  MT_REQUIRE(h, !(s->sigma_out && !s->mean_out), "mt_mppi.sigma_out without mean_out");
  rc = refit_args(h, s, kMppiNames, e);
  if (rc) return rc;
  MT_ENTER(h);
  e.weights_out = s->weights_out;
  e.w_ld = s->w_ld;
  e.weight_sum_out = s->weight_sum_out;
  e.decay = s->decay;
  launch_mppi(h, h->args, e);  // reads the state, writes the caller's rows only
  rc = check_launch(h, "mppi_kernel");
  if (rc || H == 0) return rc;
  // the commit: mt_rollout_tape(n_steps = H, actions = chosen_out), host bookkeeping included
  TapeArgs r = tape_args(s, s->chosen_out, s->chosen_ld, H);
  r.nt_loads = h->tape_nt_loads ? 1u : 0u;
  return commit_tape(h, r, s->seed, auto_reset, false);
}

int mt_observe(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_observe before reset");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  MT_DISPATCH_D(h->D, launch_observe_d, h);
  return check_launch(h, "observe_kernel");
}

int mt_check_done(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->is_reset) return fail(h, MT_ERR_STATE, "mt_check_done before reset");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  MT_DISPATCH_D(h->D, launch_check_done_d, h);
  return check_launch(h, "check_done_kernel");
}

// ---- inverse kinematics -------------------------------------------------------------------------
int mt_jacobian(mt_handle h, const void* angles, int64_t angles_ld, void* jac_out, int64_t jac_ld, void* pos_out,
                int64_t pos_ld) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, jac_out != nullptr, "mt_jacobian: jac_out is NULL");
  MT_REQUIRE(h, angles == nullptr || angles_ld >= h->n, "mt_jacobian: angles_ld is smaller than n_envs");
  MT_REQUIRE(h, jac_ld >= h->n, "mt_jacobian: jac_ld is smaller than n_envs");
  MT_REQUIRE(h, pos_out == nullptr || pos_ld >= h->n, "mt_jacobian: pos_ld is smaller than n_envs");
  if (h->args.dh.fe == 0) return fail(h, MT_ERR_UNSUPPORTED, "mt_jacobian: ee_frame is the origin row, which no joint moves");
  if (!angles && !h->is_reset) return fail(h, MT_ERR_STATE, "mt_jacobian of the resident pose before reset");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  JacobianArgs r{};
  r.angles = angles ? static_cast<const float*>(angles) : h->args.goals;
  r.angles_ld = angles ? angles_ld : h->ld;
  r.jac = static_cast<float*>(jac_out);
  r.jac_ld = jac_ld;
  r.pos = static_cast<float*>(pos_out);
  r.pos_ld = pos_ld;
  r.n = h->n;
  r.dh = h->args.dh;
  launch_jacobian(h, r);
  return check_launch(h, "jacobian_kernel");
}

// Staging (MT_IK_STAGE) needs no bookkeeping of its own: MT_F_ACTIONS has no host-side record (only MT_F_GOALS and
// MT_F_POINTS have: GoalsRow, codes_valid, the exposure flags), and the mt_step that executes staged actions is what ends
// kFlagWholeGoals and the record of the pose -- whoever staged them.  The call enters as mt_observe does, which folds the
// chains back, so the write is ordered ahead of a per-chain mt_step as well.
int mt_ik(mt_handle h, const struct mt_ik* s) {
  MT_REQUIRE(h, s != nullptr, "ik is NULL");  // (the struct first: its size is checked with or without a handle)
  MT_REQUIRE(h, s->struct_size == (int32_t)sizeof(struct mt_ik), "mt_ik.struct_size does not match this library");
  MT_REQUIRE(h, s->reserved == 0, "mt_ik.reserved must be 0");
  MT_REQUIRE(h, (s->flags & ~(uint32_t)(MT_IK_STAGE | MT_IK_WRAP)) == 0, "mt_ik.flags: unknown MT_IK_* flag");
  MT_REQUIRE(h, s->iters >= 1 && s->iters <= MT_IK_MAX_ITERS, "mt_ik.iters must be 1.." + std::to_string(MT_IK_MAX_ITERS));
  // (bit patterns: the build is -ffinite-math-only)
  MT_REQUIRE(h, first_unusable(&s->damping, 1, kMaxFiniteBits) < 0 && s->damping > 0.f, "mt_ik.damping must be finite and > 0");
  MT_REQUIRE(h, first_unusable(&s->max_step_deg, 1, kMaxFiniteBits) < 0 && s->max_step_deg > 0.f, "mt_ik.max_step_deg must be finite and > 0");
  MT_REQUIRE(h, first_unusable(&s->tol, 1, kMaxFiniteBits) < 0 && s->tol >= 0.f, "mt_ik.tol must be finite and >= 0");
  const bool stage = (s->flags & MT_IK_STAGE) != 0;
  MT_REQUIRE(h, stage || s->angles_out || s->residual_out || s->iters_out || s->index_out, "mt_ik: no output and no MT_IK_STAGE");
  MT_REQUIRE(h, s->target == nullptr || s->index_out == nullptr, "mt_ik.index_out is for the nearest-target mode (target NULL)");
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  const int64_t n = h->n;
  MT_REQUIRE(h, s->target == nullptr || s->target_ld >= n, "mt_ik.target_ld is smaller than n_envs");
  MT_REQUIRE(h, s->start == nullptr || s->start_ld >= n, "mt_ik.start_ld is smaller than n_envs");
  MT_REQUIRE(h, s->angles_out == nullptr || s->angles_ld >= n, "mt_ik.angles_ld is smaller than n_envs");
  if (h->args.dh.fe == 0) return fail(h, MT_ERR_UNSUPPORTED, "mt_ik: ee_frame is the origin row, which no joint moves");
  if ((!s->target || !s->start || stage) && !h->is_reset) return fail(h, MT_ERR_STATE, "mt_ik reads or stages resident state before reset");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  IkArgs r{};
  r.start = s->start ? s->start : h->args.goals;
  r.start_ld = s->start ? s->start_ld : h->ld;
  r.target = s->target;
  r.target_ld = s->target_ld;
  r.points = h->args.points;
  r.alive = h->args.alive;
  r.ld = h->ld;
  r.angles = s->angles_out;
  r.angles_ld = s->angles_ld;
  r.stage = stage ? h->args.actions : nullptr;
  r.residual = s->residual_out;
  r.steps = s->iters_out;
  r.index = s->index_out;
  r.n = n;
  r.K = h->K;
  r.iters = s->iters;
  r.wrap = (s->flags & MT_IK_WRAP) ? 1u : 0u;
  r.lambda2 = s->damping * s->damping;  // one fp32 product
  r.max_step = s->max_step_deg;
  r.tol = s->tol;
  r.dh = h->args.dh;
  launch_ik(h, r);
  return check_launch(h, "ik_kernel");
}

// ---- getters / setters ------------------------------------------------------------------------
static int64_t env_major_bytes(mt_handle h, int field) {
  const int64_t n = h->n;
  switch (field) {
    case MT_F_ACTIONS:
    case MT_F_GOALS: return n * h->D * 4;
    case MT_F_POINTS:
    case MT_F_OBS: return n * 3 * h->K * 4;
    case MT_F_ALIVE: return n * h->K;
    case MT_F_REWARD:
    case MT_F_TOTAL_REWARD:
    case MT_F_EPISODES:
    case MT_F_LAST_RETURN: return n * 4;
    case MT_F_DONE: return n;
    case MT_F_DONE_BITS: return (n + 63) / 64 * 8;
    case MT_F_EE: return n * 3 * 4;
    case MT_F_JOINTS: return n * h->D * 3 * 4;
    case MT_F_RETURN_RING: return h->args.ring ? n * (int64_t)h->args.ring_slots * 4 : -1;
    case MT_F_TRACE: return h->trace ? n * (int64_t)h->cfg.substeps * 3 * 4 : -1;
    case MT_F_ZMIN: return h->args.zmin ? n * 4 : -1;
    default: return -1;
  }
}

int mt_get(mt_handle h, int field, void* dst, int64_t dst_bytes, int is_device) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, dst != nullptr, "dst is NULL");
  const int64_t need = env_major_bytes(h, field);
  MT_REQUIRE(h, need > 0, "unknown field (or a field this handle was created without)");
  MT_REQUIRE(h, dst_bytes == need, "dst_bytes does not match the field's env-major size");
  MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  const dim3 g = grid_for(h->n), b(kBlock);
  void* out = dst;
  if (!is_device) {
    int rc = ensure_staging(h, (size_t)need);
    if (rc) return rc;
    out = h->staging;
  }
  const StepArgs& a = h->args;
  bool direct = false;  // single-row fields need no transpose
  const void* direct_src = nullptr;
  switch (field) {
    case MT_F_ACTIONS: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.actions, h->ld, h->D, h->n, (float*)out); break;
    case MT_F_GOALS: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.goals, h->ld, h->D, h->n, (float*)out); break;
    case MT_F_POINTS: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.points, h->ld, 3 * h->K, h->n, (float*)out); break;
    case MT_F_OBS: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.obs, h->ld, 3 * h->K, h->n, (float*)out); break;
    case MT_F_EE: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.ee, h->ld, 3, h->n, (float*)out); break;
    case MT_F_RETURN_RING: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, a.ring, h->ld, (int)a.ring_slots, h->n, (float*)out); break;
    case MT_F_TRACE: hipLaunchKernelGGL((soa_to_env_major<float>), g, b, 0, h->stream, h->trace, h->ld, 3 * h->cfg.substeps, h->n, (float*)out); break;
    case MT_F_ALIVE: hipLaunchKernelGGL(alive_unpack, g, b, 0, h->stream, a.alive, h->K, h->n, (uint8_t*)out); break;
    case MT_F_JOINTS: MT_DISPATCH_D(h->D, launch_joints_d, h, (float*)out); break;
    case MT_F_REWARD: direct = true; direct_src = a.reward; break;
    case MT_F_TOTAL_REWARD: direct = true; direct_src = a.total_reward; break;
    case MT_F_EPISODES: direct = true; direct_src = a.episodes; break;
    case MT_F_LAST_RETURN: direct = true; direct_src = a.last_return; break;
    case MT_F_DONE: direct = true; direct_src = a.done; break;
    case MT_F_DONE_BITS: direct = true; direct_src = a.done_bits; break;
    case MT_F_ZMIN: direct = true; direct_src = a.zmin; break;
    default: return fail(h, MT_ERR_INVALID_ARG, "unknown field");
  }
  if (direct) {
    MT_HIP(h, hipMemcpyAsync(dst, direct_src, (size_t)need, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             h->stream));
  } else {
    int rc = check_launch(h, "mt_get transpose");
    if (rc) return rc;
    if (!is_device) MT_HIP(h, hipMemcpyAsync(dst, h->staging, (size_t)need, hipMemcpyDeviceToHost, h->stream));
  }
  if (!is_device) MT_HIP(h, hipStreamSynchronize(h->stream));
  return MT_OK;
}

int mt_set(mt_handle h, int field, const void* src, int64_t src_bytes) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, src != nullptr, "src is NULL");
  MT_REQUIRE(h, field == MT_F_GOALS || field == MT_F_POINTS || field == MT_F_ALIVE || field == MT_F_TOTAL_REWARD ||
                    field == MT_F_DONE || field == MT_F_EPISODES || field == MT_F_LAST_RETURN || field == MT_F_RETURN_RING,
             "field is not settable");
  const int64_t need = env_major_bytes(h, field);
  MT_REQUIRE(h, need > 0, "the handle was created without this field");
  MT_REQUIRE(h, src_bytes == need, "src_bytes does not match the field's env-major size");
  if (field == MT_F_GOALS || field == MT_F_POINTS || field == MT_F_TOTAL_REWARD || field == MT_F_LAST_RETURN ||
      field == MT_F_RETURN_RING) {
    const int64_t bad = first_unusable((const float*)src, need / 4, field == MT_F_GOALS ? kMaxAngleBits : kMaxFiniteBits);
    if (bad >= 0)
      return fail(h, MT_ERR_INVALID_ARG, "mt_set: element " + std::to_string(bad) + " is NaN, infinite or (joint angles) beyond "
                                         "+-32768 degrees");
  }
  MT_ENTER(h);
  const dim3 g = grid_for(h->n), b(kBlock);
  const StepArgs& a = h->args;
  void* row = field == MT_F_TOTAL_REWARD ? (void*)a.total_reward : field == MT_F_DONE ? (void*)a.done :
              field == MT_F_EPISODES ? (void*)a.episodes : field == MT_F_LAST_RETURN ? (void*)a.last_return : nullptr;
  if (field == MT_F_LAST_RETURN || field == MT_F_RETURN_RING) {  // rows an in-place exchange may still be reading
    int rcg = order_behind_inplace_gather(h, h->stream);
    if (rcg) return rcg;
  }
  if (row) {  // single-row fields: env-major == SoA
    MT_HIP(h, hipMemcpyAsync(row, src, (size_t)need, hipMemcpyHostToDevice, h->stream));
    if (field == MT_F_DONE) {
      hipLaunchKernelGGL(done_bits_rebuild_kernel, g, b, 0, h->stream, a.done, h->n, a.done_bits);
      int rc = check_launch(h, "done_bits_rebuild_kernel");
      if (rc) return rc;
    }
  } else {
    int rc = ensure_staging(h, (size_t)need);
    if (rc) return rc;
    MT_HIP(h, hipMemcpyAsync(h->staging, src, (size_t)need, hipMemcpyHostToDevice, h->stream));
    if (field == MT_F_GOALS) {
      hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)h->staging, h->D, h->n, a.goals, h->ld);
      h->args.flags &= ~kFlagWholeGoals;
    } else if (field == MT_F_POINTS) {
      hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)h->staging, 3 * h->K, h->n, a.points, h->ld);
      h->codes_valid = false;  // anybody's floats: no codes for them
    }
    else if (field == MT_F_RETURN_RING)
      hipLaunchKernelGGL((env_major_to_soa<float>), g, b, 0, h->stream, (const float*)h->staging, (int)a.ring_slots, h->n, a.ring, h->ld);
    else
      hipLaunchKernelGGL(alive_pack, g, b, 0, h->stream, (const uint8_t*)h->staging, h->K, h->n, a.alive);
    rc = check_launch(h, "mt_set");
    if (rc) return rc;
  }
  MT_HIP(h, hipStreamSynchronize(h->stream));
  return MT_OK;
}

int mt_set_episode_base(mt_handle h, uint32_t episode0) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  h->args.episode0 = episode0;
  return MT_OK;
}

int mt_device_ptr(mt_handle h, int field, void** ptr, int64_t* rows, int64_t* ld, int* dtype) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, ptr != nullptr, "ptr is NULL");
  FieldInfo fi{};
  int rc = field_info(h, field, &fi);
  if (rc) return rc;
  if (h->reset_pending) {  // the caller is about to look at (or write) the rows themselves
    MT_ON_DEVICE(h, h->cfg.device);
    rc = flush_pending_reset(h);
    if (rc) return rc;
  }
  h->snap_valid = false;
  if (field == MT_F_GOALS) {
    // the caller can now write joint angles behind the library's back at any time: the host's knowledge that every
    // angle is a whole degree (kFlagWholeGoals: table look-ups for the pose a step starts from) ends here, for good
    h->goals_exposed = true;
    h->args.flags &= ~kFlagWholeGoals;
  }
  if (field == MT_F_POINTS) {  // the same for the targets: the step kernels read the floats from now on
    h->points_exposed = true;
    h->codes_valid = false;
  }
  *ptr = fi.ptr;
  if (rows) *rows = fi.rows;
  if (ld) *ld = (field == MT_F_DONE_BITS) ? h->ld / 64 : h->ld;
  if (dtype) *dtype = fi.dtype;
  return MT_OK;
}

// ---- timing -----------------------------------------------------------------------------------
int mt_timer_start(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ENTER_TIMER(h);
  MT_HIP(h, hipEventRecord(h->ev0, h->stream));
  return MT_OK;
}

int mt_timer_stop(mt_handle h, float* elapsed_ms) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, elapsed_ms != nullptr, "elapsed_ms is NULL");
  MT_ENTER_TIMER(h);
  MT_HIP(h, hipEventRecord(h->ev1, h->stream));
  MT_HIP(h, hipEventSynchronize(h->ev1));
  MT_HIP(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
  return MT_OK;
}

int mt_timer_stop_async(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_ON_DEVICE(h, h->cfg.device);  // NOT a join: one end event per stream that may still carry work of the handle
  MT_HIP(h, hipEventRecord(h->ev1, h->stream));
  h->timer_ends = 1;
  if (h->forked)
    for (int c = 1; c < h->chains; ++c) {
      if (!h->chain_streams[c] || (int64_t)c * chain_span(h, h->chains) >= h->n) continue;
      if (!h->ev1c[c]) MT_HIP(h, hipEventCreateWithFlags(&h->ev1c[c], event_flags(true)));
      MT_HIP(h, hipEventRecord(h->ev1c[c], h->chain_streams[c]));
      h->timer_ends = c + 1;
    }
  h->timer_with_gather = h->gather_pending;  // an exchange begun on the side stream ends at ev_g1
  return MT_OK;
}

int mt_timer_read(mt_handle h, float* elapsed_ms) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, elapsed_ms != nullptr, "elapsed_ms is NULL");
  if (h->timer_ends < 1) return fail(h, MT_ERR_STATE, "mt_timer_read without mt_timer_stop_async");
  MT_ON_DEVICE(h, h->cfg.device);
  float best = 0.f, v = 0.f;
  MT_HIP(h, hipEventSynchronize(h->ev1));
  MT_HIP(h, hipEventElapsedTime(&best, h->ev0, h->ev1));
  for (int c = 1; c < h->timer_ends; ++c) {
    if (!h->ev1c[c]) continue;
    MT_HIP(h, hipEventSynchronize(h->ev1c[c]));
    MT_HIP(h, hipEventElapsedTime(&v, h->ev0, h->ev1c[c]));
    best = v > best ? v : best;
  }
  if (h->timer_with_gather && h->ev_g1) {
    MT_HIP(h, hipEventSynchronize(h->ev_g1));
    if (hipEventElapsedTime(&v, h->ev0, h->ev_g1) == hipSuccess)
      best = v > best ? v : best;  // (an exchange that ended before the timer started reads negative: ignored)
    else
      (void)hipGetLastError();
  }
  *elapsed_ms = best;
  h->timer_ends = 0;
  return MT_OK;
}

// The lap pool holds at least `count` unused events.  Called at the BEGIN of a lap for the whole lap (its begin event and one
// end event per stream), ahead of the begin event's record: creating an event can stall the host for milliseconds (80 ms
// observed, once per process, inside the HIP runtime), and a host stall between a lap's last launch and the record of its
// end event would read as device time of the lap -- an event recorded on an idle stream completes at once.
static int lap_reserve(mt_handle h, size_t count) {
  while (h->lap_events.size() < h->lap_events_used + count) {
    hipEvent_t e = nullptr;
    MT_HIP(h, hipEventCreateWithFlags(&e, event_flags(true)));
    h->lap_events.push_back(e);
  }
  return MT_OK;
}

// one event of the lap pool, recorded on `stream`; its index
static int lap_event(mt_handle h, hipStream_t stream, uint32_t* index) {
  int rcr = lap_reserve(h, 1);
  if (rcr) return rcr;
  MT_HIP(h, hipEventRecord(h->lap_events[h->lap_events_used], stream));
  *index = (uint32_t)h->lap_events_used++;
  return MT_OK;
}

int mt_timer_lap_begin(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (h->lap_open) return fail(h, MT_ERR_STATE, "mt_timer_lap_begin: a lap is already open");
  // A lap starts behind everything queued before it.  While the chains are forked on the handle's own stream they stay
  // forked: one begin event per chain, the lap runs from the earliest of them to the latest end event (a join here would
  // put two cross-stream dependencies into the timed work for the sake of the stopwatch: 20 us per episode at 1 M arms).
  const bool per_chain = h->forked && h->lazy_chains && h->stream == h->own_stream;
  if (per_chain) {
    MT_ON_DEVICE(h, h->cfg.device);
    int rcf = flush_pending_reset(h);  // (per chain as well while forked)
    if (rcf) return rcf;
  } else {
    MT_ENTER_KEEP(h);  // (MT_F_GOALS stays as it is)
  }
  mt_engine::LapRec rec{0, 1, 0, 0};
  int rc = lap_reserve(h, 2 * (size_t)mt_engine::kMaxChains);  // the whole lap's events exist before it begins
  if (rc) return rc;
  rc = lap_event(h, h->stream, &rec.begin);
  if (rc) return rc;
  if (per_chain && h->forked)
    for (int c = 1; c < h->chains; ++c) {
      if (!h->chain_streams[c] || (int64_t)c * chain_span(h, h->chains) >= h->n) continue;
      uint32_t idx;
      rc = lap_event(h, h->chain_streams[c], &idx);  // consecutive indices: begin, begin + 1, ...
      if (rc) return rc;
      ++rec.n_begin;
    }
  h->lap_recs.push_back(rec);
  h->lap_open = true;
  return MT_OK;
}

int mt_timer_lap_end(mt_handle h) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  if (!h->lap_open) return fail(h, MT_ERR_STATE, "mt_timer_lap_end without mt_timer_lap_begin");
  MT_ON_DEVICE(h, h->cfg.device);  // NOT a join: while the chains are forked the lap ends when the last of them is done
  mt_engine::LapRec& rec = h->lap_recs.back();
  int rc = lap_event(h, h->stream, &rec.end0);
  if (rc) return rc;
  rec.n_end = 1;
  if (h->forked)
    for (int c = 1; c < h->chains; ++c) {
      if (!h->chain_streams[c] || (int64_t)c * chain_span(h, h->chains) >= h->n) continue;
      uint32_t idx;
      rc = lap_event(h, h->chain_streams[c], &idx);  // consecutive indices: end0, end0 + 1, ...
      if (rc) return rc;
      ++rec.n_end;
    }
  h->lap_open = false;
  return MT_OK;
}

// milliseconds of lap `rec`: from the earliest of its begin events to the latest of its end events
static int lap_ms(mt_handle h, const mt_engine::LapRec& rec, float* ms) {
  float best = 0.f;
  for (uint32_t k = 0; k < rec.n_end; ++k) {
    MT_HIP(h, hipEventSynchronize(h->lap_events[rec.end0 + k]));
    for (uint32_t b = 0; b < rec.n_begin; ++b) {
      float v = 0.f;
      MT_HIP(h, hipEventElapsedTime(&v, h->lap_events[rec.begin + b], h->lap_events[rec.end0 + k]));
      best = v > best ? v : best;
    }
  }
  *ms = best;
  return MT_OK;
}

int mt_timer_lap_times(mt_handle h, float* ms, int capacity, int* n_laps) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, n_laps != nullptr && (ms != nullptr || capacity == 0), "NULL argument");
  if (h->lap_open) return fail(h, MT_ERR_STATE, "mt_timer_lap_times: a lap is still open");
  const size_t laps = h->lap_recs.size();
  *n_laps = (int)laps;
  if ((size_t)capacity < laps) return fail(h, MT_ERR_INVALID_ARG, "mt_timer_lap_times: capacity is smaller than the number of laps");
  MT_ON_DEVICE(h, h->cfg.device);
  for (size_t i = 0; i < laps; ++i) {
    int rc = lap_ms(h, h->lap_recs[i], &ms[i]);
    if (rc) return rc;
  }
  h->lap_recs.clear();
  h->lap_events_used = 0;
  return MT_OK;
}

int mt_timer_laps_total(mt_handle h, float* total_ms, int* n_laps) {
  MT_REQUIRE(nullptr, h != nullptr, "handle is NULL");
  MT_REQUIRE(h, total_ms != nullptr, "total_ms is NULL");
  if (h->lap_open) return fail(h, MT_ERR_STATE, "mt_timer_laps_total: a lap is still open");
  MT_ON_DEVICE(h, h->cfg.device);
  double sum = 0.0;
  for (const auto& rec : h->lap_recs) {
    float v = 0.f;
    int rc = lap_ms(h, rec, &v);
    if (rc) return rc;
    sum += v;
  }
  *total_ms = (float)sum;
  if (n_laps) *n_laps = (int)h->lap_recs.size();
  h->lap_recs.clear();
  h->lap_events_used = 0;
  return MT_OK;
}

// ---- stateless helpers ------------------------------------------------------------------------
// They have no handle to keep buffers on, so the device scratch they need is cached per device and only ever
// grows; one lock serialises them (they are small synchronous calls on the null stream).
namespace {
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
};
std::mutex g_scratch_mu;
Scratch g_scratch[64];

int scratch_reserve(int device, size_t bytes, void** out) {  // g_scratch_mu held, `device` current
  if (device < 0 || device >= 64) return fail(nullptr, MT_ERR_INVALID_ARG, "device ordinal out of range");
  Scratch& sc = g_scratch[device];
  if (sc.bytes < bytes) {
    if (sc.p) (void)hipFree(sc.p);
    sc.p = nullptr;
    sc.bytes = 0;
    const size_t want = align_up(bytes, (size_t)1 << 16);
    if (hipMalloc(&sc.p, want) != hipSuccess) {
      (void)hipGetLastError();
      sc.p = nullptr;
      return fail(nullptr, MT_ERR_ALLOC, "hipMalloc of the helper scratch failed");
    }
    sc.bytes = want;
  }
  *out = sc.p;
  return MT_OK;
}
}  // namespace

int mt_fk_batch(int device, const float* dh_table, int dof, int mode, const float* angles, int angles_in_radians,
                int64_t n, float* out_mat16) {
  MT_REQUIRE(nullptr, dh_table && angles && out_mat16, "NULL argument");
  MT_REQUIRE(nullptr, dof >= 1 && dof <= MT_MAX_DOF && mode >= 0 && mode <= dof, "dof/mode out of range");
  MT_REQUIRE(nullptr, n >= 1, "n must be >= 1");
  MT_REQUIRE(nullptr, first_unusable(dh_table, (int64_t)dof * 4, kMaxFiniteBits) < 0 && first_unusable(angles, n * dof, kMaxFiniteBits) < 0,
             "mt_fk_batch: NaN or infinity in dh_table / angles");
  MT_ON_DEVICE(nullptr, device);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  const size_t in_b = align_up((size_t)n * dof * 4, 256);
  void* base = nullptr;
  int rc = scratch_reserve(device, in_b + (size_t)n * 64, &base);
  if (rc) return rc;
  float* d_in = (float*)base;
  float* d_out = (float*)((char*)base + in_b);
  FkArgs a{d_in, d_out, n, dof, mode, angles_in_radians, make_dh(dh_table, dof)};
  hipError_t e = hipMemcpy(d_in, angles, (size_t)n * dof * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fk_kernel, grid_for(n), dim3(kBlock), 0, 0, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_mat16, d_out, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (e != hipSuccess) rc = fail(nullptr, MT_ERR_HIP, std::string("mt_fk_batch: ") + hipGetErrorString(e));
  return rc;
}

int mt_route_trace(int device, const float* dh_table, int dof, int substeps, const float* prev, const float* action,
                   int64_t n, float* out) {
  MT_REQUIRE(nullptr, dh_table && prev && action && out, "NULL argument");
  MT_REQUIRE(nullptr, dof >= 2 && dof <= MT_MAX_DOF && substeps >= 2, "dof/substeps out of range");
  MT_REQUIRE(nullptr, n >= 1 && n * substeps < ((int64_t)1 << 31), "n out of range");
  MT_REQUIRE(nullptr, first_unusable(dh_table, (int64_t)dof * 4, kMaxFiniteBits) < 0 && first_unusable(prev, n * dof, kMaxFiniteBits) < 0 &&
                          first_unusable(action, n * dof, kMaxFiniteBits) < 0,
             "mt_route_trace: NaN or infinity in dh_table / prev / action");
  MT_ON_DEVICE(nullptr, device);
  const size_t in_b = align_up((size_t)n * dof * 4, 256), out_b = (size_t)n * substeps * dof * 3 * 4;
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  void* base = nullptr;
  int rc = scratch_reserve(device, 2 * in_b + out_b, &base);
  if (rc) return rc;
  char* d = (char*)base;
  TraceArgs a{(const float*)d, (const float*)(d + in_b), (float*)(d + 2 * in_b), n, dof, substeps, make_dh(dh_table, dof)};
  hipError_t e = hipMemcpy(d, prev, (size_t)n * dof * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + in_b, action, (size_t)n * dof * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(route_trace_kernel, grid_for(n * substeps), dim3(kBlock), 0, 0, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + 2 * in_b, out_b, hipMemcpyDeviceToHost);
  if (e != hipSuccess) rc = fail(nullptr, MT_ERR_HIP, std::string("mt_route_trace: ") + hipGetErrorString(e));
  return rc;
}

int mt_r_theta_batch(int device, const float* v1, const float* v2, int64_t n, float* out_r_theta) {
  MT_REQUIRE(nullptr, v1 && v2 && out_r_theta, "NULL argument");
  MT_REQUIRE(nullptr, n >= 1, "n must be >= 1");
  MT_REQUIRE(nullptr, first_unusable(v1, 3 * n, kMaxFiniteBits) < 0 && first_unusable(v2, 3 * n, kMaxFiniteBits) < 0,
             "mt_r_theta_batch: NaN or infinity in v1 / v2");
  MT_ON_DEVICE(nullptr, device);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  void* base = nullptr;
  int rc = scratch_reserve(device, (size_t)n * 8 * 4, &base);
  if (rc) return rc;
  float* d = (float*)base;
  float *d1 = d, *d2 = d + 3 * n, *dout = d + 6 * n;
  hipError_t e = hipMemcpy(d1, v1, (size_t)n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d2, v2, (size_t)n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(r_theta_kernel, grid_for(n), dim3(kBlock), 0, 0, d1, d2, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_r_theta, dout, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) rc = fail(nullptr, MT_ERR_HIP, std::string("mt_r_theta_batch: ") + hipGetErrorString(e));
  return rc;
}

// The streaming yardstick of the step's own access shape (kernels.h: stream_probe_kernel): `reps` passes over n_envs envs
// after 3 untimed ones, on a private stream, HIP events around them.  Allocates and frees its own buffers.
int mt_stream_probe(int device, int dof, int n_targets, int64_t n_envs, int reps, float* us_per_pass, int64_t* bytes_per_pass) {
  MT_REQUIRE(nullptr, us_per_pass != nullptr && bytes_per_pass != nullptr, "NULL argument");
  MT_REQUIRE(nullptr, n_envs >= 256 && n_envs <= ((int64_t)1 << 30) - 256 && reps >= 1 && reps <= 100000, "n_envs / reps out of range");
  const bool d4k7 = dof == 4 && n_targets == 7, d7k7 = dof == 7 && n_targets == 7, d4k10 = dof == 4 && n_targets == 10;
  if (!(d4k7 || d7k7 || d4k10))
    return fail(nullptr, MT_ERR_UNSUPPORTED, "mt_stream_probe: built for (dof, targets) = (4, 7), (7, 7), (4, 10)");
  MT_ON_DEVICE(nullptr, device);
  const int64_t ld = (int64_t)align_up((size_t)n_envs, 256) + 256;  // the arena's row pitch (mt_create)
  const int RD = dof + 3 * n_targets + 2, WN = 3 * n_targets + 4;
  float *state = nullptr, *out = nullptr;
  uint8_t* bytes = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipMalloc(&state, (size_t)RD * ld * 4);
  if (e == hipSuccess) e = hipMalloc(&out, (size_t)WN * ld * 4);
  if (e == hipSuccess) e = hipMalloc(&bytes, (size_t)ld);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipMemsetAsync(state, 0, (size_t)RD * ld * 4, st);
  float ms = 0.f;
  if (e == hipSuccess) {
    auto pass = [&]() {
      if (d4k7)
        hipLaunchKernelGGL((stream_probe_kernel<4, 7>), grid_for(n_envs), dim3(kBlock), 0, st, state, out, bytes, n_envs, ld);
      else if (d7k7)
        hipLaunchKernelGGL((stream_probe_kernel<7, 7>), grid_for(n_envs), dim3(kBlock), 0, st, state, out, bytes, n_envs, ld);
      else
        hipLaunchKernelGGL((stream_probe_kernel<4, 10>), grid_for(n_envs), dim3(kBlock), 0, st, state, out, bytes, n_envs, ld);
    };
    for (int w = 0; w < 3; ++w) pass();
    e = hipEventRecord(e0, st);
    for (int r = 0; r < reps; ++r) pass();
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (st) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  if (state) (void)hipFree(state);
  if (out) (void)hipFree(out);
  if (bytes) (void)hipFree(bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, e == hipErrorOutOfMemory ? MT_ERR_ALLOC : MT_ERR_HIP, std::string("mt_stream_probe: ") + hipGetErrorString(e));
  }
  *us_per_pass = ms * 1e3f / (float)reps;
  *bytes_per_pass = (int64_t)(8 * dof + 24 * n_targets + 33) * n_envs;
  return MT_OK;
}

}  // extern "C"
