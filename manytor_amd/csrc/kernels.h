// HIP kernels of the ManyTor step engine (gfx950, wave64).
//
// One thread = one environment.  State is struct-of-arrays with row stride
// `ld`, so every load/store below is a fully coalesced row access
// (lane l of a wave touches element 64*w + l of a row).
//
// Reference semantics restated here (file:line = /root/reference/manytor.py):
//   dh()               :25-32   one DH row = Rz(theta) Tz(d) Tx(a) Rx(alpha)
//   fk()               :35-53   product of the first `mode` rows, degrees in
//   get_observations() :141-153 from joints_coordinates[-2] (the elbow)
//   is_done()          :155-173 from joints_coordinates[-1] (the end effector)
//   action()           :175-213 25 interpolated sub-steps, ground flag, reward
//   step()             :255-260
//   reset()            :219-253
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mt_math.h"
#include "philox.h"
#include "step_args.h"

namespace mt {

// This header is included by more than one translation unit (engine.hip, actor_critic.hip: compiled side by side): every
// definition in it is a template, a forceinline function or an `inline` kernel.

// Write-only outputs of a step (observations, reward, done, end effector) are never re-read by the next
// step.  MT_NT_STORES marks them non-temporal so they do not displace the re-read state (goals, targets,
// alive mask, return) from L2 / Infinity Cache.
#ifndef MT_NT_STORES
#define MT_NT_STORES 1
#endif
// Row access: every SoA row is addressed as (wave-uniform row base) + (32-bit per-lane BYTE offset), which maps
// onto the `global_load/store v, v_off, s[base:base+1]` form -- the row base stays in SGPRs and no 64-bit
// per-lane address arithmetic is needed.  Byte offsets fit 32 bits because mt_create caps n_envs below 2^30.
// The row base MUST be the same in every lane.  It is passed through readfirstlane (free on a value that already
// sits in SGPRs): without that the optimiser folds `base + row * ld` and the lane offset into one per-lane 64-bit
// address per row and keeps all of them in VGPRs for the whole kernel (14 registers for 7 joint rows plus 64-bit
// VALU adds; measured: step_kernel<Dh7Table> 86 -> VGPRs, see profiles/r02_kernel_resources.txt).
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;  // a pointer known to be global memory: global_*, not flat_*

__device__ __forceinline__ global_ptr<char> uniform_row(const void* row) {
  const uint64_t v = reinterpret_cast<uint64_t>(row);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (global_ptr<char>)(((uint64_t)hi << 32) | lo);
}
// The lane offset has to reach instruction selection as a 32-BIT value in the basic block of the access: selection works
// per block, and an offset that was zero-extended once at the top and carried into other blocks as a 64-bit register can
// no longer be proven to fit the `saddr + zext(voffset)` form -- every access then costs a v_lshl_add_u64 and a 64-bit
// VGPR pair (96 of them in the prefetch kernel of the reference arm, 8 % of its instructions: round 3).  The empty asm
// "redefines" the offset in place before every access -- the SAME register, no instruction -- so the extension is
// re-materialised, and folded into the access, where it is used.  Hence the offset travels by reference: a kernel keeps
// ONE variable per element size (o4 = 4 i for the 32-bit rows, o1 = i for the byte rows) and every accessor renews it.
//   LaneOffset<true>  : renewed at every access (1 106 -> 1 013 VALU instructions in that kernel; 3-5 % less time where
//                       the step is latency- or issue-bound: <= 262 144 envs, the 7-joint arm, the fused episodes)
//   LaneOffset<false> : left to the optimiser (the 64-bit adds stay).  Where the reference arm's step is HBM-bound
//                       (>= ~400 k envs per launch) THIS form is the faster one by 0.7-2 % -- same memory operations in
//                       the same order, so the cause is the waves' timing against the memory system, not the code
//                       (profiles/r03_variants.md section 8) -- and step_kernel's FLAT instantiation keeps it.
#ifndef MT_PLAIN_LANE_OFFSET
#define MT_PLAIN_LANE_OFFSET 0  // 1: no renewal anywhere (A/B builds: tools/ab_lane_offset.sh)
#endif
template <bool RENEW>
struct LaneOffset {
  uint32_t v;
};
template <bool RENEW>
__device__ __forceinline__ uint32_t lane_offset(LaneOffset<RENEW>& o) {
#if !MT_PLAIN_LANE_OFFSET
  if (RENEW) asm volatile("" : "+v"(o.v));
#endif
  return o.v;
}
// MT_BUFFER_ROWS: the same access as a BUFFER instruction -- `buffer_load/store v, v_off, s[rsrc:rsrc+3], 0 offen`: the row
// base sits in a 128-bit resource descriptor in SGPRs (built by the scalar unit: base, no stride, no range check, the raw
// 32-bit data format of gfx94x / gfx950), the lane's byte offset is the VGPR operand by construction.  Neither the 64-bit
// per-lane adds of the plain form nor the renewal asm of the saddr form (a scheduling barrier at every access) are needed.
#ifndef MT_BUFFER_ROWS
#define MT_BUFFER_ROWS 0
#endif
#if MT_BUFFER_ROWS
constexpr int kRsrcWord3 = 0x00020000;  // raw buffer, DATA_FORMAT = 32 (gfx90a / gfx94x / gfx950)
constexpr int kAuxNt = 2;               // cache policy: non-temporal (the `nt` bit of gfx94x)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void* row) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)uniform_row(row), 0, -1, kRsrcWord3);  // num_records = 2^32 - 1: no clamp
}
template <typename T, bool R>
__device__ __forceinline__ T ldr(const T* row, LaneOffset<R>& o) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 1, "rows hold 32-bit words or bytes");
  if constexpr (sizeof(T) == 4)
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(row_rsrc(row), (int)o.v, 0, 0));
  else
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b8(row_rsrc(row), (int)o.v, 0, 0));
}
template <typename T, bool R>
__device__ __forceinline__ void str(T* row, LaneOffset<R>& o, T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 1, "rows hold 32-bit words or bytes");
  if constexpr (sizeof(T) == 4)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), row_rsrc(row), (int)o.v, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b8(__builtin_bit_cast(uint8_t, v), row_rsrc(row), (int)o.v, 0, 0);
}
template <typename T, bool R>
__device__ __forceinline__ void str_stream(T* row, LaneOffset<R>& o, T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 1, "rows hold 32-bit words or bytes");
  constexpr int aux = MT_NT_STORES ? kAuxNt : 0;
  if constexpr (sizeof(T) == 4)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), row_rsrc(row), (int)o.v, 0, aux);
  else
    __builtin_amdgcn_raw_buffer_store_b8(__builtin_bit_cast(uint8_t, v), row_rsrc(row), (int)o.v, 0, aux);
}
#else
template <typename T, bool R>
__device__ __forceinline__ T ldr(const T* row, LaneOffset<R>& o) {
  return *(global_ptr<const T>)(uniform_row(row) + lane_offset(o));
}
template <typename T, bool R>
__device__ __forceinline__ void str(T* row, LaneOffset<R>& o, T v) {
  *(global_ptr<T>)(uniform_row(row) + lane_offset(o)) = v;
}
template <typename T, bool R>
__device__ __forceinline__ void str_stream(T* row, LaneOffset<R>& o, T v) {
  global_ptr<T> p = (global_ptr<T>)(uniform_row(row) + lane_offset(o));
#if MT_NT_STORES
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}
#endif

// ---------------------------------------------------------------------------
// DH table views.  The chain code below is written once against this
// interface; `RtTable` reads the per-launch constants (SGPRs or LDS), the
// static tables are compile-time constants, so after unrolling every product
// with a 0 / +-1 entry disappears and the chain collapses to the arm's closed
// form (for the reference arm: z_elbow = d0 + d2 c1, z_ee = z_elbow +
// a3 (c1 s3' ... )).  The host picks a static table only
// when the configured table matches it exactly (engine.hip: match_static).
// ---------------------------------------------------------------------------
// Which rows of joints_coordinates the observation (manytor.py:143: [2]) and the pickup (:162: [3]) are measured from,
// and whose z the ground test looks at (:191: both).  The reference arm fixes them to the last two rows, and so do the
// tables below (kFrames == false: D - 2 and D - 1 at compile time).  RtTableF takes them from the launch constants
// (mt_config.obs_frame / ee_frame); row 0 is the all-zero origin row (manytor.py:189).
template <int D_>
struct RtTable {
  static constexpr int D = D_;
  static constexpr bool kFrames = false;
  const DhConst& c;
  __device__ __forceinline__ float a(int j) const { return c.a[j]; }
  __device__ __forceinline__ float d(int j) const { return c.d[j]; }
  __device__ __forceinline__ float sa(int j) const { return c.sa[j]; }
  __device__ __forceinline__ float ca(int j) const { return c.ca[j]; }
  __device__ __forceinline__ float off(int j) const { return c.off_deg[j]; }
};

template <int D_>
struct RtTableF {
  static constexpr int D = D_;
  static constexpr bool kFrames = true;
  const DhConst& c;
  __device__ __forceinline__ float a(int j) const { return c.a[j]; }
  __device__ __forceinline__ float d(int j) const { return c.d[j]; }
  __device__ __forceinline__ float sa(int j) const { return c.sa[j]; }
  __device__ __forceinline__ float ca(int j) const { return c.ca[j]; }
  __device__ __forceinline__ float off(int j) const { return c.off_deg[j]; }
  __device__ __forceinline__ int fo() const { return c.fo; }
  __device__ __forceinline__ int fe() const { return c.fe; }
};

#define MT_SEL8(j, v0, v1, v2, v3, v4, v5, v6, v7) \
  ((j) == 0 ? (v0) : (j) == 1 ? (v1) : (j) == 2 ? (v2) : (j) == 3 ? (v3) : (j) == 4 ? (v4) : (j) == 5 ? (v5) : (j) == 6 ? (v6) : (v7))

// The reference arm, manytor.py:42-48: rows (a, alpha, d, theta offset) =
// (0,-pi/2,4.3,0) (0,pi/2,0,0) (0,-pi/2,24.3,0) (27,pi/2,0,-pi/2).
struct Ref4Table {
  static constexpr int D = 4;
  static constexpr bool kFrames = false;
  __host__ __device__ static constexpr float a(int j) { return MT_SEL8(j, 0.f, 0.f, 0.f, 27.0f, 0.f, 0.f, 0.f, 0.f); }
  __host__ __device__ static constexpr float d(int j) { return MT_SEL8(j, 4.3f, 0.f, 24.3f, 0.f, 0.f, 0.f, 0.f, 0.f); }
  __host__ __device__ static constexpr float sa(int j) { return MT_SEL8(j, -1.f, 1.f, -1.f, 1.f, 0.f, 0.f, 0.f, 0.f); }
  __host__ __device__ static constexpr float ca(int j) { return MT_SEL8(j, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.f); }
  __host__ __device__ static constexpr float off(int j) { return MT_SEL8(j, 0.f, 0.f, 0.f, -90.f, 0.f, 0.f, 0.f, 0.f); }
};

// The 7-joint table of BASELINE.json configs[4] (manytor_amd/engine.py DH7_TABLE, fixture F7).
struct Dh7Table {
  static constexpr int D = 7;
  static constexpr bool kFrames = false;
  __host__ __device__ static constexpr float a(int j) { return MT_SEL8(j, 0.f, 0.f, 4.5f, -4.5f, 0.f, 8.8f, 0.f, 0.f); }
  __host__ __device__ static constexpr float d(int j) { return MT_SEL8(j, 34.0f, 0.f, 40.0f, 0.f, 40.0f, 0.f, 12.6f, 0.f); }
  __host__ __device__ static constexpr float sa(int j) { return MT_SEL8(j, -1.f, 1.f, 1.f, -1.f, -1.f, 1.f, 0.f, 0.f); }
  __host__ __device__ static constexpr float ca(int j) { return MT_SEL8(j, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f); }
  __host__ __device__ static constexpr float off(int j) { return MT_SEL8(j, 0.f, 0.f, 0.f, 0.f, 0.f, -90.f, 0.f, 0.f); }
};

// ---------------------------------------------------------------------------
// DH chain.  R = [X Y Z] (columns), p = origin.  One joint:
//   X' = X c + Y s ;  T = Y c - X s ;  Y' = T ca + Z sa ;  Z' = Z ca - T sa
//   p' = p + a X' + d Z
// which is R' = R * M(theta, alpha), p' = p + R * (a c, a s, d) for the matrix
// M of manytor.py:28-31.
// ---------------------------------------------------------------------------
template <class Tbl>
__device__ __forceinline__ void chain_all(const float (&s)[Tbl::D], const float (&c)[Tbl::D], const Tbl& t,
                                          float (&p)[Tbl::D][3]) {
  constexpr int D = Tbl::D;
  float X[3] = {1.f, 0.f, 0.f}, Y[3] = {0.f, 1.f, 0.f}, Z[3] = {0.f, 0.f, 1.f};
  float o[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float nx = pfma(X[q], c[j], pmul(Y[q], s[j]));
      const float tt = pfma(Y[q], c[j], -pmul(X[q], s[j]));
      o[q] = pfma(t.a(j), nx, pfma(t.d(j), Z[q], o[q]));
      X[q] = nx;
      Y[q] = pfma(tt, t.ca(j), pmul(Z[q], t.sa(j)));
      Z[q] = pfma(Z[q], t.ca(j), -pmul(tt, t.sa(j)));
      p[j][q] = o[q];
    }
  }
}

// z components only, of the frames after D-1 and after D joints: what the
// ground test of manytor.py:191 needs.  Joint 0's angle drops out (the z row of
// the identity is (0,0,1)), which the compiler sees after unrolling.
template <class Tbl>
__device__ __forceinline__ void chain_z(const float (&s)[Tbl::D], const float (&c)[Tbl::D], const Tbl& t, float& z_obs,
                                        float& z_ee) {
  constexpr int D = Tbl::D;
  float x = 0.f, y = 0.f, z = 1.f, o = 0.f;
  z_obs = 0.f;
  if constexpr (Tbl::kFrames) z_ee = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float nx = pfma(x, c[j], pmul(y, s[j]));
    const float tt = pfma(y, c[j], -pmul(x, s[j]));
    o = pfma(t.a(j), nx, pfma(t.d(j), z, o));
    x = nx;
    y = pfma(tt, t.ca(j), pmul(z, t.sa(j)));
    z = pfma(z, t.ca(j), -pmul(tt, t.sa(j)));
    if constexpr (Tbl::kFrames) {  // row 0 of joints_coordinates is the origin: z = 0 whatever joint 0 does
      if (j >= 1 && j == t.fo()) z_obs = o;
      if (j >= 1 && j == t.fe()) z_ee = o;
    } else {
      if (j == D - 2 && D > 2) z_obs = o;
    }
  }
  if constexpr (!Tbl::kFrames) z_ee = o;
}

// The observation frame and the pickup frame out of the chain's frame origins.
template <class Tbl>
__device__ __forceinline__ void pick_frames(const Tbl& t, const float (&p)[Tbl::D][3], float (&el)[3], float (&e)[3]) {
  constexpr int D = Tbl::D;
  if constexpr (Tbl::kFrames) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      el[q] = 0.f;
      e[q] = 0.f;
    }
#pragma unroll
    for (int j = 1; j < D; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        el[q] = (j == t.fo()) ? p[j][q] : el[q];
        e[q] = (j == t.fe()) ? p[j][q] : e[q];
      }
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      el[q] = (D > 2) ? p[D - 2][q] : 0.f;  // joints_coordinates[-2]; row 0 is zeros (manytor.py:189)
      e[q] = p[D - 1][q];
    }
  }
}

// One target: observation triple (manytor.py:150-152, :17-22) and pickup test
// (manytor.py:160-168).
__device__ __forceinline__ void observe_target(const float (&el)[3], float x, float y, float z, float& dist, float& r,
                                               float& th) {
  const float m0 = fabsf(el[0] - x), m1 = fabsf(el[1] - y), m2 = fabsf(el[2] - z);
  const float h2 = __builtin_fmaf(m0, m0, m1 * m1);
  const float h = __builtin_amdgcn_sqrtf(h2);            // v_sqrt_f32, 1 ulp: no refinement sequence
  dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(m2, m2, h2));
  r = atan2_deg_q1(m0, m1);
  th = atan2_deg_q1(h, m2);
}

__device__ __forceinline__ bool within_box(const float (&e)[3], float x, float y, float z, float tol) {
  return (fabsf(e[0] - x) <= tol) && (fabsf(e[1] - y) <= tol) && (fabsf(e[2] - z) <= tol);
}

// The alive mask of a fresh episode: bit k set for every target k < K (K <= 32).
__device__ __forceinline__ uint32_t all_alive_mask(int K) { return (K >= 32) ? 0xFFFFFFFFu : ((1u << K) - 1u); }

// A target's coordinates out of its three 21-bit Philox fields (philox.h candidate_fields): x = 2r u(fx) - r,
// y = 2r u(fy) - r, z = r u(fz).  Contraction is off so that every op rounds once, exactly as the numpy restatement
// (oracle/philox_ref.py) does.
__device__ __forceinline__ void target_coords(uint32_t fx, uint32_t fy, uint32_t fz, float radius, float& x, float& y, float& z) {
#pragma clang fp contract(off)
  const float r2 = 2.0f * radius;
  const float tx = r2 * u21(fx);
  const float ty = r2 * u21(fy);
  x = tx - radius;
  y = ty - radius;
  z = radius * u21(fz);
}

// Target code: the three fields in 63 bits of two words, lo = fx | fy << 21, hi = fy >> 11 | fz << 10 -- 8 bytes per
// target instead of 12.  Every target the library draws is such a triple, so decode_target gives back the float bits of
// the draw (it IS target_coords).  The dead target (0, 0, 0) is the code of (2^20, 2^20, 0) (2r * 1/2 - r = +0, r * 0 =
// +0), the draw's fallback point (0, 0, r / 2) that of (2^20, 2^20, 2^20).  Internal rows of the arena (StepArgs::codes,
// [2K][ld]), valid while the host knows them to match MT_F_POINTS (engine_internal.h: codes_valid).
struct TargetCode {
  uint32_t lo, hi;
};
__device__ __forceinline__ TargetCode encode_target(uint32_t fx, uint32_t fy, uint32_t fz) {
  return TargetCode{fx | (fy << 21), (fy >> 11) | (fz << 10)};
}
__device__ __forceinline__ void decode_target(TargetCode c, float radius, float& x, float& y, float& z) {
  target_coords(c.lo & 0x1FFFFFu, (c.lo >> 21) | ((c.hi & 0x3FFu) << 11), c.hi >> 10, radius, x, y, z);
}
constexpr uint32_t kHalfField = 1u << 20;  // u21 = 1/2
constexpr TargetCode kZeroTargetCode{kHalfField, kHalfField >> 11};
constexpr TargetCode kFallbackTargetCode{kHalfField, (kHalfField >> 11) | (kHalfField << 10)};

// One rejection-sampling candidate of manytor.py:229-239: half HALF of a Philox block (philox.h: two candidates
// per block), its coordinates and (if asked for) its code.
template <int HALF>
__device__ __forceinline__ bool target_candidate(const u32x4& w, float radius, float& x, float& y, float& z,
                                                 TargetCode* code = nullptr) {
#pragma clang fp contract(off)
  uint32_t fx, fy, fz;
  candidate_fields<HALF>(w, fx, fy, fz);
  if (code) *code = encode_target(fx, fy, fz);
  const float rr = radius * radius;
  target_coords(fx, fy, fz, radius, x, y, z);
  const float xx = x * x, yy = y * y, zz = z * z;
  const float sxy = xx + yy;
  const float n2 = sxy + zz;
  return n2 <= rr;
}

// A code parked in a float LDS stage (draw_targets_wave, reset_split_kernel): its two words, `stride` floats apart.
__device__ __forceinline__ TargetCode staged_code(const float* cell, int stride) {
  return TargetCode{__float_as_uint(cell[0]), __float_as_uint(cell[stride])};
}

// One target inside step(): obs2 triple (taken before the pickup, manytor.py:204), pickup test
// (manytor.py:206), and the zeroing of a target that died earlier (manytor.py:148) -- with CODES its code as well.
template <bool ABLATE_OBS, bool CODES = false, bool R>
__device__ __forceinline__ void step_target(const StepArgs& a, int64_t ld, LaneOffset<R>& o4, int k, uint32_t am, uint32_t& nam,
                                            const float (&el)[3], const float (&e)[3], float x, float y, float z) {
  const bool al = (am >> k) & 1u;
  float dist = 0.f, r = 0.f, th = 0.f;
  if (al) {
    if (ABLATE_OBS) {
      dist = x + el[0];
      r = y + el[1];
      th = z + el[2];
    } else {
      observe_target(el, x, y, z, dist, r, th);
    }
    if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << k);
  } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {
    float* row = a.points + (int64_t)(3 * k) * ld;
    str(row, o4, 0.f);
    str(row + ld, o4, 0.f);
    str(row + 2 * ld, o4, 0.f);
    if (CODES) {
      uint32_t* crow = a.codes + (int64_t)(2 * k) * ld;
      str(crow, o4, kZeroTargetCode.lo);
      str(crow + ld, o4, kZeroTargetCode.hi);
    }
  }
  float* orow = a.obs + (int64_t)(3 * k) * ld;
  str_stream(orow, o4, dist);
  str_stream(orow + ld, o4, r);
  str_stream(orow + 2 * ld, o4, th);
}

// ---------------------------------------------------------------------------
// step: Environment.step() for all envs (manytor.py:255-260 + :175-213).
//   Tbl    : RtTable<D> (any table, constants per launch) or a static table
//   SAMPLE : draw the action in-kernel (== sample_actions_kernel then step)
//   TRIG   : how sin/cos of the S-2 interior sub-step poses are obtained
//            0 angle-addition recurrence: the poses are g + k*delta, so
//              (c,s)_{k+1} = (c,s)_k rotated by delta -- 4 FMA-class ops per joint
//              instead of a sincos.  Run forward from the previous pose (k = 0,
//              exact) and backward from the action (k = S-1, exact) to the middle,
//              which halves the drift (<= 12 rotations, < 1e-4 in z, inside the
//              1e-3 guard band of the ground flag) and gives two independent
//              dependency chains per iteration.
//            1 polynomial sincos at every sub-step (reference-shaped, slowest)
//            2 hardware v_sin_f32/v_cos_f32 at every interior sub-step
//            3, 4 DIAGNOSTIC ablations for profiling (MT_FLAG_ABLATE_*): outputs wrong
//   LDS    : stage the runtime DH constants in LDS instead of SGPRs (measured
//            variant; BASELINE.json's north_star asks for the comparison)
// The first and last pose are always evaluated with the polynomial sincos.
// ---------------------------------------------------------------------------
template <class Tbl>
struct TableMaker {
  static __device__ __forceinline__ Tbl make(const DhConst&) { return Tbl{}; }
};
template <int D>
struct TableMaker<RtTable<D>> {
  static __device__ __forceinline__ RtTable<D> make(const DhConst& c) { return RtTable<D>{c}; }
};
template <int D>
struct TableMaker<RtTableF<D>> {
  static __device__ __forceinline__ RtTableF<D> make(const DhConst& c) { return RtTableF<D>{c}; }
};

// The step index that keys this launch's action draw (see StepArgs::major_base; the address is wave-uniform: s_load).
__device__ __forceinline__ uint32_t step_index(const StepArgs& a) {
  return a.major_base ? a.major + *a.major_base : a.major;
}

// Environment.action_sample for one env (manytor.py:215-217): D integer degrees from one Philox block.
template <int D>
__device__ __forceinline__ void draw_action(uint64_t seed, uint64_t env_id, uint32_t step_idx, float (&act)[D]) {
  static_assert(D <= 8, "one Philox block yields at most 8 joint angles");
  const u32x4 w = stream_block(seed, env_id, kTagAction, step_idx, 0u);
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int j = 0; j < D; ++j) act[j] = (j < 4) ? action_from_word(ws[j]) : action_from_word_digit1(ws[j - 4]);
}

// The kinematic part of Environment.action (manytor.py:178-192) for one env: S poses on the straight line in
// joint space from `g` (previous pose) to `act`.  Returns the elbow and end-effector positions at the final pose
// and the minimum z of those two frames over all S poses (ground flag <=> zmin < 0).  Shared by step_kernel and
// rollout_kernel so both evaluate exactly the same arithmetic.
// Joints whose angle can influence the z of the last two frames (what chain_z computes).  Joint 0 never does (handled
// by the callers: index 0 is skipped everywhere); the LAST joint does only through a(D-1) * X'.z, so for a static
// table whose last row has a = 0 (the 7-joint table: a pure d offset along the previous z) its sine / cosine are never
// needed at the interior sub-steps.  The compiler does not discover this by itself (the rotation is a loop-carried
// cycle): 6 of 57 instructions of the 7-joint sub-step loop.
template <class Tbl>
struct ZJoints {
  static constexpr int value = (Tbl::a(Tbl::D - 1) == 0.f) ? Tbl::D - 1 : Tbl::D;
};
template <int D>
struct ZJoints<RtTable<D>> {
  static constexpr int value = D;
};
template <int D>
struct ZJoints<RtTableF<D>> {
  static constexpr int value = D;
};

// rotate (s, c) of joints 1..JN-1 by +delta (SIGN = +1) or -delta (SIGN = -1): the angle-addition step of the recurrence
template <int D, int JN, int SIGN>
__device__ __forceinline__ void rotate_pose(float (&s)[D], float (&c)[D], const float (&sd)[D], const float (&cd)[D]) {
#pragma unroll
  for (int j = 1; j < JN; ++j) {
    const float c2 = __builtin_fmaf(c[j], cd[j], SIGN > 0 ? -(s[j] * sd[j]) : s[j] * sd[j]);
    s[j] = __builtin_fmaf(s[j], cd[j], SIGN > 0 ? c[j] * sd[j] : -(c[j] * sd[j]));
    c[j] = c2;
  }
}

// sin / cos of the per-sub-step increment.  It is small (|delta| <= 15 degrees for sampled actions at S = 25): when
// every lane of the wave has |delta| <= 45 the quadrant reduction is skipped.  Both paths give identical bits for
// such angles (sincos_deg reduces with q = 0), so a lane's result does not depend on its wave-mates.
template <int D, int JN>
__device__ __forceinline__ void sincos_increment(const float (&st)[D], float (&sd)[D], float (&cd)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    sd[j] = 0.f;
    cd[j] = 1.f;
  }
  bool small = true;
#pragma unroll
  for (int j = 1; j < JN; ++j) small &= fabsf(st[j]) <= 45.0f;
  if (__all(small)) {
#pragma unroll
    for (int j = 1; j < JN; ++j) sincos_deg_small(st[j], sd[j], cd[j]);
  } else {
#pragma unroll
    for (int j = 1; j < JN; ++j) sincos_deg(st[j], sd[j], cd[j]);
  }
}

// Sines / cosines of a SAMPLED action (rollout kernels).  draw_action yields integer degrees in [-180, 180), and the
// joint offsets of the compile-time tables are whole degrees in [-90, 0], so action + offset is one of the 450
// integers -270 .. 179: the block fills an LDS table with sincos_deg of exactly those floats once per launch and every
// step looks its D pairs up instead of evaluating D range reductions and polynomials (~30 instructions each, 8-11 %
// of a rollout step).  Same function on the same float => the same bits as computing it in place.
constexpr int kTrigBias = 270;
constexpr int kTrigEntries = 450;
struct SinCos {
  float s, c;
};
template <class Tbl>
struct ActionTrigTable {
  static constexpr bool value = false;
};
template <>
struct ActionTrigTable<Ref4Table> {
  static constexpr bool value = true;
};
template <>
struct ActionTrigTable<Dh7Table> {
  static constexpr bool value = true;
};
template <class Tbl>
constexpr bool whole_degree_offsets() {
  for (int j = 0; j < Tbl::D; ++j) {
    const float o = Tbl::off(j);
    if (o != (float)(int)o || o < -90.f || o > 0.f) return false;
  }
  return true;
}
// The table itself: sincos_deg of exactly the floats -270 .. 179, computed ONCE per handle by this kernel (mt_create) into
// the arena.  Every block that wants it copies the 3 600 bytes into LDS (one 16-byte load per thread from L2, instead
// of two range reductions + polynomials per thread and launch): the load is issued first, the write and the barrier
// come after whatever the kernel can do in between (its pose loads, the Philox block).
constexpr int kTrigVec4 = kTrigEntries * 2 / 4;  // the table as float4s
static_assert(kTrigEntries * 2 % 4 == 0 && kTrigVec4 <= kBlock, "one float4 per thread stages the table");
inline __global__ __launch_bounds__(kBlock) void fill_trig_table_kernel(float* table) {
  for (int idx = threadIdx.x; idx < kTrigEntries; idx += kBlock) {
    float sv, cv;
    sincos_deg((float)(idx - kTrigBias), sv, cv);
    table[2 * idx] = sv;
    table[2 * idx + 1] = cv;
  }
}
__device__ __forceinline__ float4 trig_table_load(const float* table) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (threadIdx.x < kTrigVec4) v = reinterpret_cast<const float4*>(table)[threadIdx.x];
  return v;
}
// every wave of the block executes this exactly once (the barrier counts arrivals, wherever the s_barrier sits)
// Values that must be COMPLETE, in the instruction stream too, before the next barrier / wait: the compiler is free to sink
// pure arithmetic below a __syncthreads(), and it does so with the whole Philox block of the step kernels -- which then runs
// AFTER the wait for the table load, i.e. after (nearly) every load of the kernel had come back (vmcnt counts in issue
// order, and the conditional prefetch loads make the count conservative), instead of under their latency.
template <int D>
__device__ __forceinline__ void complete_before_here(float (&v)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) asm volatile("" : "+v"(v[j]));
}
__device__ __forceinline__ void trig_table_commit(SinCos* lds, const float4& v) {
  if (threadIdx.x < kTrigVec4) reinterpret_cast<float4*>(lds)[threadIdx.x] = v;
  __syncthreads();
}
template <class Tbl, bool TABLE>
__device__ __forceinline__ void action_sincos(const Tbl& t, const float (&act)[Tbl::D], float (&sv)[Tbl::D],
                                              float (&cv)[Tbl::D], const SinCos* trig) {
#pragma unroll
  for (int j = 0; j < Tbl::D; ++j) {
    if constexpr (TABLE) {
      static_assert(whole_degree_offsets<Tbl>(), "the table covers whole-degree offsets in [-90, 0] only");
      const SinCos v = trig[(int)act[j] + ((int)Tbl::off(j) + kTrigBias)];
      sv[j] = v.s;
      cv[j] = v.c;
    } else {
      sincos_deg(act[j] + t.off(j), sv[j], cv[j]);
    }
  }
}

// The kinematic part of Environment.action (manytor.py:178-192) for one env: S poses on the straight line in
// joint space from `g` (previous pose) to `act`.  Returns the elbow and end-effector positions at the final pose
// and the minimum z of those two frames over all S poses (ground flag <=> zmin < 0).  Shared by step_kernel and
// rollout_kernel so both evaluate exactly the same arithmetic.
//
// Two schedules of the recurrence (TRIG == 0), same poses, same arithmetic per pose, hence the same bits (min is
// order-free):
//   interleaved (D <= 5): forward and backward half advance in the same loop iteration -- two independent
//     dependency chains, and 56 VGPRs for the reference arm;
//   sequential (D >= 6): forward half first, then the action's sincos, the full chain and the backward half.  The two
//     halves never hold their (s, c) state at the same time: 4 (D - 1) fewer live registers, which is what takes the
//     7-joint kernel from 97 VGPRs (4 waves/SIMD) to <= 64 (8 waves/SIMD).
//
// PoseCache (rollout_kernel only): inside a rollout the pose a step starts from is the action of the step before, whose
// sines / cosines and frame heights were computed then.  Handing them over saves the k = 0 pose's sincos and z chain
// (JN - 1 sincos + one chain_z per step, 6 % of the instructions for the reference arm).  Same inputs to the same
// functions, so the bits do not change; when any lane of the wave has no valid cache (first step of a launch, right
// after an in-kernel re-arm) the whole wave simply recomputes.
template <int D>
struct PoseCache {
  float s[D], c[D];  // joints 1 .. JN-1 of the pose the next step starts from
  float zmin;        // min z of its last two frames
};

// sines / cosines of joints 1 .. JN-1 at the pose a step starts from: out of the whole-degree table when the host
// knows every angle of the batch to be a whole degree in [-180, 180) (kFlagWholeGoals, wave-uniform), else computed.
// The table holds sincos_deg of the very float g + off, so both ways give the same bits.
template <class Tbl, bool TABLE>
__device__ __forceinline__ void prev_pose_sincos(const Tbl& t, const float (&g)[Tbl::D], float (&sF)[Tbl::D],
                                                 float (&cF)[Tbl::D], const SinCos* trig, bool whole) {
  constexpr int JN = ZJoints<Tbl>::value;
  if constexpr (TABLE) {
    if (whole) {
#pragma unroll
      for (int j = 1; j < JN; ++j) {
        const SinCos v = trig[(int)g[j] + ((int)Tbl::off(j) + kTrigBias)];
        sF[j] = v.s;
        cF[j] = v.c;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 1; j < JN; ++j) sincos_deg(g[j] + t.off(j), sF[j], cF[j]);
}

template <class Tbl, int TRIG, bool CACHED, bool TABLE>
__device__ __forceinline__ float route_kinematics_narrow(const Tbl& t, int S, float inv_sm1, const float (&g)[Tbl::D],
                                                         const float (&act)[Tbl::D], float (&el)[3], float (&e)[3],
                                                         PoseCache<Tbl::D>* cache, bool cache_valid, const SinCos* trig,
                                                         bool prev_whole) {
  constexpr int D = Tbl::D;
  constexpr int JN = ZJoints<Tbl>::value;
  constexpr bool kSequential = (TRIG == 0 || TRIG == 5) && D >= 6;
  const bool use_cache = CACHED && __all(cache_valid);
  // route[k] = goals + k * (action - goals) / (S-1), route[S-1] = action (np.linspace, manytor.py:182)
  float st[D];
#pragma unroll
  for (int j = 0; j < D; ++j) st[j] = (act[j] - g[j]) * inv_sm1;

  float zmin, zo, ze;
  if (kSequential) {
    const int nf = (S - 1) / 2;   // forward poses k = 1..nf
    const int nb = S - 2 - nf;    // backward poses k = S-2..nf+1   (nb = nf or nf-1)
    float sd[D], cd[D];
    sincos_increment<D, JN>(st, sd, cd);
    {  // k = 0 (the previous pose, manytor.py:182-192 evaluates it again) and the forward half
      float sF[D], cF[D];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        sF[j] = 0.f;
        cF[j] = 1.f;
      }
      if (use_cache) {
#pragma unroll
        for (int j = 1; j < JN; ++j) {
          sF[j] = cache->s[j];
          cF[j] = cache->c[j];
        }
        zmin = cache->zmin;
      } else {
        prev_pose_sincos<Tbl, TABLE>(t, g, sF, cF, trig, prev_whole);
        chain_z<Tbl>(sF, cF, t, zo, ze);
        zmin = fminf(zo, ze);
      }
#pragma unroll 2
      for (int it = 1; it <= nf; ++it) {
        rotate_pose<D, JN, +1>(sF, cF, sd, cd);
        chain_z<Tbl>(sF, cF, t, zo, ze);
        zmin = fminf(zmin, fminf(zo, ze));
      }
    }
    // k = S-1: the action itself, full chain (positions are consumed by the caller), then the backward half
    float sB[D], cB[D], p[D][3];
    action_sincos<Tbl, TABLE>(t, act, sB, cB, trig);
    chain_all<Tbl>(sB, cB, t, p);
    pick_frames<Tbl>(t, p, el, e);
    zmin = fminf(zmin, fminf(el[2], e[2]));
    if (CACHED) {
#pragma unroll
      for (int j = 1; j < JN; ++j) {
        cache->s[j] = sB[j];
        cache->c[j] = cB[j];
      }
      cache->zmin = fminf(el[2], e[2]);
    }
    sB[0] = 0.f;
    cB[0] = 1.f;
#pragma unroll 2
    for (int it = 1; it <= nb; ++it) {
      rotate_pose<D, JN, -1>(sB, cB, sd, cd);
      chain_z<Tbl>(sB, cB, t, zo, ze);
      zmin = fminf(zmin, fminf(zo, ze));
    }
    return zmin;
  }

  // k = S-1: the action itself, full chain (positions are consumed by the caller)
  float sA[D], cA[D], p[D][3];
  action_sincos<Tbl, TABLE>(t, act, sA, cA, trig);
  chain_all<Tbl>(sA, cA, t, p);
  pick_frames<Tbl>(t, p, el, e);
  zmin = fminf(el[2], e[2]);

  // k = 0: the previous pose (manytor.py:182-192 evaluates it again: a pose left below ground costs -1 twice)
  float sF[D], cF[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    sF[j] = 0.f;
    cF[j] = 1.f;
  }
  if (use_cache) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      sF[j] = cache->s[j];
      cF[j] = cache->c[j];
    }
    zmin = fminf(zmin, cache->zmin);
  } else {
    prev_pose_sincos<Tbl, TABLE>(t, g, sF, cF, trig, prev_whole);
    chain_z<Tbl>(sF, cF, t, zo, ze);
    zmin = fminf(zmin, fminf(zo, ze));
  }
  if (CACHED) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      cache->s[j] = sA[j];
      cache->c[j] = cA[j];
    }
    cache->zmin = fminf(el[2], e[2]);
  }

  if (TRIG == 3 || TRIG == 4) {
    // diagnostic builds: no interior sub-steps
  } else if (TRIG == 0 || TRIG == 5) {
    float sd[D], cd[D];
    sincos_increment<D, JN>(st, sd, cd);
    float sB[D], cB[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      sB[j] = sA[j];
      cB[j] = cA[j];
    }
    sB[0] = 0.f;
    cB[0] = 1.f;
    const int nf = (S - 1) / 2;   // forward poses k = 1..nf
    const int nb = S - 2 - nf;    // backward poses k = S-2..nf+1   (nb = nf or nf-1)
    // both halves advance together for nb iterations (no condition inside the loop: the two chains' registers stay where
    // they are), then the forward half's extra pose when the number of interior poses is odd
#pragma unroll 2
    for (int it = 1; it <= nb; ++it) {
      rotate_pose<D, JN, +1>(sF, cF, sd, cd);
      chain_z<Tbl>(sF, cF, t, zo, ze);
      zmin = fminf(zmin, fminf(zo, ze));
      rotate_pose<D, JN, -1>(sB, cB, sd, cd);
      chain_z<Tbl>(sB, cB, t, zo, ze);
      zmin = fminf(zmin, fminf(zo, ze));
    }
    if (nf > nb) {
      rotate_pose<D, JN, +1>(sF, cF, sd, cd);
      chain_z<Tbl>(sF, cF, t, zo, ze);
      zmin = fminf(zmin, fminf(zo, ze));
    }
  } else {
    float gq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) gq[j] = g[j] + t.off(j);
    for (int k = 1; k < S - 1; ++k) {
      const float fk = (float)k;
#pragma unroll
      for (int j = 1; j < JN; ++j) {
        const float pose = __builtin_fmaf(fk, st[j], gq[j]);
        if (TRIG == 2)
          sincos_deg_hw(pose, sF[j], cF[j]);
        else
          sincos_deg(pose, sF[j], cF[j]);
      }
      chain_z<Tbl>(sF, cF, t, zo, ze);
      zmin = fminf(zmin, fminf(zo, ze));
    }
  }
  return zmin;
}

// ---------------------------------------------------------------------------
// Routes with an end beyond +-180 degrees (mt_math.h: wide_angle).  Staged actions, and the poses they leave behind,
// are accepted up to +-32 768 degrees, where the fp32 increment (act - g) / (S - 1), the sums g + k * increment and
// g + offset all round by more than the position tolerance.  Such a route is evaluated pose by pose from angles formed
// in double and reduced modulo 360 there (sincos_deg_route): S sincos per joint instead of the recurrence, no drift,
// the per-pose accuracy of a route inside +-180.  An end within +-180 keeps its fp32 sum (sincos_deg_off), so the final
// pose -- elbow, end effector, observations, the PoseCache handed to the next step -- has the bits of the narrow form
// whenever the ACTION is narrow, wherever the route started.
//
// Cold by construction: `any joint of g or act wide` is tested per lane and the branch is taken per WAVE (__any), so a
// wave without such a lane executes the narrow form alone, unchanged, and the two forms never share registers: a
// batch within +-180 gets the bits and the kernel the resources it had.  A wave WITH such a lane takes this form as a
// whole.  Its narrow lanes lose nothing (their ends are the narrow form's bits, their interior poses have no recurrence
// drift), but their z-minimum is then this form's, not the recurrence's: within the same 1e-4 of the reference, so
// the ground flag can differ from a narrow wave's only inside the guard band.
// ---------------------------------------------------------------------------
// The test itself is on the hot path of every step, so it is kept to what can be wide at all: not the pose while the
// host knows the whole batch to sit on whole degrees in [-180, 180) (kFlagWholeGoals, a launch constant: the steps of a
// sampled rollout test one scalar flag), not an action out of the whole-degree table (TABLE: drawn in-kernel, always in
// [-180, 180)).  The rest is one running maximum of magnitudes (v_max3_f32 with |.| modifiers) and one compare.
template <class Tbl, bool TABLE>
__device__ __forceinline__ bool wide_route(const float (&g)[Tbl::D], const float (&act)[Tbl::D], bool prev_whole) {
  float reach = 0.f;
  if (!prev_whole) {
#pragma unroll
    for (int j = 0; j < Tbl::D; ++j) reach = fmaxf(reach, __builtin_fabsf(g[j]));
  }
  if (!TABLE) {
#pragma unroll
    for (int j = 0; j < Tbl::D; ++j) reach = fmaxf(reach, __builtin_fabsf(act[j]));
  }
  return wide_angle(reach);
}

template <class Tbl, bool CACHED>
__device__ __forceinline__ float route_kinematics_wide(const Tbl& t, int S, const float (&g)[Tbl::D],
                                                       const float (&act)[Tbl::D], float (&el)[3], float (&e)[3],
                                                       PoseCache<Tbl::D>* cache) {
  constexpr int D = Tbl::D;
  constexpr int JN = ZJoints<Tbl>::value;
  float s[D], c[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {  // chain_z reads joints 1 .. JN-1 only
    s[j] = 0.f;
    c[j] = 1.f;
  }
  // k = 0 (the previous pose, evaluated again: manytor.py:182-192) .. S-2.  The action's pose comes last, as in the
  // sequential schedule of the narrow form: what it leaves behind (el, e, the cache) is not held across the loop.
  float zmin = 0.f;
  const double inv = 1.0 / (double)(S - 1);
  for (int k = 0; k < S - 1; ++k) {
    const double frac = (double)k * inv;
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      // (opaque copies: the conversions to double are redone per pose instead of being kept, two doubles per joint, across
      // the loop -- this form has to fit the register budget the narrow form sets for the kernel)
      float gj = g[j], aj = act[j];
      asm volatile("" : "+v"(gj), "+v"(aj));
      sincos_deg_route(gj, aj, frac, t.off(j), s[j], c[j]);
    }
    float zo, ze;
    chain_z<Tbl>(s, c, t, zo, ze);
    zmin = (k == 0) ? fminf(zo, ze) : fminf(zmin, fminf(zo, ze));
  }
  // k = S-1: the action itself, full chain
  float p[D][3];
#pragma unroll
  for (int j = 0; j < D; ++j) sincos_deg_off(act[j], t.off(j), s[j], c[j]);
  chain_all<Tbl>(s, c, t, p);
  pick_frames<Tbl>(t, p, el, e);
  if (CACHED) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      cache->s[j] = s[j];
      cache->c[j] = c[j];
    }
    cache->zmin = fminf(el[2], e[2]);
  }
  zmin = fminf(zmin, fminf(el[2], e[2]));
  return zmin;
}

template <class Tbl, int TRIG, bool CACHED = false, bool TABLE = false>
__device__ __forceinline__ float route_kinematics(const Tbl& t, int S, float inv_sm1, const float (&g)[Tbl::D],
                                                  const float (&act)[Tbl::D], float (&el)[3], float (&e)[3],
                                                  PoseCache<Tbl::D>* cache = nullptr, bool cache_valid = false,
                                                  const SinCos* trig = nullptr, bool prev_whole = false) {
  if constexpr (TRIG <= 2) {  // (3, 4, 5: diagnostic builds, timing only)
    if (__builtin_expect(__any(wide_route<Tbl, TABLE>(g, act, prev_whole)), 0))
      return route_kinematics_wide<Tbl, CACHED>(t, S, g, act, el, e, cache);
  }
  return route_kinematics_narrow<Tbl, TRIG, CACHED, TABLE>(t, S, inv_sm1, g, act, el, e, cache, cache_valid, trig, prev_whole);
}

// ---------------------------------------------------------------------------
// The ground test of a block, with the interior poses run on dense lanes (step_kernel<.., GC>).
//
// The interior poses of a route yield one bit, zmin < 0, and both END poses are evaluated anyway (the action's for the
// elbow and the end effector, the previous one because manytor.py:182-192 evaluates it again).  Where an end pose already
// has a frame below ground the bit is decided and the S - 2 interior poses cannot change any output: 78 % of the env-steps
// of a random rollout of the reference arm.  The undecided envs are spread evenly over the lanes (14 of a wave's 64 on
// average), so no wave can skip the loop by itself; a block can: its undecided lanes park what the recurrence needs --
// per joint 1 .. JN-1 the start (s, c), the end (s, c) and the increment (sd, cd) -- in an LDS queue, and after a barrier
// the queued routes are dealt out as HALF routes (the forward half from the previous pose, the backward half from the
// action: independent chains, the unit route_kinematics_split_narrow walks) to the first 2 Q lanes of the block, rotated by
// blockIdx.x so that the working waves of the blocks resident on a CU fall on different SIMDs.  A working lane runs
// rotate_pose / chain_z on the owner's values in the owner's order and leaves the half's minimum in LDS; after a second
// barrier the owner combines the two halves with its end poses.  The same arithmetic on the same inputs in another lane
// (-(s * -sd) == s * sd exactly, min is order-free), so zmin < 0 is the same bit for every env.
//
// The queue holds kCap routes.  An undecided lane that finds it full (the first step of an episode leaves 47 % undecided,
// staged actions can leave a whole block) walks its own two halves in place, like route_kinematics_narrow: any number of
// undecided envs, 0 .. 256, is handled without rounds.  Waves with a wide route (route_kinematics_wide) evaluate all
// poses themselves, queue nothing, and lend their lanes to the block's queue like every other wave.
// Every thread of the block must reach both barriers: lanes past the end of the batch come along as decided lanes.
// ---------------------------------------------------------------------------
template <class Tbl>
struct GroundQueue {
  static constexpr int kJoints = ZJoints<Tbl>::value - 1;  // the joints chain_z reads
  static constexpr int kFields = 6 * kJoints;              // start (s, c), end (s, c), increment (sd, cd) per joint
  // routes per block: at most kBlock / 2 (one half route per lane), fewer for long arms (<= 14 KB of LDS, whole waves)
  static constexpr int kCap = (14336 / (4 * kFields) >= kBlock / 2) ? kBlock / 2 : (14336 / (4 * kFields)) / 32 * 32;
  static_assert(kCap >= 32 && 2 * kCap <= kBlock, "one half route per lane");
  uint32_t count;             // undecided lanes of the block so far (may exceed kCap: the rest walk their own routes)
  float zres[2 * kCap];       // [2 r + half] minimum z over the interior poses of that half of route r
  float field[kFields][kCap]; // field-major: the lanes of a wave write / read consecutive words
};

// min z over this half's interior poses: `n_half` rotations from (s, c) by (sd, cd), of which the first `mine` count (the
// halves differ by at most one pose; the loop bound stays uniform).  3e38 when the half has no pose.
template <class Tbl>
__device__ __forceinline__ float half_route_zmin(const Tbl& t, float (&s)[Tbl::D], float (&c)[Tbl::D], const float (&sd)[Tbl::D],
                                                 const float (&cd)[Tbl::D], int n_half, int mine) {
  constexpr int D = Tbl::D;
  constexpr int JN = ZJoints<Tbl>::value;
  float zm = 3.0e38f, zo, ze;
#pragma unroll 2
  for (int it = 1; it <= n_half; ++it) {
    rotate_pose<D, JN, +1>(s, c, sd, cd);
    chain_z<Tbl>(s, c, t, zo, ze);
    if (it <= mine) zm = fminf(zm, fminf(zo, ze));
  }
  return zm;
}

struct NoGroundQueue {  // what a kernel without the queue declares in its place: never referenced, no LDS
  uint32_t count;
};
__device__ __forceinline__ void ground_queue_reset(uint32_t* count) {  // ahead of a barrier that every thread reaches
  if (threadIdx.x == 0) *count = 0u;
}

// route_kinematics for the recurrence (TRIG == 0) of a whole block; `live` = this lane has an env.  Called by every
// thread of the block, after a barrier behind ground_queue_reset.
template <class Tbl, bool TABLE>
__device__ __forceinline__ float route_kinematics_block(const Tbl& t, int S, float inv_sm1, const float (&g)[Tbl::D],
                                                        const float (&act)[Tbl::D], float (&el)[3], float (&e)[3],
                                                        const SinCos* trig, bool prev_whole, bool live, GroundQueue<Tbl>& q) {
  constexpr int D = Tbl::D;
  constexpr int JN = ZJoints<Tbl>::value;
  constexpr int kCap = GroundQueue<Tbl>::kCap;
  const int nf = (S - 1) / 2;   // forward poses k = 1..nf
  const int nb = S - 2 - nf;    // backward poses k = S-2..nf+1   (nb = nf or nf-1)
  float zmin;
  bool undecided = false;
  float sF[D], cF[D], sA[D], cA[D], sd[D], cd[D];
  if (__builtin_expect(__any(live && wide_route<Tbl, TABLE>(g, act, prev_whole)), 0)) {
    zmin = route_kinematics_wide<Tbl, false>(t, S, g, act, el, e, nullptr);
  } else {
    // the two end poses, as route_kinematics_narrow evaluates them
    float st[D];
#pragma unroll
    for (int j = 0; j < D; ++j) st[j] = (act[j] - g[j]) * inv_sm1;
    float p[D][3], zo, ze;
    action_sincos<Tbl, TABLE>(t, act, sA, cA, trig);
    chain_all<Tbl>(sA, cA, t, p);
    pick_frames<Tbl>(t, p, el, e);
    zmin = fminf(el[2], e[2]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      sF[j] = 0.f;
      cF[j] = 1.f;
    }
    prev_pose_sincos<Tbl, TABLE>(t, g, sF, cF, trig, prev_whole);
    chain_z<Tbl>(sF, cF, t, zo, ze);
    zmin = fminf(zmin, fminf(zo, ze));
    sincos_increment<D, JN>(st, sd, cd);
    sA[0] = 0.f;
    cA[0] = 1.f;
    undecided = live && !(zmin < 0.f);
  }

  // a place in the block's queue for every undecided lane: one LDS atomic per wave
  const unsigned long long um = __ballot(undecided);
  uint32_t slot = kCap;
  if (um != 0ull) {
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(&q.count, (uint32_t)__popcll(um));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(um >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)um, 0u));
  }
  const bool queued = undecided && slot < (uint32_t)kCap;
  if (queued) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      float(*f)[kCap] = q.field + 6 * (j - 1);
      f[0][slot] = sF[j];
      f[1][slot] = cF[j];
      f[2][slot] = sA[j];
      f[3][slot] = cA[j];
      f[4][slot] = sd[j];
      f[5][slot] = cd[j];
    }
  }
  if (undecided && !queued) {  // the queue was full: this lane's own two halves (ahead of the barrier: nothing of it stays live across the queue's work)
    zmin = fminf(zmin, half_route_zmin<Tbl>(t, sF, cF, sd, cd, nf, nf));
#pragma unroll
    for (int j = 1; j < JN; ++j) sd[j] = -sd[j];
    zmin = fminf(zmin, half_route_zmin<Tbl>(t, sA, cA, sd, cd, nf, nb));
  }
  __syncthreads();  // the queue is complete

  const uint32_t routes = q.count < (uint32_t)kCap ? q.count : (uint32_t)kCap;
  const uint32_t w = (threadIdx.x + 64u * (blockIdx.x & 3u)) & (uint32_t)(kBlock - 1);  // this lane's half route
  if (w < 2u * routes) {
    const uint32_t r = w >> 1;
    const bool backward = (w & 1u) != 0u;
    float sW[D], cW[D], sdW[D], cdW[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      sW[j] = 0.f;
      cW[j] = 1.f;
      sdW[j] = 0.f;
      cdW[j] = 1.f;
    }
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      const float(*f)[kCap] = q.field + 6 * (j - 1);
      sW[j] = backward ? f[2][r] : f[0][r];
      cW[j] = backward ? f[3][r] : f[1][r];
      const float sdj = f[4][r];
      sdW[j] = backward ? -sdj : sdj;  // rotate by -delta: the sign rides in the operand
      cdW[j] = f[5][r];
    }
    q.zres[w] = half_route_zmin<Tbl>(t, sW, cW, sdW, cdW, nf, backward ? nb : nf);
  }
  __syncthreads();  // the halves' minima are in place
  if (queued) zmin = fminf(zmin, fminf(q.zres[2u * slot], q.zres[2u * slot + 1u]));
  return zmin;
}

// An env finished its episode `episode` with return `ret` and is being re-armed: keep the return in the ring
// (slot = number of episodes it finished before, modulo the ring size) and in the one-slot last_return row.
__device__ __forceinline__ void record_finished(const StepArgs& a, uint32_t i, uint32_t episode, float ret) {
  LaneOffset<true> o4{i * 4u};
  str(a.last_return, o4, ret);
  if (a.ring_slots)  // the slot differs from lane to lane: plain per-lane addressing, not a uniform row
    a.ring[(int64_t)((episode - a.episode0) % a.ring_slots) * a.ld + i] = ret;
}

// In-kernel phase stamps (cdna_hip_programming.md section 7): only in the diagnostic build of
// tools/microbench/step_stamps.hip (-DMT_STAMPS); in the library the macro is empty and no stamp executes.
#ifdef MT_STAMPS
#define MT_STAMP(a, i, slot)                                                                 \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    unsigned long long t__;                                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");              \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    if ((a).stamps && (threadIdx.x & 63) == 0) (a).stamps[(size_t)((i) >> 6) * 8 + (slot)] = t__; \
  } while (0)
#else
#define MT_STAMP(a, i, slot) \
  do {                       \
  } while (0)
#endif

// Staged actions come from outside (a policy, a host array): anything that is not a finite angle of at most
// 2^15 degrees in magnitude -- NaN, +-inf, garbage -- would poison `goals` for good.  Tested on the bit pattern,
// so the check survives -ffinite-math-only.
__device__ __forceinline__ bool unusable_angle(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) > 0x47000000u; }

// Asking for 8 waves per SIMD (= 64 VGPRs) only where the default recurrence kernel is within reach of it: the
// 7-joint table lands on 68 without the request and fits 64 with it, no scratch (profiles/r02_kernel_resources.txt).
template <class Tbl, int TRIG>
constexpr int step_min_waves() { return (TRIG == 0 && Tbl::D >= 6 && Tbl::D <= 7) ? 8 : 1; }

//   PF     : number of targets whose coordinates are requested at the very top, ahead of the kinematics (0 or
//            kPrefetch).  In-kernel stamps (tools/microbench/step_stamps.hip) show that with few waves per SIMD the
//            target loop is a chain of exposed load latencies -- 55 % of a wave's lifetime at 65 536 arms -- which the
//            ~3700 cycles of kinematics hide completely if the loads are already in flight.  Costs 3 * PF registers,
//            so the host uses it where occupancy is not the limit (small batches); same arithmetic, same bits.
//            (Staging the same rows through LDS-DMA -- global_load_lds_dword into a [3K][256] tile, no VGPRs -- was
//            measured and is slower at every batch size: profiles/r02_variants.md section 5.)
constexpr int kPrefetch = 8;

//   TT     : sampled actions are whole degrees, and so is the pose they leave behind: with a compile-time table (whole-
//            degree joint offsets) the sines / cosines of BOTH end poses of the route come out of the 450-entry
//            whole-degree table (fill_trig_table_kernel), staged into LDS per block, instead of 2 (JN - 1) + 1 range
//            reductions and polynomials per env: 1 277 -> 1 153 instructions per wave for the reference arm, 1.5-6 % time
//            (most where an env is spread over lanes and the end poses are replicated; profiles/r03_variants.md section 3).
//            Whole batch or a 256-aligned range of it only (threads past the end run up to the barrier: their loads stay
//            inside the rows, which are ld >= round_up(n, 256) long); same bits as the computed values.
//   FLAT   : the rows are addressed through LaneOffset<false> (see there): the HBM-bound launches of the prefetch kernel.
__device__ __forceinline__ void draw_targets_wave(uint64_t seed, uint64_t env0, uint32_t episode, bool need, int K, float radius,
                                                  float* col0, uint8_t* slots);

//   FRESH  : the launch BEGINS with the full random reset mt_reset_random deferred to it (the chained launch-per-step form of
//            mt_rollout, engine.hip): instead of loading pose / alive mask / return / targets the kernel keeps the finished
//            return (MT_F_LAST_RETURN), starts from the zero pose with every target alive, stores the episode index, draws
//            the targets with reset_kernel's wave-cooperative draw into LDS columns and writes them out -- reset_kernel's
//            state, bit for bit, without its launch, without its stores of what this step overwrites anyway (pose, alive
//            mask, return, end effector, reward, done: 41 B per env) and without this step's loads of what it would have
//            written (108 B per env).  Dynamic LDS: [2K][kBlock] target codes.
//   CODES  : the targets are read as their 8-byte codes (StepArgs::codes, kernels.h TargetCode) instead of the 12 bytes of
//            their floats: 56 instead of 84 B per env at K = 7, of the 233 a step moves.  Only while the host knows the codes
//            to match MT_F_POINTS (engine_internal.h: codes_valid); a dead target's code is zeroed with its floats.
//   PREV   : where the pose the step starts from comes from.  A sampled step stores goals = its action, one Philox block of
//            (seed, env, step); a full reset leaves the zero pose.  While the host knows the row to be one of the two
//            (engine_internal.h: GoalsRow) the launch re-derives it -- kPrevDraw: draw_action of step - 1, issued where the load
//            was, ahead of the action draw, so that the two Philox states are never live together; kPrevZero: as FRESH -- and
//            the 4 D bytes per env stay in HBM.  The goals STORE stays: every visible field keeps its bits.  Both poses are whole
//            degrees by construction (kFlagWholeGoals).
enum : int { kPrevLoad = 0, kPrevZero = 1, kPrevDraw = 2 };
template <class Tbl, bool SAMPLE, int TRIG, bool LDS, int PF = 0, bool TT = false, bool FLAT = false, bool FRESH = false,
          bool CODES = false, bool GC = false, int PREV = kPrevLoad>
__global__ __launch_bounds__(kBlock, (PF ? 1 : step_min_waves<Tbl, TRIG>())) void step_kernel(const StepArgs a) {
  constexpr int D = Tbl::D;
  static_assert(PREV == kPrevLoad || CODES, "the previous pose is re-derived by the code-reading kernels (the HBM-bound launches)");
  static_assert(!GC || (TRIG == 0 && !LDS && !FRESH), "the block-cooperative ground test serves the recurrence");
  static_assert(!TT || (SAMPLE && TRIG == 0 && !LDS && ActionTrigTable<Tbl>::value), "the table serves sampled actions of a static table");
  static_assert(!FRESH || TT, "the reset prologue exists for the sampled-action kernels of the static tables");
  static_assert(!CODES || (PF && TT && !FRESH), "codes are read by the prefetch kernels of the static tables");
  extern __shared__ float fresh_stage[];                          // FRESH: the drawn target codes, [2K][kBlock]
  __shared__ uint8_t fresh_slots[FRESH ? kBlock / 64 : 1][64];    // FRESH: draw_targets_wave's scratch
  __shared__ DhConst sh;
  __shared__ __attribute__((aligned(16))) SinCos trig_lds[TT ? kTrigEntries : 1];
  __shared__ std::conditional_t<GC, GroundQueue<Tbl>, NoGroundQueue> ground_q;  // (the queue's type exists for GC kernels only)
  float4 trig_v;
  if (TT) trig_v = trig_table_load(a.trig_table);
  if constexpr (GC) {
    ground_queue_reset(&ground_q.count);
    if (!TT) __syncthreads();  // (TT: the barrier of trig_table_commit below)
  }
  if (LDS) {
    const float* src = reinterpret_cast<const float*>(&a.dh);
    float* dst = reinterpret_cast<float*>(&sh);
    if (threadIdx.x < sizeof(DhConst) / sizeof(float)) dst[threadIdx.x] = src[threadIdx.x];
    __syncthreads();
  }
  const Tbl t = TableMaker<Tbl>::make(LDS ? sh : a.dh);

  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  LaneOffset<!FLAT> o4{i * 4u}, o1{i};  // byte offsets of this lane in the 32-bit rows / the byte rows
  // (TT, and with it FRESH: every thread stays up to the barrier / takes part in the draw; GC: up to the ground test's
  // barriers, as a lane without an env -- its loads stay inside the rows, it stores nothing)
  const bool live = i < a.n;
  if (!TT && !GC && !live) return;
  const int64_t ld = a.ld;
  // Read ahead of every row access: behind one (its lane offset renewal is an opaque asm to the memory analysis) the
  // word is no longer provably unclobbered, and the s_load turns into a vector load with an s_waitcnt vmcnt(0) behind
  // it -- which also waits for every prefetched row (measured: +2 % per step at 1 M envs under graph replay).
  const uint32_t step_no = SAMPLE ? step_index(a) : 0u;

  // Long arms (D >= 6) are register-bound: their kernel keeps nothing alive across the sub-step loops that it can
  // fetch or store on the other side of them (alive mask and return loaded after, new goals stored before).
  constexpr bool kLean = D >= 6;
  MT_STAMP(a, i, 0);
  float g[D], act[D];
  if constexpr (PREV == kPrevDraw) {
    draw_action<D>(((uint64_t)a.seed_hi << 32) | a.seed_lo, (uint64_t)(a.env_base + i), step_no - 1u, g);
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = (FRESH || PREV == kPrevZero) ? 0.f : ldr(a.goals + j * ld, o4);
  }
  float tx[PF ? PF : 1][3];
  uint32_t tc[CODES ? PF : 1][2];
  if constexpr (FRESH) {
    const bool mine = i < a.n;
    const uint32_t lane = threadIdx.x & 63u;
    if (mine) {
      str(a.last_return, o4, ldr(a.total_reward, o4));  // what reset_kernel<.., RANDOM, false> keeps of the episode that ends here
      str(a.episodes, o4, a.reset_episode);
    }
    draw_targets_wave(((uint64_t)a.reset_seed_hi << 32) | a.reset_seed_lo, (uint64_t)(a.env_base + (i - lane)), a.reset_episode, mine,
                      a.K, a.radius, fresh_stage + (threadIdx.x - lane), fresh_slots[threadIdx.x >> 6]);
    if (mine) {
      const float* col = fresh_stage + threadIdx.x;
#pragma unroll
      for (int k = 0; k < (PF ? PF : 0); ++k)
        if (k < a.K) {
          decode_target(staged_code(col + 2 * k * kBlock, kBlock), a.radius, tx[k][0], tx[k][1], tx[k][2]);
#pragma unroll
          for (int q = 0; q < 3; ++q) str(a.points + (int64_t)(3 * k + q) * ld, o4, tx[k][q]);
        }
      for (int k = PF; k < a.K; ++k) {
        float x, y, z;
        decode_target(staged_code(col + 2 * k * kBlock, kBlock), a.radius, x, y, z);
        const int64_t r = 3 * k;
        str(a.points + r * ld, o4, x);
        str(a.points + (r + 1) * ld, o4, y);
        str(a.points + (r + 2) * ld, o4, z);
      }
    }
  } else if (PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (k < a.K) {
        // (Loads under a condition make every later s_waitcnt vmcnt(N) conservative -- the compiler can only count the loads
        // certainly issued behind the one it waits for -- so the kinematics starts once nearly all prefetched rows are back.
        // Unconditional loads, the last row again for the slots past K, give exact counts and were measured: +2 % at
        // 98 304-131 072 envs, nothing elsewhere: profiles/r03_ab_unconditional_prefetch.txt.)
        if constexpr (CODES) {
          const uint32_t* crow = a.codes + (int64_t)(2 * k) * ld;
          tc[k][0] = ldr(crow, o4);
          tc[k][1] = ldr(crow + ld, o4);
        } else {
          const float* row = a.points + (int64_t)(3 * k) * ld;
#pragma unroll
          for (int q = 0; q < 3; ++q) tx[k][q] = ldr(row + q * ld, o4);
        }
      }
  }
  // The alive mask and the return are requested now, ahead of the arithmetic that does not need them.
  // (Requesting the target rows here as well was measured: no gain, -2 waves/SIMD -- profiles/r01_variants.md.)
  uint32_t am = 0;
  float total_in = 0.f;
  if (FRESH) {
    am = all_alive_mask(a.K);
  } else if (!kLean || PF) {
    am = ldr(a.alive, o4);
    total_in = ldr(a.total_reward, o4);
  }
  if (SAMPLE) {
    // not stored separately: the action taken becomes `goals` below (manytor.py:184), 4D bytes of traffic saved
    draw_action<D>(((uint64_t)a.seed_hi << 32) | a.seed_lo, (uint64_t)(a.env_base + i), step_no, act);
  } else {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      act[j] = ldr(a.actions + j * ld, o4);
      bad |= unusable_angle(act[j]);
    }
    if (bad) {  // the env holds its pose this step; the call is counted (mt_bad_action_count)
#pragma unroll
      for (int j = 0; j < D; ++j) act[j] = g[j];
      if (!GC || live) atomicAdd(a.bad_actions, 1u);
    }
  }
  if constexpr (GC) {  // a lane without an env: whatever the rows hold past the batch stays out of the arithmetic
#pragma unroll
    for (int j = 0; j < D; ++j) {
      g[j] = live ? g[j] : 0.f;
      if (!SAMPLE) act[j] = live ? act[j] : 0.f;
    }
  }
  MT_STAMP(a, i, 1);  // action known (Philox done / staged action loaded)
  if (TT) {
    // (complete_before_here(act) -- the Philox block ahead of this wait -- was measured here: nothing at >= 262 144 envs,
    // +1 % at 131 072; the lane-split kernels gain 1-2 % and have it: profiles/r03_ab_philox_before_wait.txt)
    trig_table_commit(trig_lds, trig_v);  // the table load has had the pose loads to arrive
    if (!GC && !live) return;
  }
  if (kLean && (!GC || live)) {  // goals = action (manytor.py:184): the old pose is in registers already
#pragma unroll
    for (int j = 0; j < D; ++j) str(a.goals + j * ld, o4, act[j]);
  }

  float el[3], e[3];
  float zmin;
  const bool prev_whole = PREV != kPrevLoad || (a.flags & kFlagWholeGoals) != 0;
  if constexpr (GC) {
    zmin = route_kinematics_block<Tbl, TT>(t, a.S, a.inv_sm1, g, act, el, e, trig_lds, prev_whole, live, ground_q);
    if (!live) return;  // behind the last barrier
  } else {
    zmin = route_kinematics<Tbl, TRIG, false, TT>(t, a.S, a.inv_sm1, g, act, el, e, nullptr, false, trig_lds, prev_whole);
  }
  const bool ground = zmin < 0.f;  // manytor.py:191
  if (a.zmin) str_stream(a.zmin, o4, zmin);  // MT_FLAG_DEBUG_ZMIN: wave-uniform branch on an SGPR pointer, NULL by default
  if (kLean && !PF && !FRESH) {
    am = ldr(a.alive, o4);
    total_in = ldr(a.total_reward, o4);
  }
  MT_STAMP(a, i, 2);  // kinematics done (this waits for the pose loads)

  // obs2 (before pickup, manytor.py:204) and pickup (manytor.py:206) per target
  uint32_t nam = am;
  if (PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k)
      if (k < a.K) {
        if constexpr (CODES) decode_target(TargetCode{tc[k][0], tc[k][1]}, a.radius, tx[k][0], tx[k][1], tx[k][2]);
        step_target<false, CODES>(a, ld, o4, k, am, nam, el, e, tx[k][0], tx[k][1], tx[k][2]);
      }
  }
  for (int k = PF; k < a.K; ++k) {
    if (TRIG == 5) {  // DIAGNOSTIC: arithmetic only, no HBM traffic for targets / observations
      float dist, r, th;
      const float x = (float)(i & 63) + (float)k, y = 3.0f + (float)k, z = 5.0f + g[0];
      observe_target(el, x, y, z, dist, r, th);
      if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << k);
      if (dist + r + th == -12345.0f) (a.obs + (int64_t)(3 * k) * ld)[i] = dist;
      continue;
    }
    if constexpr (CODES) {
      const uint32_t* crow = a.codes + (int64_t)(2 * k) * ld;
      float x, y, z;
      decode_target(TargetCode{ldr(crow, o4), ldr(crow + ld, o4)}, a.radius, x, y, z);
      step_target<false, true>(a, ld, o4, k, am, nam, el, e, x, y, z);
      continue;
    }
    const float* row = a.points + (int64_t)(3 * k) * ld;
    {
      const float x = ldr(row, o4), y = ldr(row + ld, o4), z = ldr(row + 2 * ld, o4);
      step_target<TRIG == 4>(a, ld, o4, k, am, nam, el, e, x, y, z);
    }
  }

  MT_STAMP(a, i, 3);  // target loop done
  const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);  // manytor.py:205-212
  bool done = (nam == 0u);                                    // manytor.py:170-171
  if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;

  if (!kLean) {
#pragma unroll
    for (int j = 0; j < D; ++j) str(a.goals + j * ld, o4, act[j]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) str_stream(a.ee + q * ld, o4, e[q]);
  str(a.alive, o4, nam);
  str_stream(a.reward, o4, rew);
  str(a.total_reward, o4, total_in + (float)rew);  // manytor.py:258
  if (a.snap) str(a.snap, o4, total_in + (float)rew);  // (wave-uniform branch on an SGPR pointer, like a.zmin)
  str_stream(a.done, o1, (uint8_t)(done ? 1 : 0));
  const unsigned long long bits = __ballot(done);
  if ((threadIdx.x & 63) == 0) a.done_bits[i >> 6] = bits;
  MT_STAMP(a, i, 4);  // all stores issued
#ifdef MT_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  MT_STAMP(a, i, 5);  // all stores acknowledged
#endif
}

// route_kinematics for an env that is spread over L lanes (step_split_kernel, rollout_split_kernel): the same S poses,
// each with the arithmetic of route_kinematics, but a sub-lane walks only ONE half of the recurrence -- the forward half
// from the previous pose (backward == false) or the backward half from the action -- in a loop body that is the same
// for both (the start state and the sign of sin(delta) ride in registers), and the running min of z is combined over
// the env's sub-lanes at the end (lane = q * (64 / L) + e, so the partners sit 64 / L, 2 * 64 / L ... lanes apart).
// Every sub-lane computes the endpoint sincos and the full chain at the final pose itself (it needs elbow and end
// effector for its targets).  -(s * -sd) == s * sd exactly and min is order-free => the bits of route_kinematics.
template <class Tbl, int L, bool CACHED, bool TABLE>
__device__ __forceinline__ float route_kinematics_split_narrow(const Tbl& t, int S, float inv_sm1, const float (&g)[Tbl::D],
                                                               const float (&act)[Tbl::D], bool backward, float (&el)[3],
                                                               float (&e)[3], PoseCache<Tbl::D>* cache, bool cache_valid,
                                                               const SinCos* trig, bool prev_whole) {
  constexpr int D = Tbl::D;
  constexpr int JN = ZJoints<Tbl>::value;
  constexpr int EPW = 64 / L;
  const bool use_cache = CACHED && __all(cache_valid);
  float st[D];
#pragma unroll
  for (int j = 0; j < D; ++j) st[j] = (act[j] - g[j]) * inv_sm1;
  float sA[D], cA[D], p3[D][3];
  action_sincos<Tbl, TABLE>(t, act, sA, cA, trig);
  chain_all<Tbl>(sA, cA, t, p3);
  pick_frames<Tbl>(t, p3, el, e);
  float sF[D], cF[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    sF[j] = 0.f;
    cF[j] = 1.f;
  }
  float zo, ze, z0;
  if (use_cache) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      sF[j] = cache->s[j];
      cF[j] = cache->c[j];
    }
    z0 = cache->zmin;
  } else {
    prev_pose_sincos<Tbl, TABLE>(t, g, sF, cF, trig, prev_whole);
    chain_z<Tbl>(sF, cF, t, zo, ze);
    z0 = fminf(zo, ze);
  }
  if (CACHED) {
#pragma unroll
    for (int j = 1; j < JN; ++j) {
      cache->s[j] = sA[j];
      cache->c[j] = cA[j];
    }
    cache->zmin = fminf(el[2], e[2]);
  }
  // start state and first z of this sub-lane's half: k = 0 (previous pose) forward, k = S - 1 (the action) backward
  float zmin = backward ? fminf(el[2], e[2]) : z0;
  float sd[D], cd[D];
  sincos_increment<D, JN>(st, sd, cd);
  float sW[D], cW[D];
  sW[0] = 0.f;
  cW[0] = 1.f;
#pragma unroll
  for (int j = 1; j < D; ++j) {
    sW[j] = backward ? sA[j] : sF[j];
    cW[j] = backward ? cA[j] : cF[j];
    sd[j] = backward ? -sd[j] : sd[j];                         // rotate by -delta: the sign rides in the operand
  }
  const int nf = (S - 1) / 2;                                  // forward poses k = 1..nf
  const int nb = S - 2 - nf;                                   // backward poses k = S-2..nf+1 (nb = nf or nf - 1)
  const int mine = backward ? nb : nf;
#pragma unroll 2
  for (int it = 1; it <= nf; ++it) {
    rotate_pose<D, JN, +1>(sW, cW, sd, cd);
    chain_z<Tbl>(sW, cW, t, zo, ze);
    if (it <= mine) zmin = fminf(zmin, fminf(zo, ze));
  }
#pragma unroll
  for (int sh = EPW; sh < 64; sh <<= 1) zmin = fminf(zmin, __shfl_xor(zmin, sh));
  return zmin;
}

// A wave with a wide route (see route_kinematics_wide): every sub-lane of an env walks all S poses itself -- the sub-lanes
// hold the same pose and action, so they agree on the result, and there is nothing to combine.
template <class Tbl, int L, bool CACHED, bool TABLE = false>
__device__ __forceinline__ float route_kinematics_split(const Tbl& t, int S, float inv_sm1, const float (&g)[Tbl::D],
                                                        const float (&act)[Tbl::D], bool backward, float (&el)[3],
                                                        float (&e)[3], PoseCache<Tbl::D>* cache = nullptr,
                                                        bool cache_valid = false, const SinCos* trig = nullptr,
                                                        bool prev_whole = false) {
  if (__builtin_expect(__any(wide_route<Tbl, TABLE>(g, act, prev_whole)), 0))
    return route_kinematics_wide<Tbl, CACHED>(t, S, g, act, el, e, cache);
  return route_kinematics_split_narrow<Tbl, L, CACHED, TABLE>(t, S, inv_sm1, g, act, backward, el, e, cache, cache_valid, trig,
                                                              prev_whole);
}

// ---------------------------------------------------------------------------
// step, one env spread over L lanes of a wave (L = 2 or 4) -- for batches so small that the chip is mostly idle and a
// launch's time is one wave's dependent chain plus the kernel boundary (profiles/r02_variants.md section 3).
//   lane layout   : lane = q * (64 / L) + e;  e = env within the wave (64 / L envs per wave), q = its sub-lane
//   kinematics    : sub-lanes with even q walk the forward half of the recurrence (from the previous pose), odd q the
//                   backward half (from the action) -- the SAME loop body, the sign of sin(delta) and the start state
//                   differ per lane, so there is no divergence; every pose keeps the arithmetic of route_kinematics
//                   (-(s * -sd) == s * sd exactly), and min over the halves is order-free => bit-identical results
//   targets       : sub-lane q handles targets q, q + L, q + 2L, ...; the cleared alive bits are AND-ed over the
//                   sub-lanes, the running min of z is min-ed (ds_bpermute via __shfl_xor)
//   replicated    : the Philox draw, the endpoint sincos and the full chain at the final pose (every sub-lane needs the
//                   elbow and the end effector for its targets)
//   stores        : each sub-lane its targets' observations; sub-lane 0 the env's state and step outputs
// Only the default trigonometry (TRIG 0); D, the table kinds and both action sources as in step_kernel.
// ---------------------------------------------------------------------------
template <class Tbl, bool SAMPLE, int L, bool TT = false>
__global__ __launch_bounds__(kBlock) void step_split_kernel(const StepArgs a) {
  static_assert(L == 2 || L == 4, "an env is spread over 2 or 4 lanes");
  static_assert(!TT || (SAMPLE && ActionTrigTable<Tbl>::value), "the table serves sampled actions of a static table");
  constexpr int D = Tbl::D;
  constexpr int EPW = 64 / L;                                  // envs per wave
  constexpr int PFS = (kPrefetch + L - 1) / L;                 // targets per sub-lane requested up front
  __shared__ __attribute__((aligned(16))) SinCos trig_lds[TT ? kTrigEntries : 1];   // as in step_kernel<.., TT>
  float4 trig_v;
  if (TT) trig_v = trig_table_load(a.trig_table);
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t q = lane / EPW;
  const int64_t first = (int64_t)wave * EPW;                   // first env of this wave
  if (first >= a.n) {                                          // whole wave beyond the batch
    if (TT) trig_table_commit(trig_lds, trig_v);               // its arrival at the block's barrier, and its quarter of the table
    return;
  }
  const uint32_t env = (uint32_t)first + lane % EPW;
  const bool live = env < a.n;                                 // tail lanes compute on the last env and store nothing
  const uint32_t i = live ? env : (uint32_t)(a.n - 1);
  const int64_t ld = a.ld;

  float g[D], act[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = (a.goals + j * ld)[i];
  // this sub-lane's first targets, ahead of the arithmetic (target index p = q + L * m)
  float tx[PFS][3];
#pragma unroll
  for (int m = 0; m < PFS; ++m) {
    const int p = (int)q + L * m;
    if (p < a.K) {
      const float* row = a.points + (int64_t)(3 * p) * ld;
#pragma unroll
      for (int c = 0; c < 3; ++c) tx[m][c] = (row + c * ld)[i];
    }
  }
  const uint32_t am = a.alive[i];
  const float total_in = a.total_reward[i];
  if (SAMPLE) {
    draw_action<D>(((uint64_t)a.seed_hi << 32) | a.seed_lo, (uint64_t)(a.env_base + i), step_index(a), act);
  } else {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      act[j] = (a.actions + j * ld)[i];
      bad |= unusable_angle(act[j]);
    }
    if (bad) {
#pragma unroll
      for (int j = 0; j < D; ++j) act[j] = g[j];
      if (live && q == 0) atomicAdd(a.bad_actions, 1u);
    }
  }

  if (TT) {
    complete_before_here(act);  // Philox under the loads' latency: 32 768 arms 4.76 -> 4.68 us per step, 65 536: 5.84 -> 5.77
    trig_table_commit(trig_lds, trig_v);
  }

  // ---- kinematics: the poses of route_kinematics, one half per sub-lane parity ------------------------------
  float el[3], e[3];
  const float zmin = route_kinematics_split<Tbl, L, false, TT>(t, a.S, a.inv_sm1, g, act, (q & 1u) != 0, el, e, nullptr, false,
                                                                trig_lds, (a.flags & kFlagWholeGoals) != 0);
  const bool ground = zmin < 0.f;  // manytor.py:191
  if (a.zmin && live && q == 0) __builtin_nontemporal_store(zmin, a.zmin + i);  // MT_FLAG_DEBUG_ZMIN

  // ---- this sub-lane's targets ------------------------------------------------------------------------------
  uint32_t nam = am;
  for (int m = 0; (int)q + L * m < a.K; ++m) {
    const int p = (int)q + L * m;
    float* row = a.points + (int64_t)(3 * p) * ld;
    float x, y, z;
    bool have = false;
#pragma unroll
    for (int mm = 0; mm < PFS; ++mm)
      if (m == mm) {
        x = tx[mm][0];
        y = tx[mm][1];
        z = tx[mm][2];
        have = true;
      }
    if (!have) {
      x = row[i];
      y = (row + ld)[i];
      z = (row + 2 * ld)[i];
    }
    const bool al = (am >> p) & 1u;
    float dist = 0.f, r = 0.f, th = 0.f;
    if (al) {
      observe_target(el, x, y, z, dist, r, th);
      if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << p);
    } else if (live && ((x != 0.f) | (y != 0.f) | (z != 0.f))) {  // manytor.py:148
      row[i] = 0.f;
      (row + ld)[i] = 0.f;
      (row + 2 * ld)[i] = 0.f;
    }
    if (live) {
      float* orow = a.obs + (int64_t)(3 * p) * ld;
      __builtin_nontemporal_store(dist, orow + i);
      __builtin_nontemporal_store(r, orow + ld + i);
      __builtin_nontemporal_store(th, orow + 2 * ld + i);
    }
  }
#pragma unroll
  for (int sh = EPW; sh < 64; sh <<= 1) nam &= (uint32_t)__shfl_xor((int)nam, sh);

  const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);  // manytor.py:205-212
  bool done = (nam == 0u);                                    // manytor.py:170-171
  if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;
  if (live && q == 0) {
#pragma unroll
    for (int j = 0; j < D; ++j) (a.goals + j * ld)[i] = act[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(e[c], a.ee + c * ld + i);
    a.alive[i] = nam;
    __builtin_nontemporal_store(rew, a.reward + i);
    a.total_reward[i] = total_in + (float)rew;  // manytor.py:258
    if (a.snap) a.snap[i] = total_in + (float)rew;
    __builtin_nontemporal_store((uint8_t)(done ? 1 : 0), a.done + i);
  }
  // sub-lane 0 occupies lanes 0 .. EPW-1: the low EPW bits of the ballot are this wave's slice of the done_bits word
  const unsigned long long bits = __ballot(done && live && q == 0);
  if (lane == 0) {
    if (L == 2)
      reinterpret_cast<uint32_t*>(a.done_bits)[wave] = (uint32_t)bits;
    else
      reinterpret_cast<uint16_t*>(a.done_bits)[wave] = (uint16_t)bits;
  }
}

// Sub-step trajectory of the whole batch (manytor.py:190 appends joints_coordinates[3] of every
// sub-step to `trajectory`): the end effector at each of the S poses of the route goals -> action, as SoA rows
// [3S][ld] (row 3k + axis).  Launched BEFORE the step kernel of the same call (it needs the previous pose) with the
// same action source, only on handles created with MT_FLAG_TRACE: the timed step kernel is untouched.  Every pose gets
// the full polynomial sincos, like route_trace_kernel.
template <int D, bool SAMPLE>
__global__ __launch_bounds__(kBlock) void trace_kernel(const StepArgs a, float* trace) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  LaneOffset<true> o4{i * 4u};
  if (i >= a.n) return;
  const int64_t ld = a.ld;
  const RtTableF<D> t{a.dh};
  const uint32_t step_no = SAMPLE ? step_index(a) : 0u;  // ahead of the row accesses: see step_kernel
  float g[D], act[D], st[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = ldr(a.goals + j * ld, o4);
  if (SAMPLE) {
    draw_action<D>(((uint64_t)a.seed_hi << 32) | a.seed_lo, (uint64_t)(a.env_base + i), step_no, act);
  } else {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      act[j] = ldr(a.actions + j * ld, o4);
      bad |= unusable_angle(act[j]);
    }
    if (bad) {
#pragma unroll
      for (int j = 0; j < D; ++j) act[j] = g[j];
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) st[j] = (act[j] - g[j]) * a.inv_sm1;
  for (int k = 0; k < a.S; ++k) {
    float s[D], c[D], p[D][3];
    const double frac = (double)k / (double)(a.S - 1);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (wide_angle(g[j]) | wide_angle(act[j])) {  // see route_kinematics_wide
        if (k == a.S - 1)
          sincos_deg_off(act[j], t.off(j), s[j], c[j]);
        else
          sincos_deg_route(g[j], act[j], frac, t.off(j), s[j], c[j]);
        continue;
      }
      const float pose = (k == a.S - 1) ? act[j] : __builtin_fmaf((float)k, st[j], g[j]);  // np.linspace, manytor.py:182
      sincos_deg(pose + t.off(j), s[j], c[j]);
    }
    chain_all<RtTableF<D>>(s, c, t, p);
    float el[3], e[3];
    pick_frames<RtTableF<D>>(t, p, el, e);
#pragma unroll
    for (int q = 0; q < 3; ++q) str_stream(trace + (int64_t)(3 * k + q) * ld, o4, e[q]);
  }
}

// done_bits word `word` rebuilt from the done bytes: single-env launches (mt_env_step / mt_env_reset) cannot produce
// the 64-env ballot themselves.  One wavefront.
inline __global__ __launch_bounds__(64) void done_bits_word_kernel(const uint8_t* done, int64_t n, int64_t word,
                                                            unsigned long long* done_bits) {
  const int64_t i = word * 64 + threadIdx.x;
  const unsigned long long bits = __ballot(i < n && done[i] != 0);
  if (threadIdx.x == 0) done_bits[word] = bits;
}

// All done_bits words rebuilt from the done bytes (mt_set(MT_F_DONE): restoring a checkpoint).
inline __global__ __launch_bounds__(kBlock) void done_bits_rebuild_kernel(const uint8_t* done, int64_t n, unsigned long long* done_bits) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long bits = __ballot(i < n && done[i] != 0);
  if ((threadIdx.x & 63) == 0 && (int64_t)i < n) done_bits[i >> 6] = bits;
}


// Rejection-sample K targets for one env (manytor.py:229-239) and hand each accepted one to `put(k, x, y, z)`.
// Candidates are taken in the order (block 0, half 0), (block 0, half 1), (block 1, half 0), ...
// The draw loop is bounded; the tail branch is unreachable in practice (acceptance pi/6 per candidate).
template <class Put>
__device__ __forceinline__ void draw_targets(uint64_t seed, uint64_t env_id, uint32_t episode, int K, float radius,
                                             Put&& put) {
  int cnt = 0;
  for (uint32_t blk = 0; blk < 2048u && cnt < K; ++blk) {
    const u32x4 w = stream_block(seed, env_id, kTagTarget, episode, blk);
    float x, y, z;
    if (target_candidate<0>(w, radius, x, y, z)) {
      put(cnt, x, y, z);
      ++cnt;
    }
    if (cnt < K && target_candidate<1>(w, radius, x, y, z)) {
      put(cnt, x, y, z);
      ++cnt;
    }
  }
  for (; cnt < K; ++cnt) put(cnt, 0.f, 0.f, 0.5f * radius);
}

// ---------------------------------------------------------------------------
// action_sample for all envs (manytor.py:215-217), device RNG.
// ---------------------------------------------------------------------------
inline __global__ __launch_bounds__(kBlock) void sample_actions_kernel(float* actions, int64_t n, int64_t ld, int D,
                                                                int64_t env_base, uint64_t seed, uint32_t step_idx) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  const u32x4 w = stream_block(seed, (uint64_t)(env_base + i), kTagAction, step_idx, 0u);
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
  for (int j = 0; j < D; ++j)
    (actions + (int64_t)j * ld)[i] = (j < 4) ? action_from_word(ws[j]) : action_from_word_digit1(ws[j - 4]);
}

// ---------------------------------------------------------------------------
// reset (manytor.py:219-253).  RANDOM: draw the targets here; otherwise the
// caller has already filled `points`.  ONLY_DONE: re-arm finished envs only.
// ---------------------------------------------------------------------------
// The draw of reset_kernel, shared by the 64 envs of a wave.  Rejection sampling makes the lanes of a wave need different
// numbers of Philox blocks (6.7 on average for K = 7, ~13 for the unluckiest of 64), and a wave runs as long as its
// unluckiest lane.  So: while more than half of the lanes still need targets every lane draws for itself, one block per
// trip; once m <= 32 lanes are still needy, the whole wave works for them -- the 64 lanes are cut into m groups of
// h = 64 / m lanes, group g serves the g-th needy lane T and evaluates T's NEXT h blocks at once (lane r of the group:
// block blk_T + r), the accepted candidates are numbered in (block, half) order with two ballots and written straight
// into T's LDS column.  That is exactly the sequential order of draw_targets, so the targets are the same bits; the wave
// finishes in ~9 trips instead of ~13, and a reset_done with few finished envs in one or two.
// `need` = this lane's env wants targets; `col0` = the LDS column of the wave's lane 0 ([2K][kBlock] target codes per block).
__device__ __forceinline__ void draw_targets_wave(uint64_t seed, uint64_t env0, uint32_t episode, bool need, int K, float radius,
                                                  float* col0, uint8_t* slots) {
  const uint32_t lane = threadIdx.x & 63u;
  auto put = [&](uint32_t t, int k, TargetCode c) {  // (the stage is float: the words travel as bit patterns, never as values)
    float* cell = col0 + t + 2 * k * kBlock;
    cell[0] = __uint_as_float(c.lo);
    cell[kBlock] = __uint_as_float(c.hi);
  };
  int cnt = need ? 0 : K;
  uint32_t blk = 0;
  unsigned long long M = __ballot(cnt < K);
  for (int trip = 0; M != 0ull && trip < 4096; ++trip) {
    const int m = __popcll(M);
    if (m > 32) {  // every needy lane for itself: one block, two candidates (draw_targets' loop body)
      if (cnt < K) {
        const u32x4 w = stream_block(seed, env0 + lane, kTagTarget, episode, blk);
        float x, y, z;
        TargetCode c;
        if (target_candidate<0>(w, radius, x, y, z, &c)) put(lane, cnt++, c);
        if (cnt < K && target_candidate<1>(w, radius, x, y, z, &c)) put(lane, cnt++, c);
        ++blk;
      }
    } else {
      const uint32_t h = 64u / (uint32_t)m;                                   // lanes per needy lane: 2 .. 64
      const bool needy = cnt < K;
      const uint32_t rank = (uint32_t)__popcll(M & ((1ull << lane) - 1ull));  // needy lane -> its group
      if (needy) slots[rank] = (uint8_t)lane;
      __builtin_amdgcn_wave_barrier();
      const uint32_t g = lane / h, r = lane % h;
      const bool serving = g < (uint32_t)m;
      const uint32_t T = serving ? slots[g] : 0u;
      __builtin_amdgcn_wave_barrier();                                        // all reads done before the next trip's writes
      const uint32_t blkT = (uint32_t)__shfl((int)blk, (int)T);
      const int cntT = __shfl(cnt, (int)T);
      const uint32_t epT = (uint32_t)__shfl((int)episode, (int)T);
      bool a0 = false, a1 = false;
      float x0 = 0.f, y0 = 0.f, z0 = 0.f, x1 = 0.f, y1 = 0.f, z1 = 0.f;
      TargetCode c0{0u, 0u}, c1{0u, 0u};
      if (serving) {
        const u32x4 w = stream_block(seed, env0 + T, kTagTarget, epT, blkT + r);
        a0 = target_candidate<0>(w, radius, x0, y0, z0, &c0);
        a1 = target_candidate<1>(w, radius, x1, y1, z1, &c1);
      }
      const unsigned long long A0 = __ballot(a0), A1 = __ballot(a1);
      auto group_mask = [&](uint32_t grp) { return (h == 64u ? ~0ull : ((1ull << h) - 1ull)) << (grp * h); };
      if (serving) {  // number my candidates behind those of the lower lanes of my group: (block, half) order
        const unsigned long long lower = group_mask(g) & ((1ull << lane) - 1ull);
        const int k0 = cntT + __popcll(A0 & lower) + __popcll(A1 & lower);
        if (a0 && k0 < K) put(T, k0, c0);
        const int k1 = k0 + (a0 ? 1 : 0);
        if (a1 && k1 < K) put(T, k1, c1);
      }
      if (needy) {  // what my group found for me
        const unsigned long long gm = group_mask(rank);
        cnt += __popcll(A0 & gm) + __popcll(A1 & gm);
        blk += h;
      }
    }
    M = __ballot(cnt < K);
  }
  for (; cnt < K; ++cnt) put(lane, cnt, kFallbackTargetCode);  // unreachable in practice, as in draw_targets
  __builtin_amdgcn_wave_barrier();  // a lane's column was written by other lanes of its wave
}

// A thread's LDS column of draw_targets_wave ([2K][kBlock] codes) turned into the [3K][kBlock] floats in place: last target
// first, so the rows written for target k (3k .. 3k + 2) lie past the code rows of every target below it (<= 2k - 1).
__device__ __forceinline__ void decode_column(float* col, int K, float radius) {
  for (int k = K - 1; k >= 0; --k) {
    const TargetCode c = staged_code(col + 2 * k * kBlock, kBlock);
    float x, y, z;
    decode_target(c, radius, x, y, z);
    col[3 * k * kBlock] = x;
    col[(3 * k + 1) * kBlock] = y;
    col[(3 * k + 2) * kBlock] = z;
  }
}

// Target k of env i as a reset leaves it: the floats decoded from its code (MT_F_POINTS), and the code.
__device__ __forceinline__ void store_target(const StepArgs& a, int64_t ld, uint32_t i, int k, TargetCode c, float radius) {
  float x, y, z;
  decode_target(c, radius, x, y, z);
  float* row = a.points + (int64_t)(3 * k) * ld;
  row[i] = x;
  (row + ld)[i] = y;
  (row + 2 * ld)[i] = z;
  uint32_t* crow = a.codes + (int64_t)(2 * k) * ld;
  crow[i] = c.lo;
  (crow + ld)[i] = c.hi;
}

// The draw of an env that is spread over L lanes of a wave (lane = q * (64 / L) + e: reset_split_kernel, rollout_split_kernel):
// sub-lane q evaluates blocks q, q + L, q + 2 L, ...; in every round the accepted candidates are numbered in block order across
// the env's sub-lanes (their counts travel by shuffle), so the K target codes handed to `put(k, code)` -- by whichever sub-lane
// found them -- are exactly the first K accepted candidates of draw_targets' sequential order: the same bits.  Every sub-lane of
// the env must call it (`go` = the env wants targets; equal in all of them, so they leave the loop together).
template <int L, class Put>
__device__ __forceinline__ void draw_targets_split(uint64_t seed, uint64_t env_id, uint32_t episode, bool go, int K, float radius,
                                                   uint32_t q, uint32_t e, Put&& put) {
  constexpr int EPW = 64 / L;
  int cnt = go ? 0 : K;
  for (uint32_t round = 0; round < 2048u / L && cnt < K; ++round) {
    const u32x4 w = stream_block(seed, env_id, kTagTarget, episode, round * L + q);
    float x0, y0, z0, x1, y1, z1;
    TargetCode c0, c1;
    const bool a0 = target_candidate<0>(w, radius, x0, y0, z0, &c0);
    const bool a1 = target_candidate<1>(w, radius, x1, y1, z1, &c1);
    const int mine = (a0 ? 1 : 0) + (a1 ? 1 : 0);
    int before = 0, total = 0;
#pragma unroll
    for (int qq = 0; qq < L; ++qq) {
      const int c = __shfl(mine, qq * EPW + (int)e);
      total += c;
      before += (qq < (int)q) ? c : 0;
    }
    const int k0 = cnt + before;
    if (a0 && k0 < K) put(k0, c0);
    const int k1 = k0 + (a0 ? 1 : 0);
    if (a1 && k1 < K) put(k1, c1);
    cnt += total;
  }
  if (q == 0)
    for (; cnt < K; ++cnt) put(cnt, kFallbackTargetCode);  // unreachable in practice, as in draw_targets
}

template <int D, bool RANDOM, bool ONLY_DONE>
__global__ __launch_bounds__(kBlock) void reset_kernel(const StepArgs a, float radius) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < a.n;
  if (!RANDOM && !valid) return;  // with RANDOM every lane of a wave takes part in the draw (draw_targets_wave)
  const int64_t ld = a.ld;
  // done byte: 1 = finished, waiting for this call; 2 = finished and already re-armed inside mt_rollout_fused
  const uint8_t dn = !valid ? (uint8_t)0 : (ONLY_DONE ? a.done[i] : (uint8_t)1);
  const bool go = dn == 1;
  if (ONLY_DONE && dn == 2) a.done[i] = 0;
  uint32_t episode = a.major;
  if (go) {
    float s[D], c[D], p[D][3];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      (a.goals + j * ld)[i] = 0.f;
      sincos_deg(a.dh.off_deg[j], s[j], c[j]);
    }
    const RtTableF<D> t{a.dh};
    chain_all<RtTableF<D>>(s, c, t, p);  // joints_coordinates at the zero pose, manytor.py:224-225
    float el0[3], e0[3];
    pick_frames<RtTableF<D>>(t, p, el0, e0);
#pragma unroll
    for (int q = 0; q < 3; ++q) (a.ee + q * ld)[i] = e0[q];
    if (ONLY_DONE)
      record_finished(a, i, a.episodes[i], a.total_reward[i]);
    else
      a.last_return[i] = a.total_reward[i];
    a.total_reward[i] = 0.f;
    a.reward[i] = 0;
    a.done[i] = 0;
    uint32_t all_alive = all_alive_mask(a.K);
    if (!RANDOM) {
      // Targets the caller placed (mt_reset; from device memory they cannot be screened on the host): one with a NaN or an
      // infinite coordinate is dropped -- dead from the start, coordinates zeroed, counted with the unusable actions -- instead
      // of reaching arithmetic that is built with -ffinite-math-only.  Tested on the bit pattern.
      for (int k = 0; k < a.K; ++k) {
        float* row = a.points + (int64_t)(3 * k) * ld;
        const uint32_t bx = __float_as_uint(row[i]), by = __float_as_uint((row + ld)[i]), bz = __float_as_uint((row + 2 * ld)[i]);
        if (((bx & 0x7FFFFFFFu) > 0x7F7FFFFFu) | ((by & 0x7FFFFFFFu) > 0x7F7FFFFFu) | ((bz & 0x7FFFFFFFu) > 0x7F7FFFFFu)) {
          row[i] = 0.f;
          (row + ld)[i] = 0.f;
          (row + 2 * ld)[i] = 0.f;
          all_alive &= ~(1u << k);
          atomicAdd(a.bad_actions, 1u);
        }
      }
    }
    a.alive[i] = all_alive;
    // full reset: the caller names the episode; re-arm of a finished env: its own counter advances by one
    if (ONLY_DONE) episode = a.episodes[i] + 1u;
    a.episodes[i] = episode;
  }
  if (RANDOM) {
    // manytor.py:229-239: uniform in the cube, keep z >= 0 and |p| <= radius.  z is drawn from
    // [0, R) directly (same conditional law).  fp32, one rounding per op, mirrored by oracle/philox_ref.py.
    // Envs of one wave accept their k-th target at different candidates, so storing from inside the draw loop
    // would write partial lines of different rows per instruction.  The codes of the accepted targets are parked in the
    // env's LDS column ([2K][kBlock] words, conflict-free) and written out row by row afterwards, codes and floats.
    extern __shared__ float stage[];
    __shared__ uint8_t slots[kBlock / 64][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t seed = ((uint64_t)a.seed_hi << 32) | a.seed_lo;
    draw_targets_wave(seed, (uint64_t)(a.env_base + (i - lane)), episode, go, a.K, radius, stage + (threadIdx.x - lane),
                      slots[threadIdx.x >> 6]);
    if (go) {
      const float* col = stage + threadIdx.x;
      for (int k = 0; k < a.K; ++k) store_target(a, ld, i, k, staged_code(col + 2 * k * kBlock, kBlock), radius);
    }
  }
  if (valid && (threadIdx.x & 63) == 0) a.done_bits[i >> 6] = 0ull;  // every env of the wave has done == 0 now
}

// reset with the draw of an env's targets spread over L lanes of a wave -- for batches so small that the kernel's time
// is one wave per SIMD walking its ~13 Philox blocks one after the other (11-12 us at <= 65 536 arms, of which the
// launch and the stores are about half).  Lane layout as in step_split_kernel (lane = q * (64 / L) + e).  Sub-lane q of an
// env evaluates blocks q, q + L, q + 2 L, ...; in every round the accepted candidates are numbered in block order
// across the env's sub-lanes (their counts travel by shuffle), so the K targets are exactly the first K accepted
// candidates of draw_targets' sequential order: the same bits as reset_kernel.  The target codes are parked in the env's
// LDS column ([2K][kBlock / L]) and written out (codes and floats) by the sub-lanes in turn; everything else by sub-lane 0.
template <int D, bool ONLY_DONE, int L>
__global__ __launch_bounds__(kBlock) void reset_split_kernel(const StepArgs a, float radius) {
  static_assert(L == 2 || L == 4, "an env is spread over 2 or 4 lanes");
  extern __shared__ float stage[];  // [2K][kBlock / L] target codes
  constexpr int EPW = 64 / L;
  constexpr int EPB = kBlock / L;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t q = lane / EPW;
  const uint32_t e = lane % EPW;
  const int64_t first = (int64_t)wave * EPW;
  if (first >= a.n) return;
  const uint32_t env = (uint32_t)first + e;
  const bool live = env < a.n;  // tail lanes shadow the last env (in their own column) and store nothing
  const uint32_t i = live ? env : (uint32_t)(a.n - 1);
  const int64_t ld = a.ld;
  // every sub-lane reads what it needs of the old state first; sub-lane 0 overwrites it after the draw
  const uint8_t dn = ONLY_DONE ? a.done[i] : (uint8_t)1;
  const bool go = dn == 1;
  const uint32_t old_episode = ONLY_DONE ? a.episodes[i] : 0u;
  const float old_total = a.total_reward[i];
  const uint32_t episode = ONLY_DONE ? old_episode + 1u : a.major;
  float* col = stage + (threadIdx.x >> 6) * EPW + e;
  const uint64_t seed = ((uint64_t)a.seed_hi << 32) | a.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);
  const int K = a.K;
  auto put = [&](int k, TargetCode c) {  // (bit patterns in the float stage, as in draw_targets_wave)
    float* cell = col + 2 * k * EPB;
    cell[0] = __uint_as_float(c.lo);
    cell[EPB] = __uint_as_float(c.hi);
  };
  draw_targets_split<L>(seed, env_id, episode, go, K, radius, q, e, put);
  __builtin_amdgcn_wave_barrier();  // the columns were written by the env's sub-lanes; a wave only touches its own
  if (live && go)
    for (int k = (int)q; k < K; k += L) store_target(a, ld, i, k, staged_code(col + 2 * k * EPB, EPB), radius);
  if (live && q == 0) {
    if (ONLY_DONE && dn == 2) a.done[i] = 0;
    if (go) {
      float s[D], c[D], p[D][3];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        (a.goals + j * ld)[i] = 0.f;
        sincos_deg(a.dh.off_deg[j], s[j], c[j]);
      }
      const RtTableF<D> t{a.dh};
      chain_all<RtTableF<D>>(s, c, t, p);
      float el0[3], e0[3];
      pick_frames<RtTableF<D>>(t, p, el0, e0);
#pragma unroll
      for (int qq = 0; qq < 3; ++qq) (a.ee + qq * ld)[i] = e0[qq];
      if (ONLY_DONE)
        record_finished(a, i, old_episode, old_total);
      else
        a.last_return[i] = old_total;
      a.total_reward[i] = 0.f;
      a.reward[i] = 0;
      a.done[i] = 0;
      a.alive[i] = all_alive_mask(K);
      a.episodes[i] = episode;
    }
  }
  if (lane == 0) a.done_bits[first >> 6] = 0ull;  // every env of the word has done == 0 after this launch
}

// One env's column of an LDS target tile [3K][STRIDE], as rollout_kernel and rollout_tape_kernel (STRIDE = kBlock) and
// rollout_split_kernel (kBlock / L) keep it: coordinate c of target k is col[(3 k + c) * STRIDE].
template <int STRIDE>
struct TargetColumn {
  float* col;
  __device__ __forceinline__ float& row(int r) const { return col[r * STRIDE]; }  // r = 3 k + c, the row of MT_F_POINTS
  __device__ __forceinline__ float& cell(int k, int c) const { return row(3 * k + c); }
  __device__ __forceinline__ float* target(int k) const { return col + 3 * k * STRIDE; }  // x, y, z at [0], [STRIDE], [2 STRIDE]
  __device__ __forceinline__ void get(int k, float& x, float& y, float& z) const { x = target(k)[0], y = target(k)[STRIDE], z = target(k)[2 * STRIDE]; }
  __device__ __forceinline__ void put(int k, float x, float y, float z) const { target(k)[0] = x, target(k)[STRIDE] = y, target(k)[2 * STRIDE] = z; }
  __device__ __forceinline__ void zero(int k) const { put(k, 0.f, 0.f, 0.f); }
};

// ---------------------------------------------------------------------------
// rollout: T consecutive Environment.step()s with in-kernel random actions in ONE launch (the inner loop of
// test_multi.py:19-21), optionally re-arming an env the moment it finishes.
// Joint angles, alive mask and return stay in registers between steps and the env's targets stay in LDS
// ([3K][256] floats per block, one column per thread, conflict-free), so per step only the outputs are
// written: obs 12K + reward 4 + done 1 + ee 12 bytes per env instead of the 233 a single-step launch moves.
// Per step it runs exactly the arithmetic of step_kernel (shared device functions), so
//   rollout(T)  ==  T x step_random          (auto_reset = 0)
//   rollout(T)  ==  T x (step_random; reset_done)   (auto_reset = 1, state fields)
// bit for bit; tests/test_gpu_parity.py checks both.
// ---------------------------------------------------------------------------
struct RolloutArgs {
  int32_t T;
  uint32_t step0;
  uint32_t auto_reset;
  float radius;
  // Episode boundary folded into the launch (mt_rollout's multi-step form, engine.hip):
  //   reset_first : the launch BEGINS with the full random reset of every env that mt_reset_random(reset seed, reset_episode)
  //                 deferred to it -- last_return <- return, zero pose, all targets alive, episode index, targets drawn from
  //                 the (seed, env, episode) stream in draw_targets' sequential order: reset_kernel<.., RANDOM, false>'s
  //                 state, bit for bit -- instead of loading pose / alive mask / return / targets: no reset launch, no
  //                 re-fetch of what it would have written
  //   snap        : the launch ENDS by storing every env's return to this row as well (the snapshot the overlapped return
  //                 gather would otherwise take with a launch of its own behind it), or NULL
  uint32_t reset_first, reset_episode, reset_seed_lo, reset_seed_hi;
  float* snap;
};

//   RPF : prologue form.  0: the state and all targets are loaded (targets straight into LDS) before the first step starts
//         -- a launch's first step then waits for the table load, the barrier and every state load in turn before its
//         Philox block even begins (~6 us before the first step's outputs at 131 072 envs, tools/rollout_k_sweep.py), which
//         nothing amortises when mt_rollout runs only a few steps per launch.  RPF = kPrefetch: everything is REQUESTED at
//         the top (table, pose, alive mask, return, the first RPF targets into registers), the first step's Philox block and
//         kinematics run under those loads, and the targets go to LDS between the first step's kinematics and its target
//         loop (step 0 is peeled).  Same device functions on the same inputs: the same bits.  The host takes RPF for the
//         short launches of mt_rollout (engine.hip), the long fused launches keep RPF = 0 (24 fewer live registers).
template <class Tbl, int RPF = 0>
__global__ __launch_bounds__(kBlock) void rollout_kernel(const StepArgs a, const RolloutArgs r) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [3K][kBlock] (+ the action sin / cos table for the compile-time tables)
  constexpr int D = Tbl::D;
  constexpr bool kTable = ActionTrigTable<Tbl>::value;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const SinCos* trig = nullptr;
  float4 trig_v;
  if constexpr (kTable) {
    trig = reinterpret_cast<const SinCos*>(tile + 3 * a.K * kBlock);
    trig_v = trig_table_load(a.trig_table);
    if (!RPF) trig_table_commit(reinterpret_cast<SinCos*>(tile + 3 * a.K * kBlock), trig_v);
  }
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  LaneOffset<true> o4{i * 4u}, o1{i};
  // (threads past the end: with a table and RPF they stay until the barrier -- their loads stay inside the rows, which are
  // ld >= round_up(n, 256) long, and the launch covers the batch or a 256-aligned range of it -- and leave right behind it)
  // (... and with a reset folded into the launch every lane of a wave takes part in the wave-cooperative draw below)
  const bool stay = (kTable && RPF) || r.reset_first != 0;
  if (!stay && i >= a.n) return;
  const int64_t ld = a.ld;
  const uint64_t seed = ((uint64_t)a.seed_hi << 32) | a.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);
  const TargetColumn<kBlock> tc{tile + threadIdx.x};
  __shared__ uint8_t draw_slots[kBlock / 64][64];  // draw_targets_wave's scratch (used by launches with reset_first only)

  const uint32_t all_alive = all_alive_mask(a.K);
  const bool fresh = r.reset_first != 0;  // (wave-uniform: a launch argument)
  float g[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = fresh ? 0.f : ldr(a.goals + j * ld, o4);
  uint32_t am = fresh ? all_alive : ldr(a.alive, o4);
  float total = ldr(a.total_reward, o4);
  uint32_t episode = fresh ? r.reset_episode : (r.auto_reset ? ldr(a.episodes, o4) : 0u);
  bool ended = fresh, dirty = fresh;  // a fresh episode writes its episode index and its targets back at the end
  float tx[RPF ? RPF : 1][3];
  if (fresh) {
    const bool mine = i < a.n;  // (threads past the end help with the draw and stay for the barrier, nothing else)
    if (mine) str(a.last_return, o4, total);  // what reset_kernel<.., RANDOM, false> keeps of the episode that ends here
    total = 0.f;
    const uint32_t lane = threadIdx.x & 63u;
    draw_targets_wave(((uint64_t)r.reset_seed_hi << 32) | r.reset_seed_lo, (uint64_t)(a.env_base + (i - lane)), episode, mine, a.K, r.radius,
                      tile + (threadIdx.x - lane), draw_slots[threadIdx.x >> 6]);
    decode_column(tc.col, a.K, r.radius);
    if (!(kTable && RPF) && !mine) return;
  } else if (RPF) {
#pragma unroll
    for (int k = 0; k < RPF; ++k)
      if (k < a.K) {
#pragma unroll
        for (int q = 0; q < 3; ++q) tx[k][q] = ldr(a.points + (int64_t)(3 * k + q) * ld, o4);
      }
  } else {
    for (int k = 0; k < 3 * a.K; ++k) tc.row(k) = ldr(a.points + (int64_t)k * ld, o4);
  }
  PoseCache<D> pose;        // sines / cosines and frame heights of the pose the next step starts from
  bool pose_valid = false;  // nothing known about the pose loaded from memory

  // one step behind its kinematics: observation / pickup per target, outputs, re-arm (the body of the loop below)
  auto finish_step = [&](const float (&act)[D], const float (&el)[3], const float (&e)[3], float zmin) {
    const bool ground = zmin < 0.f;
    if (a.zmin) str_stream(a.zmin, o4, zmin);  // MT_FLAG_DEBUG_ZMIN (a step output like reward: the last step's stays)

    uint32_t nam = am;
    for (int k = 0; k < a.K; ++k) {
      float x, y, z, dist = 0.f, rr = 0.f, th = 0.f;
      tc.get(k, x, y, z);
      if ((am >> k) & 1u) {
        observe_target(el, x, y, z, dist, rr, th);
        if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << k);
      } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {  // manytor.py:148
        tc.zero(k);
        dirty = true;
      }
      float* orow = a.obs + (int64_t)(3 * k) * ld;
      str_stream(orow, o4, dist);
      str_stream(orow + ld, o4, rr);
      str_stream(orow + 2 * ld, o4, th);
    }
    const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);
    bool done = (nam == 0u);
    if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;
    total += (float)rew;
    am = nam;
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = act[j];
#pragma unroll
    for (int q = 0; q < 3; ++q) str_stream(a.ee + q * ld, o4, e[q]);
    str_stream(a.reward, o4, rew);
    // 2 = "finished in this step and already re-armed below": mt_reset_done must not re-arm it a second time
    str_stream(a.done, o1, (uint8_t)(done ? (r.auto_reset ? 2 : 1) : 0));
    const unsigned long long bits = __ballot(done);
    if ((threadIdx.x & 63) == 0) a.done_bits[i >> 6] = bits;

    if (done && r.auto_reset) {  // re-arm: what reset_kernel<.., RANDOM, ONLY_DONE> does in a separate launch
      record_finished(a, i, episode, total);
      ended = true;
      total = 0.f;
      am = all_alive;
      episode += 1u;
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = 0.f;
      pose_valid = false;  // the cache describes the pose the finished episode ended in, not the zero pose
      draw_targets(seed, env_id, episode, a.K, r.radius, [&](int k, float x, float y, float z) { tc.put(k, x, y, z); });
      dirty = true;
    }
  };

  int s = 0;
  if (RPF) {  // step 0, peeled: its Philox block and kinematics run under the loads requested above
    float act[D], el[3], e[3];
    draw_action<D>(seed, env_id, r.step0, act);
    if constexpr (kTable) {
      complete_before_here(act);
      trig_table_commit(reinterpret_cast<SinCos*>(tile + 3 * a.K * kBlock), trig_v);
      if (i >= a.n) return;
    }
    const float zmin = route_kinematics<Tbl, 0, true, kTable>(t, a.S, a.inv_sm1, g, act, el, e, &pose, false, trig,
                                                              (a.flags & kFlagWholeGoals) != 0);
    pose_valid = true;
    if (!fresh) {  // (a fresh episode's targets were drawn straight into LDS)
#pragma unroll
      for (int k = 0; k < RPF; ++k)
        if (k < a.K) {
#pragma unroll
          for (int q = 0; q < 3; ++q) tc.cell(k, q) = tx[k][q];
        }
      for (int k = 3 * RPF; k < 3 * a.K; ++k) tc.row(k) = ldr(a.points + (int64_t)k * ld, o4);
    }
    finish_step(act, el, e, zmin);
    s = 1;
  }
  for (; s < r.T; ++s) {
    float act[D], el[3], e[3];
    draw_action<D>(seed, env_id, r.step0 + (uint32_t)s, act);
    const float zmin = route_kinematics<Tbl, 0, true, kTable>(t, a.S, a.inv_sm1, g, act, el, e, &pose, pose_valid, trig,
                                                              (a.flags & kFlagWholeGoals) != 0 || s > 0);
    pose_valid = true;
    finish_step(act, el, e, zmin);
  }

#pragma unroll
  for (int j = 0; j < D; ++j) str(a.goals + j * ld, o4, g[j]);
  str(a.alive, o4, am);
  str(a.total_reward, o4, total);
  if (r.snap) str(r.snap, o4, total);
  if (ended) str(a.episodes, o4, episode);
  if (dirty)
    for (int k = 0; k < 3 * a.K; ++k) str(a.points + (int64_t)k * ld, o4, tc.row(k));
}

// rollout with one env spread over L lanes (L = 2 or 4): rollout_kernel for batches so small that a step's time is one
// wave's dependent chain.  Lane layout, kinematics halves and target partition as in step_split_kernel; joint angles,
// alive mask, return and episode counter are replicated in the env's sub-lanes (they all see the same combined z-min and
// alive mask, so they stay equal); the targets live in LDS, one column per ENV ([3K][kBlock / L]), written by whichever
// sub-lane owns the target.  A wave only ever touches its own columns: wave_barrier() orders the LDS traffic, no
// block barrier.  Bit-identical to rollout_kernel.
template <class Tbl, int L, int RPF = 0>
__global__ __launch_bounds__(kBlock) void rollout_split_kernel(const StepArgs a, const RolloutArgs r) {
  static_assert(L == 2 || L == 4, "an env is spread over 2 or 4 lanes");
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [3K][kBlock / L] (+ the action sin / cos table for the compile-time tables)
  constexpr int D = Tbl::D;
  constexpr int EPW = 64 / L;
  constexpr int EPB = kBlock / L;  // envs per block = columns of the tile
  constexpr int PFS = (RPF + L - 1) / L;  // targets per sub-lane requested up front (RPF form, see rollout_kernel)
  constexpr bool kTable = ActionTrigTable<Tbl>::value;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const SinCos* trig = nullptr;
  float4 trig_v;
  if constexpr (kTable) {
    trig = reinterpret_cast<const SinCos*>(tile + 3 * a.K * EPB);
    trig_v = trig_table_load(a.trig_table);
    if (!RPF) trig_table_commit(reinterpret_cast<SinCos*>(tile + 3 * a.K * EPB), trig_v);
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint32_t q = lane / EPW;
  const int64_t first = (int64_t)wave * EPW;
  if (first >= a.n) {  // whole wave beyond the batch
    if constexpr (kTable) {
      if (RPF) trig_table_commit(reinterpret_cast<SinCos*>(tile + 3 * a.K * EPB), trig_v);  // its arrival at the block's barrier
    }
    return;
  }
  const uint32_t env = (uint32_t)first + lane % EPW;
  const bool live = env < a.n;  // tail lanes work on a copy of the last env (in their own column) and store nothing
  const uint32_t i = live ? env : (uint32_t)(a.n - 1);
  const int64_t ld = a.ld;
  const uint64_t seed = ((uint64_t)a.seed_hi << 32) | a.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);
  const TargetColumn<EPB> tc{tile + (threadIdx.x >> 6) * EPW + lane % EPW};
  const bool backward = (q & 1u) != 0;

  const uint32_t all_alive = all_alive_mask(a.K);
  const bool fresh = r.reset_first != 0;  // (wave-uniform: a launch argument; see RolloutArgs)
  float g[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = fresh ? 0.f : (a.goals + j * ld)[i];
  uint32_t am = fresh ? all_alive : a.alive[i];
  float total = a.total_reward[i];
  uint32_t episode = fresh ? r.reset_episode : (r.auto_reset ? a.episodes[i] : 0u);
  bool ended = fresh, dirty = fresh;
  float tx[PFS ? PFS : 1][3];
  if (fresh) {  // the env's sub-lanes share the draw (reset_split_kernel's), whoever finds a target parks it in the env's column
    if (live && q == 0) a.last_return[i] = total;
    total = 0.f;
    draw_targets_split<L>(((uint64_t)r.reset_seed_hi << 32) | r.reset_seed_lo, env_id, episode, true, a.K, r.radius, q, lane % EPW,
                          [&](int k, TargetCode c) { decode_target(c, r.radius, tc.target(k)[0], tc.target(k)[EPB], tc.target(k)[2 * EPB]); });
    __builtin_amdgcn_wave_barrier();  // a target's cells may have been written by another sub-lane of the env (same wave)
  } else if (RPF) {  // this sub-lane's first targets into registers (target index p = q + L * m)
#pragma unroll
    for (int m = 0; m < PFS; ++m) {
      const int p = (int)q + L * m;
      if (p < a.K) {
        const float* row = a.points + (int64_t)(3 * p) * ld;
#pragma unroll
        for (int c = 0; c < 3; ++c) tx[m][c] = (row + c * ld)[i];
      }
    }
  } else {
    for (int p = (int)q; p < a.K; p += L) {  // this sub-lane's targets into the env's column
      const float* row = a.points + (int64_t)(3 * p) * ld;
#pragma unroll
      for (int c = 0; c < 3; ++c) tc.cell(p, c) = (row + c * ld)[i];
    }
  }
  PoseCache<D> pose;
  bool pose_valid = false;

  auto finish_step = [&](const float (&act)[D], const float (&el)[3], const float (&e)[3], float zmin) {
    const bool ground = zmin < 0.f;
    if (a.zmin && live && q == 0) __builtin_nontemporal_store(zmin, a.zmin + i);  // MT_FLAG_DEBUG_ZMIN

    uint32_t nam = am;
    for (int p = (int)q; p < a.K; p += L) {
      float x, y, z, dist = 0.f, rr = 0.f, th = 0.f;
      tc.get(p, x, y, z);
      if ((am >> p) & 1u) {
        observe_target(el, x, y, z, dist, rr, th);
        if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << p);
      } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {  // manytor.py:148
        tc.zero(p);
        dirty = true;
      }
      if (live) {
        float* orow = a.obs + (int64_t)(3 * p) * ld;
        __builtin_nontemporal_store(dist, orow + i);
        __builtin_nontemporal_store(rr, orow + ld + i);
        __builtin_nontemporal_store(th, orow + 2 * ld + i);
      }
    }
#pragma unroll
    for (int sh = EPW; sh < 64; sh <<= 1) nam &= (uint32_t)__shfl_xor((int)nam, sh);
    const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);
    bool done = (nam == 0u);
    if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;
    total += (float)rew;
    am = nam;
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = act[j];
    if (live && q == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(e[c], a.ee + c * ld + i);
      __builtin_nontemporal_store(rew, a.reward + i);
      __builtin_nontemporal_store((uint8_t)(done ? (r.auto_reset ? 2 : 1) : 0), a.done + i);
    }
    const unsigned long long bits = __ballot(done && live && q == 0);
    if (lane == 0) {
      if (L == 2)
        reinterpret_cast<uint32_t*>(a.done_bits)[wave] = (uint32_t)bits;
      else
        reinterpret_cast<uint16_t*>(a.done_bits)[wave] = (uint16_t)bits;
    }

    if (done && r.auto_reset) {  // re-arm, as in rollout_kernel; every sub-lane draws, each keeps its own targets
      if (live && q == 0) record_finished(a, i, episode, total);
      ended = true;
      total = 0.f;
      am = all_alive;
      episode += 1u;
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = 0.f;
      pose_valid = false;
      draw_targets(seed, env_id, episode, a.K, r.radius, [&](int k, float x, float y, float z) {
        if ((uint32_t)k % L == q) tc.put(k, x, y, z);
      });
      dirty = true;
    }
  };

  int s = 0;
  if (RPF) {  // step 0, peeled: its Philox block and kinematics run under the loads requested above
    float act[D], el[3], e[3];
    draw_action<D>(seed, env_id, r.step0, act);
    if constexpr (kTable) {
      complete_before_here(act);
      trig_table_commit(reinterpret_cast<SinCos*>(tile + 3 * a.K * EPB), trig_v);
    }
    const float zmin = route_kinematics_split<Tbl, L, true, kTable>(t, a.S, a.inv_sm1, g, act, backward, el, e, &pose, false, trig,
                                                                    (a.flags & kFlagWholeGoals) != 0);
    pose_valid = true;
    if (!fresh) {  // (a fresh episode's targets were drawn straight into LDS)
#pragma unroll
      for (int m = 0; m < PFS; ++m) {
        const int p = (int)q + L * m;
        if (p < a.K) {
#pragma unroll
          for (int c = 0; c < 3; ++c) tc.cell(p, c) = tx[m][c];
        }
      }
      for (int p = (int)q + L * PFS; p < a.K; p += L) {
        const float* row = a.points + (int64_t)(3 * p) * ld;
#pragma unroll
        for (int c = 0; c < 3; ++c) tc.cell(p, c) = (row + c * ld)[i];
      }
    }
    finish_step(act, el, e, zmin);
    s = 1;
  }
  for (; s < r.T; ++s) {
    float act[D], el[3], e[3];
    draw_action<D>(seed, env_id, r.step0 + (uint32_t)s, act);
    const float zmin = route_kinematics_split<Tbl, L, true, kTable>(t, a.S, a.inv_sm1, g, act, backward, el, e, &pose, pose_valid,
                                                                    trig, (a.flags & kFlagWholeGoals) != 0 || s > 0);
    pose_valid = true;
    finish_step(act, el, e, zmin);
  }

  if (live && q == 0) {
#pragma unroll
    for (int j = 0; j < D; ++j) (a.goals + j * ld)[i] = g[j];
    a.alive[i] = am;
    a.total_reward[i] = total;
    if (r.snap) r.snap[i] = total;
    if (ended) a.episodes[i] = episode;
  }
  if (live && dirty)
    for (int p = (int)q; p < a.K; p += L) {
      float* row = a.points + (int64_t)(3 * p) * ld;
#pragma unroll
      for (int c = 0; c < 3; ++c) (row + c * ld)[i] = tc.cell(p, c);
    }
}

// ---------------------------------------------------------------------------
// rollout driven by a device action tape (mt_rollout_tape): rollout_kernel with the second action source -- joint j of
// env i at step s is tape[(s * D + j) * tape_ld + i], screened like step_kernel's staged action (unusable_angle: the env
// holds its pose, the pair is counted) -- for callers that hold the next T actions of every env on the device (sampling
// planners, replays, open-loop policy chunks).  Pose, alive mask and return stay in registers and the targets in LDS
// ([3K][kBlock]) as in rollout_kernel; per step it runs the device functions step_kernel runs on the same inputs
// (route_kinematics with no whole-degree assumption: TABLE = false, prev_whole = false; within_box; the dead-target
// zeroing), so
//   tape(T)  ==  T x (set_actions(row t); step)                 (auto_reset = 0)
//   tape(T)  ==  T x (set_actions(row t); step; reset_done)     (auto_reset = 1, state fields)
// bit for bit.  PoseCache is kept across steps: it holds sincos_deg(act + off) of the action just taken, which is the
// very float and function the next step would evaluate for its start pose, fractional angles included.
// What the intermediate steps skip: the observation arithmetic (observe_target) and every MT_F_* output store -- only
// the LAST step of the call writes obs / reward / done / ee / zmin.  What every step writes: two log bytes (reward,
// done), where asked for.  Per env-step: 4 D bytes of tape read + 2 bytes of logs; the state is read and written once
// per call.
//   dry_run  : nothing resident is written (arena, ring, bad-action counter): only the logs and return_out
//   PREFETCH : the tape row of step s + 1 is requested before the kinematics of step s (D more live registers); else it is
//              requested behind step s, once nothing else is live.  Instantiated for the compile-time tables only.
//   nt_loads : the tape is read with non-temporal loads (it is read once)
// One env per lane, one form for every batch size and table kind.
// ---------------------------------------------------------------------------
struct TapeArgs {
  const float* tape;     // [T * D][tape_ld]
  int64_t tape_ld;
  int8_t* reward_log;    // [T][log_ld] or NULL
  uint8_t* done_log;     // [T][log_ld] or NULL
  int64_t log_ld;
  float* return_out;     // [n] or NULL
  int32_t T;
  uint32_t auto_reset, dry_run, nt_loads;
  uint32_t seed_lo, seed_hi;  // keys the targets of re-armed envs
  float radius;
  // SELECT (mt_shoot's commit): env i reads the plane its evaluation chose, tape + best[i] * cand_stride
  const int32_t* best;   // [n] or NULL
  int64_t cand_stride;   // elements between planes
};

// a tape row element: read once, so optionally non-temporal (wave-uniform choice)
template <bool R>
__device__ __forceinline__ float tape_load(const float* row, LaneOffset<R>& o, bool nt) {
  global_ptr<const float> p = (global_ptr<const float>)(uniform_row(row) + lane_offset(o));
  return nt ? __builtin_nontemporal_load(p) : *p;
}
// ... of the plane a lane chose for itself (SELECT): the one address of the kernel that is 64-bit per lane -- a plane may
// start anywhere in a (C, T, D, ld) block of any size.  These rows were read by the evaluation a launch earlier.
__device__ __forceinline__ float tape_load_plane(const float* row, uint64_t byte_off) {
  return *(global_ptr<const float>)(uniform_row(row) + byte_off);
}

// SELECT: the tape is a stack of planes r.cand_stride apart and env i follows plane r.best[i] (shoot_kernel's choice).
template <class Tbl, bool PREFETCH = false, bool SELECT = false>
__global__ __launch_bounds__(kBlock) void rollout_tape_kernel(const StepArgs a, const TapeArgs r) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [3K][kBlock]
  constexpr int D = Tbl::D;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  LaneOffset<true> o4{i * 4u}, o1{i};
  if (i >= a.n) return;  // (no block barrier and no wave-cooperative draw below)
  const int64_t ld = a.ld;
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);
  const TargetColumn<kBlock> tc{tile + threadIdx.x};
  const bool commit = r.dry_run == 0;  // (wave-uniform: a launch argument)
  const bool nt = r.nt_loads != 0;
  uint64_t plane = 0;  // byte offset of this env's column in its plane, read once
  if constexpr (SELECT) plane = (uint64_t)(uint32_t)ldr(r.best, o4) * (uint64_t)r.cand_stride * 4u + (uint64_t)i * 4u;
  auto row_load = [&](const float* row) { return SELECT ? tape_load_plane(row, plane) : tape_load(row, o4, nt); };

  const uint32_t all_alive = all_alive_mask(a.K);
  float g[D], cur[D];
#pragma unroll
  for (int j = 0; j < D; ++j) cur[j] = row_load(r.tape + (int64_t)j * r.tape_ld);
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = ldr(a.goals + j * ld, o4);
  uint32_t am = ldr(a.alive, o4);
  float total = ldr(a.total_reward, o4);
  uint32_t episode = r.auto_reset ? ldr(a.episodes, o4) : 0u;
  for (int k = 0; k < 3 * a.K; ++k) tc.row(k) = ldr(a.points + (int64_t)k * ld, o4);
  bool ended = false, dirty = false;
  float ret = 0.f;  // sum of this call's rewards, across re-arms
  PoseCache<D> pose;
  bool pose_valid = false;  // nothing known about the pose loaded from memory

  for (int s = 0; s < r.T; ++s) {
    const bool last = s == r.T - 1;  // (wave-uniform)
    float act[D], raw[D], el[3], e[3];
#pragma unroll
    for (int j = 0; j < D; ++j) raw[j] = cur[j];
    if (PREFETCH && !last) {
#pragma unroll
      for (int j = 0; j < D; ++j) cur[j] = row_load(r.tape + ((int64_t)(s + 1) * D + j) * r.tape_ld);
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) bad |= unusable_angle(raw[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) act[j] = bad ? g[j] : raw[j];  // the env holds its pose this step
    if (bad && commit) atomicAdd(a.bad_actions, 1u);          // ... and the pair is counted (mt_bad_action_count)

    const float zmin = route_kinematics<Tbl, 0, true, false>(t, a.S, a.inv_sm1, g, act, el, e, &pose, pose_valid, nullptr, false);
    pose_valid = true;
    const bool ground = zmin < 0.f;
    const bool out = last && commit;  // the step whose outputs MT_F_* keep
    if (out && a.zmin) str_stream(a.zmin, o4, zmin);

    uint32_t nam = am;
    for (int k = 0; k < a.K; ++k) {
      float x, y, z, dist = 0.f, rr = 0.f, th = 0.f;
      tc.get(k, x, y, z);
      if ((am >> k) & 1u) {
        if (out) observe_target(el, x, y, z, dist, rr, th);
        if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << k);
      } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {  // manytor.py:148
        tc.zero(k);
        dirty = true;
      }
      if (out) {
        float* orow = a.obs + (int64_t)(3 * k) * ld;
        str_stream(orow, o4, dist);
        str_stream(orow + ld, o4, rr);
        str_stream(orow + 2 * ld, o4, th);
      }
    }
    const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);
    bool done = (nam == 0u);
    if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;
    total += (float)rew;
    ret += (float)rew;
    am = nam;
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = act[j];
    if (r.reward_log) str_stream(r.reward_log + (int64_t)s * r.log_ld, o1, (int8_t)rew);
    if (r.done_log) str_stream(r.done_log + (int64_t)s * r.log_ld, o1, (uint8_t)(done ? 1 : 0));
    if (out) {
#pragma unroll
      for (int j = 0; j < D; ++j) str(a.actions + j * ld, o4, raw[j]);  // what mt_set_actions(row T - 1) would have left
#pragma unroll
      for (int q = 0; q < 3; ++q) str_stream(a.ee + q * ld, o4, e[q]);
      str_stream(a.reward, o4, rew);
      // 2 = "finished in this step and already re-armed below" (see rollout_kernel)
      str_stream(a.done, o1, (uint8_t)(done ? (r.auto_reset ? 2 : 1) : 0));
      const unsigned long long bits = __ballot(done);
      if ((threadIdx.x & 63) == 0) a.done_bits[i >> 6] = bits;
    }

    if (done && r.auto_reset) {  // re-arm, as in rollout_kernel (never in a dry run: the host refuses the combination)
      record_finished(a, i, episode, total);
      ended = true;
      total = 0.f;
      am = all_alive;
      episode += 1u;
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = 0.f;
      pose_valid = false;
      draw_targets(seed, env_id, episode, a.K, r.radius, [&](int k, float x, float y, float z) { tc.put(k, x, y, z); });
      dirty = true;
    }
    if (!PREFETCH && !last) {
#pragma unroll
      for (int j = 0; j < D; ++j) cur[j] = row_load(r.tape + ((int64_t)(s + 1) * D + j) * r.tape_ld);
    }
  }

  if (r.return_out) str_stream(r.return_out, o4, ret);
  if (!commit) return;
#pragma unroll
  for (int j = 0; j < D; ++j) str(a.goals + j * ld, o4, g[j]);
  str(a.alive, o4, am);
  str(a.total_reward, o4, total);
  if (ended) str(a.episodes, o4, episode);
  if (dirty)
    for (int k = 0; k < 3 * a.K; ++k) str(a.points + (int64_t)k * ld, o4, tc.row(k));
}

// ---------------------------------------------------------------------------
// rollout driven by an MLP policy (mt_rollout_policy): rollout_tape_kernel with the third action source -- at every step
// the env's observation at the pose it stands in goes through a small MLP whose output is the action.  State residency,
// step body, re-arm and write-back are the tape kernel's, on the same lanes (one env per lane, blocks of kBlock), so a
// call leaves what rollout_tape_kernel leaves for the logged actions, bit for bit.
//
// The observation frame of the current pose: after a step it is the `el` route_kinematics returned for the end pose (a
// held pose included: act == g); at step 0 it is computed as observe_kernel does, and after a re-arm it is the zero
// pose's, computed once in the prologue.
//
// The MLP.  Weights are wave-uniform and are read through the constant address space: scalar loads that feed the FMA's
// scalar operand, one s_load_dwordx8 per eight v_fmac.  The first layer is accumulated while the observation triples are
// produced (x is never live as a whole); hidden vectors are register arrays of the compile-time extent W (32 or 64):
//   first layer  acc[o] += W0[o][k] * x_k for every o of a block of eight outputs that the layer has (wave-uniform skip);
//                rows past the layer's width read its last row and are zeroed behind the activation
//   later layers a runtime loop over blocks of eight output rows, each a dot product over the statically indexed input
//                array in blocks of eight (a block past the layer's inputs is skipped; the one block that straddles them is
//                read element by element, so no word outside the row is ever loaded, whatever the widths, 1 included);
//                the eight results enter the output array by ROTATING it by eight, so after W / 8 iterations every
//                result sits at its own index and no register array is ever indexed dynamically
// A later layer whose input fills the extent takes a straight-line dot product, the same chain with no wave-uniform branch
// between the row's scalar loads and its FMAs (the same registers; the same form in the first layer spills SGPRs to
// scratch for RtTable<8> and is not taken).
// Accumulation: one fmaf chain per output, inputs in ascending order behind the bias.
// ---------------------------------------------------------------------------
struct PolicyArgs {
  const float* w[3];
  const float* b[3];
  int32_t n_in[3], n_out[3];  // per layer; n_in[0] = IN, n_out[L - 1] = D
  int32_t L, T;
  int32_t hidden_act, out_act;  // MT_ACT_*
  float out_scale, lo, hi;
  float sigma[MT_MAX_DOF];
  uint32_t draw, noisy, see_pose;
  float* action_log;  // [T * D][act_ld] or NULL
  int64_t act_ld;
  float* obs_log;  // [T * IN][obs_ld] or NULL
  int64_t obs_ld;
  int8_t* reward_log;  // as TapeArgs
  uint8_t* done_log;
  int64_t log_ld;
  float* return_out;
  uint32_t auto_reset, dry_run;
  uint32_t seed_lo, seed_hi;  // keys the noise stream and the targets of re-armed envs
  float radius;
  // mt_rollout_population: block b reads member b / blocks_per_member's weights, member_pitch floats behind the previous
  // member's in every w[l] and b[l] (a scalar computation: a block never straddles two members).  mt_rollout_policy: 1 and 0.
  uint32_t blocks_per_member;
  int64_t member_pitch;
};

using weight_ptr = __attribute__((address_space(4))) const float*;  // constant address space: uniform reads are scalar loads
__device__ __forceinline__ weight_ptr as_weights(const float* p) { return (weight_ptr)(uint64_t)p; }

// tanh(x) = 1 - 2 / (exp(2 x) + 1): v_exp_f32 and v_rcp_f32 (1 ulp each).  The argument is clamped to +-16 ahead of the
// multiply and the exponent capped (exp2(44) is finite: the build is -ffinite-math-only, no infinity may be formed, in the
// product either); at -16 the exponential is 2^-46 and the result is -1 exactly, as tanh is in fp32 from |x| = 9.1 on.
// A NaN goes through as it is (the clamp would drop it): the action it ends in is then unusable.
__device__ __forceinline__ bool policy_is_nan(float x) { return (__float_as_uint(x) & 0x7FFFFFFFu) > 0x7F800000u; }
__device__ __forceinline__ float policy_tanh(float x) {
  const float xc = fminf(fmaxf(x, -16.f), 16.f);
  const float e = __builtin_amdgcn_exp2f(fminf(xc * 2.8853900817779268f, 44.f));  // 2 log2(e) x
  const float t = 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
  return policy_is_nan(x) ? x : t;
}
__device__ __forceinline__ float policy_act(int act, float y) {  // (act is wave-uniform)
  if (act == MT_ACT_TANH) return policy_tanh(y);
  if (act == MT_ACT_RELU) return ((__float_as_uint(y) >> 31) && !policy_is_nan(y)) ? 0.f : y;  // a NaN of either sign stays
  return y;
}

// acc[o] += W[o][k + q] * x[q], q < NX, for the first layer's outputs o (n_out <= NOUT of them)
template <int NOUT, int NX>
__device__ __forceinline__ void policy_feed(float (&acc)[NOUT], weight_ptr w, int n_in, int n_out, int k, const float (&x)[NX]) {
#pragma unroll
  for (int o0 = 0; o0 < NOUT; o0 += 8) {
    if (o0 < n_out) {
#pragma unroll
      for (int o = o0; o < o0 + 8 && o < NOUT; ++o) {
        const weight_ptr row = w + (int64_t)min(o, n_out - 1) * n_in + k;
#pragma unroll
        for (int q = 0; q < NX; ++q) acc[o] = __builtin_fmaf(row[q], x[q], acc[o]);
      }
    }
  }
}
// the first layer's accumulators before the first input: the bias
template <int NOUT>
__device__ __forceinline__ void policy_bias(float (&acc)[NOUT], weight_ptr b, int n_out) {
#pragma unroll
  for (int o = 0; o < NOUT; ++o) acc[o] = b[min(o, n_out - 1)];
}
// ... and behind the last one: the activation, zeros past the layer's width
template <int NOUT>
__device__ __forceinline__ void policy_finish(float (&acc)[NOUT], int act, int n_out) {
#pragma unroll
  for (int o = 0; o < NOUT; ++o) acc[o] = o < n_out ? policy_act(act, acc[o]) : 0.f;
}
// b + W[row][0 .. n_in) . h: whole blocks of eight as they are, the block that straddles n_in element by element
template <int W>
__device__ __forceinline__ float policy_dot(weight_ptr row, float bias, int n_in, const float (&h)[W]) {
  float acc = bias;
  if (n_in == W) {  // a full row: straight-line, no wave-uniform branch between the row's scalar loads and its FMAs
#pragma unroll
    for (int k = 0; k < W; ++k) acc = __builtin_fmaf(row[k], h[k], acc);
    return acc;
  }
#pragma unroll
  for (int k0 = 0; k0 < W; k0 += 8) {
    if (k0 + 8 <= n_in) {
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = __builtin_fmaf(row[k0 + q], h[k0 + q], acc);
    } else if (k0 < n_in) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k0 + q < n_in) acc = __builtin_fmaf(row[k0 + q], h[k0 + q], acc);
    }
  }
  return acc;
}
// a hidden layer behind the first: out = act(W in + b), n_out <= W outputs, zeros past them
template <int W>
__device__ __forceinline__ void policy_hidden(weight_ptr w, weight_ptr b, int n_in, int n_out, int act, const float (&in)[W],
                                              float (&out)[W]) {
#pragma unroll 1
  for (int o0 = 0; o0 < W; o0 += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int o = o0 + q;
      v[q] = 0.f;
      if (o < n_out) v[q] = policy_act(act, policy_dot<W>(w + (int64_t)o * n_in, b[o], n_in, in));
    }
#pragma unroll
    for (int o = 0; o < W - 8; ++o) out[o] = out[o + 8];
#pragma unroll
    for (int q = 0; q < 8; ++q) out[W - 8 + q] = v[q];
  }
}

// mt_rollout_actor_critic: what rollout_policy_kernel<.., AC = true> reads on top of PolicyArgs.  The critic is a second MLP
// of the policy's shape with one output, on the same x; logp is policy_eval_kernel's sequence on the mean and the action
// the step already holds.
struct ActorCriticArgs : PolicyArgs {
  const float* cw[3];
  const float* cb[3];
  int32_t c_n_in[3], c_n_out[3];  // per layer; c_n_in[0] = IN, c_n_out[CL - 1] = 1
  int32_t CL;                     // the critic's layers, 0 = no critic
  int32_t c_hidden_act, c_out_act;
  float c_out_scale;
  float inv_var[MT_MAX_DOF];  // the fp32 nearest to 1 / sigma_j^2 (read with logp_log)
  float* logp_log;            // [T][logp_ld] or NULL
  int64_t logp_ld;
  float* value_log;  // [T][value_ld] or NULL
  int64_t value_ld;
  float* last_value;  // [n] or NULL
};
template <bool AC>
struct PolicyRolloutMode {
  using Args = PolicyArgs;
};
template <>
struct PolicyRolloutMode<true> {
  using Args = ActorCriticArgs;
};

// The critic on the x a lane parked in its LDS column (x_k = xcol[k kBlock]): policy_eval_kernel's forward pass with one
// output, the same helpers over the same triples in the same order, so the value has mt_policy_eval's bits.
template <int W>
__device__ __forceinline__ float critic_value(const ActorCriticArgs& r, const float* xcol, int K, int n_pose) {
  const int L = r.CL, IN = r.c_n_in[0];
  const weight_ptr w0 = as_weights(r.cw[0]), b0 = as_weights(r.cb[0]);
  const weight_ptr wl = as_weights(r.cw[L - 1]), bl = as_weights(r.cb[L - 1]);  // the output layer
  auto first_layer = [&](auto& acc, int n_out) {
    policy_bias(acc, b0, n_out);
    for (int k = 0; k < K; ++k) {
      float tri[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) tri[q] = xcol[(3 * k + q) * kBlock];
      policy_feed(acc, w0, IN, n_out, 3 * k, tri);
    }
    for (int j = 0; j < n_pose; ++j) {
      const float xj[1] = {xcol[(3 * K + j) * kBlock]};
      policy_feed(acc, w0, IN, n_out, 3 * K + j, xj);
    }
  };
  float y;
  if (L == 1) {
    float y1[1];
    first_layer(y1, 1);
    y = y1[0];
  } else {
    float h0[W];
    first_layer(h0, r.c_n_out[0]);
    policy_finish(h0, r.c_hidden_act, r.c_n_out[0]);
    if (L == 2) {
      y = policy_dot<W>(wl, bl[0], r.c_n_in[1], h0);
    } else {
      float h1[W];
#pragma unroll
      for (int o = 0; o < W; ++o) h1[o] = 0.f;
      policy_hidden<W>(as_weights(r.cw[1]), as_weights(r.cb[1]), r.c_n_in[1], r.c_n_out[1], r.c_hidden_act, h0, h1);
      y = policy_dot<W>(wl, bl[0], r.c_n_in[2], h1);
    }
  }
  return r.c_out_scale * policy_act(r.c_out_act, y);
}

// the observation frame's origin at pose g, as observe_kernel computes it
template <int D>
__device__ __forceinline__ void pose_obs_frame(const DhConst& dh, const float (&g)[D], float (&el)[3]) {
  float s[D], c[D], p[D][3], e_unused[3];
#pragma unroll
  for (int j = 0; j < D; ++j) sincos_deg_off(g[j], dh.off_deg[j], s[j], c[j]);
  const RtTableF<D> t{dh};
  chain_all<RtTableF<D>>(s, c, t, p);
  pick_frames<RtTableF<D>>(t, p, el, e_unused);
}

// AC (mt_rollout_actor_critic): the same launch also writes log pi(a_t | x_t) and the critic's V(x_t) per step and V(x_T)
// at the end.  x is parked in a lane-private LDS column behind the target tile while it streams through the policy's first
// layer, and the critic runs from there once the policy's hidden vectors are dead: no barrier, no second observation, and
// no more than the policy's own two register arrays live at a time.
template <class Tbl, int W, bool AC = false>
__global__ __launch_bounds__(kBlock) void rollout_policy_kernel(const StepArgs a, const typename PolicyRolloutMode<AC>::Args r) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [3K][kBlock]; AC with a critic: [IN][kBlock] behind it
  constexpr int D = Tbl::D;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  LaneOffset<true> o4{i * 4u}, o1{i};
  if (i >= a.n) return;  // (no block barrier and no wave-cooperative draw below)
  const int64_t ld = a.ld;
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);
  const TargetColumn<kBlock> tc{tile + threadIdx.x};
  const bool commit = r.dry_run == 0;  // (wave-uniform: a launch argument)
  const int L = r.L, IN = r.n_in[0];
  const int64_t member = (int64_t)(blockIdx.x / r.blocks_per_member) * r.member_pitch;  // (block-uniform; 0 for one policy)
  const weight_ptr w0 = as_weights(r.w[0]) + member, b0 = as_weights(r.b[0]) + member;
  const weight_ptr wl = as_weights(r.w[L - 1]) + member, bl = as_weights(r.b[L - 1]) + member;  // the output layer (the first one when L == 1)

  const uint32_t all_alive = all_alive_mask(a.K);
  float g[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = ldr(a.goals + j * ld, o4);
  uint32_t am = ldr(a.alive, o4);
  float total = ldr(a.total_reward, o4);
  uint32_t episode = r.auto_reset ? ldr(a.episodes, o4) : 0u;
  for (int k = 0; k < 3 * a.K; ++k) tc.row(k) = ldr(a.points + (int64_t)k * ld, o4);
  bool ended = false, dirty = false;
  float ret = 0.f;  // sum of this call's rewards, across re-arms
  PoseCache<D> pose;
  bool pose_valid = false;  // nothing known about the pose loaded from memory
  float el_cur[3], el_zero[3] = {0.f, 0.f, 0.f};
  pose_obs_frame<D>(a.dh, g, el_cur);
  if (r.auto_reset) {
    float zero[D];
#pragma unroll
    for (int j = 0; j < D; ++j) zero[j] = 0.f;
    pose_obs_frame<D>(a.dh, zero, el_zero);
  }

  // the policy's input at the state a step starts from, handed to `use` piece by piece (row s of `olog` gets it, if given)
  auto each_x = [&](int s, float* olog, auto&& use) {
    for (int k = 0; k < a.K; ++k) {
      float x, y, z, tri[3] = {0.f, 0.f, 0.f};
      tc.get(k, x, y, z);
      if ((am >> k) & 1u) observe_target(el_cur, x, y, z, tri[0], tri[1], tri[2]);
      if (olog) {
        float* orow = olog + ((int64_t)s * IN + 3 * k) * r.obs_ld;
#pragma unroll
        for (int q = 0; q < 3; ++q) str_stream(orow + q * r.obs_ld, o4, tri[q]);
      }
      use(3 * k, tri);
    }
    if (r.see_pose) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        if (olog) str_stream(olog + ((int64_t)s * IN + 3 * a.K + j) * r.obs_ld, o4, g[j]);
        const float xj[1] = {g[j]};
        use(3 * a.K + j, xj);
      }
    }
  };
  // AC: rows k .. of the lane's x column in LDS (written and read by this lane only)
  float* const xcol = tile + 3 * a.K * kBlock + threadIdx.x;
  auto park = [&](int k, const auto& x) {
    constexpr int NX = sizeof(x) / sizeof(float);
#pragma unroll
    for (int q = 0; q < NX; ++q) xcol[(k + q) * kBlock] = x[q];
  };
  // ... streamed into the first layer's accumulators
  auto first_layer = [&](auto& acc, int n_out, int s) {
    policy_bias(acc, b0, n_out);
    each_x(s, r.obs_log, [&](int k, const auto& x) {
      policy_feed(acc, w0, IN, n_out, k, x);
      if constexpr (AC) {
        if (r.CL) park(k, x);
      }
    });
  };

  for (int s = 0; s < r.T; ++s) {
    const bool last = s == r.T - 1;  // (wave-uniform)
    float act[D], raw[D], el[3], e[3];
    {  // observe -> MLP -> raw action
      float y[D];
      if (L == 1) {
        first_layer(y, D, s);
      } else {
        float h0[W];
        first_layer(h0, r.n_out[0], s);
        policy_finish(h0, r.hidden_act, r.n_out[0]);
        if (L == 2) {
#pragma unroll
          for (int j = 0; j < D; ++j) y[j] = policy_dot<W>(wl + (int64_t)j * r.n_in[1], bl[j], r.n_in[1], h0);
        } else {
          float h1[W];
#pragma unroll
          for (int o = 0; o < W; ++o) h1[o] = 0.f;
          policy_hidden<W>(as_weights(r.w[1]) + member, as_weights(r.b[1]) + member, r.n_in[1], r.n_out[1], r.hidden_act, h0, h1);
#pragma unroll
          for (int j = 0; j < D; ++j) y[j] = policy_dot<W>(wl + (int64_t)j * r.n_in[2], bl[j], r.n_in[2], h1);
        }
      }
      [[maybe_unused]] float lp = 0.f;  // AC: policy_eval_kernel's chain over (a_j - mu_j)^2 / sigma_j^2
      uint32_t nw[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      if (r.noisy) {
        const u32x4 n0 = stream_block(seed, env_id, kTagPolicy, r.draw, plan_minor(0u, 0u, (uint32_t)s));
        nw[0] = n0.x, nw[1] = n0.y, nw[2] = n0.z, nw[3] = n0.w;
        if constexpr (D > 4) {
          const u32x4 n1 = stream_block(seed, env_id, kTagPolicy, r.draw, plan_minor(0u, 1u, (uint32_t)s));
          nw[4] = n1.x, nw[5] = n1.y, nw[6] = n1.z, nw[7] = n1.w;
        }
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        float v = r.out_scale * policy_act(r.out_act, y[j]);
        [[maybe_unused]] const float mu = v;
        if (r.noisy && r.sigma[j] > 0.f) {
          const float sz = r.sigma[j] * plan_noise(nw[j]);
          v = v + sz;
        }
        raw[j] = unusable_angle(v) ? v : fminf(fmaxf(v, r.lo), r.hi);
        if (r.action_log) str_stream(r.action_log + ((int64_t)s * D + j) * r.act_ld, o4, raw[j]);
        if constexpr (AC) {
          const float e = raw[j] - mu;
          const float d = e * r.inv_var[j];
          lp = __builtin_fmaf(e, d, lp);
        }
      }
      if constexpr (AC) {
        if (r.logp_log) {
          bool unusable = false;
#pragma unroll
          for (int j = 0; j < D; ++j) unusable |= unusable_angle(raw[j]);
          str_stream(r.logp_log + (int64_t)s * r.logp_ld, o4, unusable ? 0.f : -0.5f * lp);
        }
      }
    }
    if constexpr (AC) {  // V(x_s): the policy's h0 / h1 are dead, x sits in the lane's LDS column
      if (r.value_log) str_stream(r.value_log + (int64_t)s * r.value_ld, o4, critic_value<W>(r, xcol, a.K, IN - 3 * a.K));
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < D; ++j) bad |= unusable_angle(raw[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) act[j] = bad ? g[j] : raw[j];  // the env holds its pose this step
    if (bad && commit) atomicAdd(a.bad_actions, 1u);          // ... and the pair is counted (mt_bad_action_count)

    const float zmin = route_kinematics<Tbl, 0, true, false>(t, a.S, a.inv_sm1, g, act, el, e, &pose, pose_valid, nullptr, false);
    pose_valid = true;
    const bool ground = zmin < 0.f;
    const bool out = last && commit;  // the step whose outputs MT_F_* keep
    if (out && a.zmin) str_stream(a.zmin, o4, zmin);

    uint32_t nam = am;
    for (int k = 0; k < a.K; ++k) {
      float x, y, z, dist = 0.f, rr = 0.f, th = 0.f;
      tc.get(k, x, y, z);
      if ((am >> k) & 1u) {
        if (out) observe_target(el, x, y, z, dist, rr, th);
        if (within_box(e, x, y, z, a.tol)) nam &= ~(1u << k);
      } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {  // manytor.py:148
        tc.zero(k);
        dirty = true;
      }
      if (out) {
        float* orow = a.obs + (int64_t)(3 * k) * ld;
        str_stream(orow, o4, dist);
        str_stream(orow + ld, o4, rr);
        str_stream(orow + 2 * ld, o4, th);
      }
    }
    const int32_t rew = ground ? -1 : ((nam != am) ? 1 : 0);
    bool done = (nam == 0u);
    if (a.flags & MT_FLAG_TERMINATE_ON_GROUND) done |= ground;
    total += (float)rew;
    ret += (float)rew;
    am = nam;
#pragma unroll
    for (int j = 0; j < D; ++j) g[j] = act[j];
#pragma unroll
    for (int q = 0; q < 3; ++q) el_cur[q] = el[q];
    if (r.reward_log) str_stream(r.reward_log + (int64_t)s * r.log_ld, o1, (int8_t)rew);
    if (r.done_log) str_stream(r.done_log + (int64_t)s * r.log_ld, o1, (uint8_t)(done ? 1 : 0));
    if (out) {
#pragma unroll
      for (int j = 0; j < D; ++j) str(a.actions + j * ld, o4, raw[j]);  // what mt_set_actions(row T - 1) would have left
#pragma unroll
      for (int q = 0; q < 3; ++q) str_stream(a.ee + q * ld, o4, e[q]);
      str_stream(a.reward, o4, rew);
      // 2 = "finished in this step and already re-armed below" (see rollout_kernel)
      str_stream(a.done, o1, (uint8_t)(done ? (r.auto_reset ? 2 : 1) : 0));
      const unsigned long long bits = __ballot(done);
      if ((threadIdx.x & 63) == 0) a.done_bits[i >> 6] = bits;
    }

    if (done && r.auto_reset) {  // re-arm, as in rollout_kernel (never in a dry run: the host refuses the combination)
      record_finished(a, i, episode, total);
      ended = true;
      total = 0.f;
      am = all_alive;
      episode += 1u;
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = 0.f;
#pragma unroll
      for (int q = 0; q < 3; ++q) el_cur[q] = el_zero[q];
      pose_valid = false;
      draw_targets(seed, env_id, episode, a.K, r.radius, [&](int k, float x, float y, float z) { tc.put(k, x, y, z); });
      dirty = true;
    }
  }

  if (r.return_out) str_stream(r.return_out, o4, ret);
  if constexpr (AC) {  // V(x_T): the input a step T would start from (after a re-arm in the last step: the zero pose, new targets)
    if (r.last_value) {
      each_x(r.T, (float*)nullptr, park);
      str_stream(r.last_value, o4, critic_value<W>(r, xcol, a.K, IN - 3 * a.K));
    }
  }
  if (!commit) return;
#pragma unroll
  for (int j = 0; j < D; ++j) str(a.goals + j * ld, o4, g[j]);
  str(a.alive, o4, am);
  str(a.total_reward, o4, total);
  if (ended) str(a.episodes, o4, episode);
  if (dirty)
    for (int k = 0; k < 3 * a.K; ++k) str(a.points + (int64_t)k * ld, o4, tc.row(k));
}

// ---------------------------------------------------------------------------
// An evolution-strategies generation (mt_es_sample, mt_es): the planners' three levels in parameter space.  The scoring is
// rollout_policy_kernel with a member's row as the weights (PolicyArgs::member_pitch); the kernels here are what surrounds
// it, and none of them touches a handle's state.
//   es_sample_kernel  a thread per (parameter i, pair p): eps from word i & 3 of the pair's Philox block i >> 2, rows 2p and
//                     2p + 1 written as theta + sigma * eps and theta - sigma * eps (a multiply, then an add or a subtract)
//   es_sums_kernel    a block per member: the member's G returns summed in int64 (integer-valued floats: the order is
//                     free) -> sums[m], fitness[m]
//   es_update_kernel  every block first ranks for itself: the M sums into LDS, the centred mid-ranks (an O(M^2) count over
//                     LDS broadcast reads) or the raw sums as the pair differences c_2p - c_2p+1, kept in LDS (block 0 also
//                     writes them out, and best); then a thread per parameter: A_i = sum_p coeff[p] * (bytesum(p, i) - 510)
//                     in int64, the noise regenerated; grad_i = (float)A_i * scale; theta_i += lr * grad_i.  Ranking once per
//                     block costs M^2 / 512 compare pairs per thread and saves a launch and a serial block.
// ---------------------------------------------------------------------------
constexpr int kEsMaxMembers = 4096;  // es_update_kernel keeps M sums and M / 2 coefficients in LDS: 48 KB
struct EsArgs {
  float* theta;  // [P]: read by the sample, updated in place by the update when `inplace`
  float* pop;    // [M][pitch]
  int64_t P, pitch;
  int32_t M;
  float sigma;
  uint32_t draw, seed_lo, seed_hi;
  const float* returns;  // [M * G]
  int64_t G;
  float inv_g, scale, lr;
  uint32_t raw, inplace;
  long long* coeff;  // [M / 2]: c_2p - c_2p+1
  long long* sums;   // [M]: S_m (NULL: fitness only)
  float* fitness;    // [M]
  int32_t* best;     // [1]
  float* grad;       // [P]
};

// word i & 3 of pair p's block i >> 2 of the ES stream
__device__ __forceinline__ uint32_t es_word(uint64_t seed, uint32_t p, uint32_t draw, int64_t i) {
  const u32x4 b = stream_block(seed, (uint64_t)p, kTagES, draw, (uint32_t)(i >> 2));
  const uint32_t q = (uint32_t)i & 3u;
  return q == 0u ? b.x : q == 1u ? b.y : q == 2u ? b.z : b.w;
}

inline __global__ __launch_bounds__(kBlock) void es_sample_kernel(const EsArgs r) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.P) return;
  const uint32_t p = blockIdx.y;
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  const float th = r.theta[i];
  const float se = r.sigma * plan_noise(es_word(seed, p, r.draw, i));
  float* row = r.pop + (int64_t)(2u * p) * r.pitch + i;
  row[0] = th + se;
  row[r.pitch] = th - se;
}

inline __global__ __launch_bounds__(kBlock) void es_sums_kernel(const EsArgs r) {
  __shared__ long long part[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x;  // (the grid is M blocks)
  const float* row = r.returns + (int64_t)m * r.G;
  long long acc = 0;
  for (int64_t k = threadIdx.x; k < r.G; k += kBlock) acc += (long long)(int32_t)row[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += part[w];
    if (r.sums) r.sums[m] = s;
    if (r.fitness) r.fitness[m] = (float)s * r.inv_g;
  }
}

inline __global__ __launch_bounds__(kBlock) void es_update_kernel(const EsArgs r) {
  extern __shared__ __attribute__((aligned(16))) long long es_lds[];  // [M] sums, [M / 2] coefficients
  const int M = r.M;
  long long* es_sum = es_lds;
  long long* coeff = es_lds + M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = threadIdx.x; m < M; m += kBlock) es_sum[m] = r.sums[m];
  __syncthreads();
  for (int p = threadIdx.x; p < M / 2; p += kBlock) {
    const long long s0 = es_sum[2 * p], s1 = es_sum[2 * p + 1];
    long long c0 = s0, c1 = s1;
    if (!r.raw) {  // centred mid-ranks: 2 #{S_j < S_m} + #{j != m : S_j == S_m}
      c0 = c1 = -1;  // (j == m counts itself once below)
      for (int j = 0; j < M; ++j) {
        const long long s = es_sum[j];
        c0 += s < s0 ? 2 : (s == s0 ? 1 : 0);
        c1 += s < s1 ? 2 : (s == s1 ? 1 : 0);
      }
    }
    coeff[p] = c0 - c1;
    if (blockIdx.x == 0) r.coeff[p] = c0 - c1;
  }
  if (blockIdx.x == 0 && r.best && wave == 0) {  // the lowest m with the largest sum
    long long bs = es_sum[lane < M ? lane : 0];
    int bm = lane < M ? lane : 0;
    for (int m = lane + 64; m < M; m += 64)
      if (es_sum[m] > bs) bs = es_sum[m], bm = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long os = __shfl_down(bs, off);
      const int om = __shfl_down(bm, off);
      if (os > bs || (os == bs && om < bm)) bs = os, bm = om;
    }
    if (lane == 0) r.best[0] = bm;
  }
  __syncthreads();  // (the last barrier: tail lanes leave behind it)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.P) return;
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  long long acc = 0;
  for (int p = 0; p < M / 2; ++p)
    acc += coeff[p] * (long long)noise_byte_sum(es_word(seed, (uint32_t)p, r.draw, i));
  const float g = (float)acc * r.scale;
  r.grad[i] = g;
  if (r.inplace) {
    const float d = r.lr * g;
    r.theta[i] = r.theta[i] + d;
  }
}

// ---------------------------------------------------------------------------
// The weighted log-likelihood gradient of the MLP policy (mt_policy_grad) and the reward-to-go that usually weights it
// (mt_reward_to_go).  Neither depends on the DH table nor touches a handle's state.
//
// policy_grad_kernel<W>: one sample (t, i) per lane, a block per tile of kBlock consecutive envs of one step; the grid is
// bounded and block b takes tiles b, b + gridDim.x, ... in that order, its sums kept in registers across them.
//   forward   policy_feed / policy_bias / policy_finish / policy_hidden / policy_dot as rollout_policy_kernel calls them:
//             the same fmaf chains, so the same mu bit for bit.  x is streamed from obs (never live as a whole); the hidden
//             vectors stay in registers for the backward pass.
//   backward  delta_L = c (a - mu) / sigma^2 out_scale out_act';  delta_l = (W_l+1^T delta_l+1) * act'(h_l): the transposed
//             product walks the rows o of W_l+1 (scalar loads of eight, the straddling block element by element, as
//             policy_dot) and takes delta_o from the front of its array, which is ROTATED by eight per block of rows: no
//             register array is indexed dynamically.
//   reduction dW_l[o][k] = sum over samples of delta_l[o] h_l[k], db_l[o] = sum of delta_l[o]: per layer, the four waves
//             of the block put their 64 samples' delta and h into LDS one after the other (sample-major images) and ALL
//             256 threads add that wave's samples, in sample order, to the (W / 16)^2 outputs each of them owns (thread
//             (to, tk) = (tid / 16, tid % 16): rows to W/16 .., columns tk W/16 .. of every W-column chunk of the input).
//             Plain VALU fmaf over LDS broadcast reads; the matrix cores are not used.
//   skipped   a lane whose sample is skipped (c == 0, an unusable a_j, i >= n_envs) loads neither x nor a and runs with
//             x = 0, a = 0, c = 0: every delta is then +-0, and adds nothing.
// Each block writes its sums to its row of the (blocks, P + 1) partials (word P: the loss); policy_grad_reduce_kernel adds
// the rows in ascending block order and applies scale once.
//
// policy_grad_kernel<W, NCH0, 1>, the PPO mode (mt_ppo_grad): a compile-time mode, so the two-parameter instantiations are
// the text they were.  `coef` holds the advantages; the lane carries A = weight * adv where the plain mode carries c, and
// once the j loop has finished lp it forms x, ratio and the clip decision, c = clipped ? 0 : ratio * A, and only then
// dl[j] = ((c * d[j]) * out_scale) * slope[j]: the plain mode's expression on the same d and slope, so the deltas -- and
// everything behind them -- are mt_policy_grad's for coef = c.  (e, d and the slope are formed a second time from y[j], by
// the same expressions and so with the same bits, rather than kept across the ratio: kept, they are 3 D live registers
// more and the W = 64 instantiations spill 64 and 132 bytes per lane to scratch; formed twice, none does.)  The lane also keeps the objective (in `loss`) and, in LDS
// words of its own (ppo_lane_sums), the KL sum, D sigma sums and two counters across its tiles; they are added in thread
// order behind the tile loop and go to the kPpoExtras words behind word P of the block's row, which
// ppo_grad_reduce_kernel adds like the others (the two counts as integers).
// ---------------------------------------------------------------------------
struct PolicyGradArgs {
  const float* w[3];
  const float* b[3];
  int32_t n_in[3], n_out[3];  // per layer, as PolicyArgs
  int64_t off[3];             // layer l's W in the flat gradient; its bias follows the matrix
  int32_t L, T, K, D;
  int32_t hidden_act, out_act;
  float out_scale;
  float inv_var[MT_MAX_DOF];  // the fp32 nearest to 1 / sigma_j^2
  uint32_t see_pose;
  const float* obs;  // [T * IN][obs_ld]
  int64_t obs_ld;
  const float* action;  // [T * D][act_ld]
  int64_t act_ld;
  const float* coef;  // [T][coef_ld]
  int64_t coef_ld;
  int64_t n;                      // envs
  int64_t tiles_per_step, tiles;  // tiles = T * tiles_per_step
  int64_t P;
  float* partials;  // [blocks][P + 1]
  int32_t blocks;
  float scale;
  float* grad;  // [P]
  float* loss;  // [1] or NULL
};
// the words behind the loss in a block's row of mt_ppo_grad's partials: kl, MT_MAX_DOF sigma sums, used, clipped
constexpr int kPpoExtras = MT_PPO_EXTRA_WORDS;
constexpr float kLog2e = 1.44269504088896340736f;
struct PpoGradArgs : PolicyGradArgs {  // coef / coef_ld: the advantages
  const float* old_logp;  // [T][old_ld]
  int64_t old_ld;
  const float* weight;  // [T][weight_ld] or NULL
  int64_t weight_ld;
  float lo, hi, shift;  // the fp32 nearest to 1 -+ clip; log_ratio_shift
  uint32_t clipping;    // clip > 0
  float* ratio;         // [T][ratio_ld] or NULL
  int64_t ratio_ld;
  float* coef_out;  // [T][coefo_ld] or NULL
  int64_t coefo_ld;
  float* sigma_grad;  // [D] or NULL
  float* kl;          // [1] or NULL
  long long* count;   // [2] or NULL
};
template <int MODE>
struct PolicyGradMode {
  using Args = PolicyGradArgs;
};
template <>
struct PolicyGradMode<1> {
  using Args = PpoGradArgs;
};
// A lane's extra sums over its tiles, word q of thread tid at [q kBlock + tid]: in LDS, not in registers -- the kernel has
// none to spare (profiles/ppo_grad_kernel_resources.md), and only the lane itself touches its words until the block adds
// them up.  Only the PPO instantiations reach this function.
__device__ __forceinline__ float* ppo_lane_sums() {
  __shared__ float sums[kPpoExtras * kBlock];
  return sums;
}

constexpr int kPolicyGradMaxIn = 3 * MT_MAX_TARGETS + MT_MAX_DOF;  // 104
constexpr int kPolicyGradOutCols = 128;  // the output layer's tile: 8 rows x 32 threads x 4 columns
static_assert(kPolicyGradOutCols >= kPolicyGradMaxIn && MT_MAX_DOF <= 8, "the output layer's gradient fits its tile");
// W: the extent of the hidden register arrays; NCH0: the W-column chunks of x a hidden first layer's gradient is kept in
// (the host picks the smallest compiled pair that holds the policy: NCH0 * W >= IN)
template <int W, int NCH0>
struct PolicyGradShape {
  static constexpr int TO = W / 16;                 // a thread's outputs of a hidden layer: TO rows x TO columns per chunk
  static constexpr int AP = W + 4;                  // pitch of the delta image [64][AP]
  static constexpr int BP = NCH0 * W + 4;           // pitch of the input image [64][BP]
  static constexpr int kWords = 64 * (AP + BP);
  static_assert(kWords >= kBlock, "the loss is summed through the same words");
};
template <int W, int NCH>
struct PolicyGradTile {  // what one thread owns of a hidden layer's gradient
  float w[NCH][W / 16][W / 16];
  float b[W / 16];
};
struct PolicyGradOutTile {  // ... and of the output layer's: row tid / 32, columns 4 (tid % 32) ..
  float w[4];
  float b;
};

__device__ __forceinline__ float policy_act_slope(int act, float h) {  // from the forward VALUE h (act is wave-uniform)
  if (act == MT_ACT_TANH) {
    const float hh = h * h;
    return 1.f - hh;
  }
  if (act == MT_ACT_RELU) return h > 0.f ? 1.f : 0.f;
  return 1.f;
}

// out[k] = sum over o < n_out of W[o][k] delta[o], k < n_in (0 past it); delta has the static extent ND >= n_out
template <int ND, int W>
__device__ __forceinline__ void policy_backprop(weight_ptr w, int n_in, int n_out, float (&delta)[ND], float (&out)[W]) {
#pragma unroll
  for (int k = 0; k < W; ++k) out[k] = 0.f;
#pragma unroll 1
  for (int o0 = 0; o0 < ND; o0 += 8) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (o0 + q < n_out) {
        const weight_ptr row = w + (int64_t)(o0 + q) * n_in;
        const float d = delta[q];
#pragma unroll
        for (int k0 = 0; k0 < W; k0 += 8) {
          if (k0 + 8 <= n_in) {
#pragma unroll
            for (int e = 0; e < 8; ++e) out[k0 + e] = __builtin_fmaf(row[k0 + e], d, out[k0 + e]);
          } else if (k0 < n_in) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (k0 + e < n_in) out[k0 + e] = __builtin_fmaf(row[k0 + e], d, out[k0 + e]);
          }
        }
      }
    }
    if constexpr (ND > 8) {  // the next eight to the front; after ND / 8 turns the array is as it was
      float head[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) head[q] = delta[q];
#pragma unroll
      for (int o = 0; o < ND - 8; ++o) delta[o] = delta[o + 8];
#pragma unroll
      for (int q = 0; q < 8; ++q) delta[ND - 8 + q] = head[q];
    }
  }
}

// a lane's vector into its row of a sample-major LDS image
template <int N>
__device__ __forceinline__ void policy_grad_put(float* row, const float (&v)[N]) {
#pragma unroll
  for (int o = 0; o < N; ++o) row[o] = v[o];
}

// the 64 samples of the images, in sample order, into the outputs this thread owns
template <int AP, int BP, int W, int NCH>
__device__ __forceinline__ void policy_grad_accumulate(PolicyGradTile<W, NCH>& g, const float* A, const float* B, int n_in, int n_out) {
  constexpr int TO = W / 16;
  const int to = threadIdx.x >> 4, tk = threadIdx.x & 15;
  if (TO * to < n_out) {
    const float* a = A + TO * to;
    const float* b = B + TO * tk;
#pragma unroll 2
    for (int s = 0; s < 64; ++s) {
      float d[TO];
#pragma unroll
      for (int i = 0; i < TO; ++i) d[i] = a[s * AP + i];
#pragma unroll
      for (int i = 0; i < TO; ++i) g.b[i] = g.b[i] + d[i];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (ch * W < n_in) {
          float x[TO];
#pragma unroll
          for (int j = 0; j < TO; ++j) x[j] = b[s * BP + ch * W + j];
#pragma unroll
          for (int i = 0; i < TO; ++i)
#pragma unroll
            for (int j = 0; j < TO; ++j) g.w[ch][i][j] = __builtin_fmaf(d[i], x[j], g.w[ch][i][j]);
        }
      }
    }
  }
}
template <int AP, int BP>
__device__ __forceinline__ void policy_grad_accumulate(PolicyGradOutTile& g, const float* A, const float* B, int n_in, int n_out) {
  const int to = threadIdx.x >> 5, tk = threadIdx.x & 31;
  if (to < n_out && 4 * tk < n_in) {  // (columns up to the next multiple of four: the images are written that far)
    const float* a = A + to;
    const float* b = B + 4 * tk;
#pragma unroll 2
    for (int s = 0; s < 64; ++s) {
      const float d = a[s * AP];
      g.b = g.b + d;
#pragma unroll
      for (int j = 0; j < 4; ++j) g.w[j] = __builtin_fmaf(d, b[s * BP + j], g.w[j]);
    }
  }
}

template <int W, int NCH>
__device__ __forceinline__ void policy_grad_store(const PolicyGradTile<W, NCH>& g, float* part, int n_in, int n_out) {
  constexpr int TO = W / 16;
  const int to = threadIdx.x >> 4, tk = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < TO; ++i) {
    const int o = TO * to + i;
    if (o < n_out) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int j = 0; j < TO; ++j) {
          const int k = ch * W + TO * tk + j;
          if (k < n_in) part[(int64_t)o * n_in + k] = g.w[ch][i][j];
        }
      if (tk == 0) part[(int64_t)n_out * n_in + o] = g.b[i];
    }
  }
}
__device__ __forceinline__ void policy_grad_store(const PolicyGradOutTile& g, float* part, int n_in, int n_out) {
  const int to = threadIdx.x >> 5, tk = threadIdx.x & 31;
  if (to < n_out) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * tk + j < n_in) part[(int64_t)to * n_in + 4 * tk + j] = g.w[j];
    if (tk == 0) part[(int64_t)n_out * n_in + to] = g.b;
  }
}

template <int W, int NCH0, int MODE = 0>
__global__ __launch_bounds__(kBlock) void policy_grad_kernel(const typename PolicyGradMode<MODE>::Args r) {
  using S = PolicyGradShape<W, NCH0>;
  __shared__ __attribute__((aligned(16))) float img[S::kWords];
  float* const A = img;
  float* const B = img + 64 * S::AP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = r.L, IN = r.n_in[0], D = r.D;
  const weight_ptr w0 = as_weights(r.w[0]), b0 = as_weights(r.b[0]);
  const weight_ptr wl = as_weights(r.w[L - 1]), bl = as_weights(r.b[L - 1]);  // the output layer
  float* const arow = A + lane * S::AP;
  float* const brow = B + lane * S::BP;

  PolicyGradOutTile gout{};           // the output layer (the first one when L == 1)
  PolicyGradTile<W, NCH0> gh0{};      // hidden layer 0: L >= 2
  PolicyGradTile<W, 1> gh1{};         // hidden layer 1: L == 3
  float loss = 0.f;
  if constexpr (MODE == 1) {
#pragma unroll
    for (int q = 0; q < kPpoExtras; ++q) ppo_lane_sums()[q * kBlock + threadIdx.x] = 0.f;  // (+0.f is the integer 0 too)
  }

  for (int64_t tile = blockIdx.x; tile < r.tiles; tile += gridDim.x) {  // (block-uniform: every thread meets every barrier)
    const int64_t t = tile / r.tiles_per_step;
    const int64_t i = (tile - t * r.tiles_per_step) * kBlock + threadIdx.x;
    bool active = i < r.n;
    float c = 0.f, a[MT_MAX_DOF];
    if (active) c = r.coef[t * r.coef_ld + i];
    if constexpr (MODE == 1) {  // c is A until the ratio is known
      if (active && r.weight) c = r.weight[t * r.weight_ld + i] * c;
    }
    active = active && c != 0.f;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < MT_MAX_DOF; ++j) {
      a[j] = 0.f;
      if (active && j < D) a[j] = r.action[(t * D + j) * r.act_ld + i];
      bad |= unusable_angle(a[j]);
    }
    active = active && !bad;
    if (!active) {
      c = 0.f;
#pragma unroll
      for (int j = 0; j < MT_MAX_DOF; ++j) a[j] = 0.f;
    }
    const float* xcol = r.obs + t * IN * r.obs_ld + i;  // x_k = xcol[k obs_ld], read by active lanes only
    auto first_layer = [&](auto& acc, int n_out) {
      policy_bias(acc, b0, n_out);
      for (int k = 0; k < r.K; ++k) {
        float tri[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) tri[q] = active ? xcol[(int64_t)(3 * k + q) * r.obs_ld] : 0.f;
        policy_feed(acc, w0, IN, n_out, 3 * k, tri);
      }
      if (r.see_pose) {
        for (int j = 0; j < D; ++j) {
          const float xj[1] = {active ? xcol[(int64_t)(3 * r.K + j) * r.obs_ld] : 0.f};
          policy_feed(acc, w0, IN, n_out, 3 * r.K + j, xj);
        }
      }
    };
    // the images of one layer, wave after wave, into the outputs the threads own
    auto reduce = [&](auto& g, const auto& delta, auto&& put_input, int n_in, int n_out) {
#pragma unroll 1
      for (int p = 0; p < kBlock / 64; ++p) {
        __syncthreads();
        if (wave == p) {
          policy_grad_put(arow, delta);
          put_input();
        }
        __syncthreads();
        policy_grad_accumulate<S::AP, S::BP>(g, A, B, n_in, n_out);
      }
    };
    auto put_x = [&]() {  // with zeros up to the end of the last W-column chunk that holds an input
#pragma unroll 1
      for (int k = 0; k < NCH0 * W && (k / W) * W < IN; ++k)
        brow[k] = (active && k < IN) ? xcol[(int64_t)k * r.obs_ld] : 0.f;
    };

    float y[MT_MAX_DOF], h0[W], h1[W];
    if (L == 1) {
      first_layer(y, D);
    } else {
      first_layer(h0, r.n_out[0]);
      policy_finish(h0, r.hidden_act, r.n_out[0]);
      if (L == 2) {
#pragma unroll
        for (int j = 0; j < MT_MAX_DOF; ++j) y[j] = j < D ? policy_dot<W>(wl + (int64_t)j * r.n_in[1], bl[j], r.n_in[1], h0) : 0.f;
      } else {
#pragma unroll
        for (int o = 0; o < W; ++o) h1[o] = 0.f;
        policy_hidden<W>(as_weights(r.w[1]), as_weights(r.b[1]), r.n_in[1], r.n_out[1], r.hidden_act, h0, h1);
#pragma unroll
        for (int j = 0; j < MT_MAX_DOF; ++j) y[j] = j < D ? policy_dot<W>(wl + (int64_t)j * r.n_in[2], bl[j], r.n_in[2], h1) : 0.f;
      }
    }
    float dl[MT_MAX_DOF], lp = 0.f;
#pragma unroll
    for (int j = 0; j < MT_MAX_DOF; ++j) {
      dl[j] = 0.f;
      if (j < D) {
        const float tj = policy_act(r.out_act, y[j]);
        const float mu = r.out_scale * tj;
        const float e = a[j] - mu;
        const float d = e * r.inv_var[j];
        lp = __builtin_fmaf(e, d, lp);
        if constexpr (MODE == 0) {
          dl[j] = ((c * d) * r.out_scale) * policy_act_slope(r.out_act, tj);
        }
      }
    }
    if constexpr (MODE == 0) {
      loss = __builtin_fmaf(c, -0.5f * lp, loss);
    } else {
      const float adv = c;  // A: not 0 on an active lane
      float ratio = 0.f;
      c = 0.f;
      if (active) {
        const float x0 = (-0.5f * lp - r.old_logp[t * r.old_ld + i]) + r.shift;
        const float x = fminf(fmaxf(x0, -MT_PPO_MAX_LOG_RATIO), MT_PPO_MAX_LOG_RATIO);
        ratio = __builtin_amdgcn_exp2f(x * kLog2e);
        const bool up = adv > 0.f;
        const bool clipped = r.clipping && (up ? ratio > r.hi : ratio < r.lo);
        const float ra = ratio * adv;
        c = clipped ? 0.f : ra;
        const float obj = clipped ? (up ? r.hi : r.lo) * adv : ra;
        loss = loss + obj;
        const float k = (ratio - 1.f) - x;
        float* const ls = ppo_lane_sums() + threadIdx.x;  // kl, MT_MAX_DOF sigma sums, used, clipped
        ls[0] = ls[0] + k;
        int* const used = reinterpret_cast<int*>(ls + (1 + MT_MAX_DOF) * kBlock);
        used[0] += 1;
        used[kBlock] += clipped ? 1 : 0;
      }
#pragma unroll
      for (int j = 0; j < MT_MAX_DOF; ++j) {
        if (j < D) {
          // e and d once more, by the loop's own expressions from a y the compiler cannot tell from a new one: kept across
          // the ratio they would be 3 D more live registers where the kernel has none
          float yj = y[j];
          asm volatile("" : "+v"(yj));
          const float tj = policy_act(r.out_act, yj);
          const float mu = r.out_scale * tj;
          const float e = a[j] - mu;
          const float d = e * r.inv_var[j];
          dl[j] = ((c * d) * r.out_scale) * policy_act_slope(r.out_act, tj);
          float* const sg = ppo_lane_sums() + (1 + j) * kBlock + threadIdx.x;
          sg[0] = __builtin_fmaf(c, __builtin_fmaf(e, d, -1.f), sg[0]);
        }
      }
      if (i < r.n) {
        if (r.ratio) r.ratio[t * r.ratio_ld + i] = ratio;
        if (r.coef_out) r.coef_out[t * r.coefo_ld + i] = c;
      }
    }

    if (L == 1) {
      reduce(gout, dl, put_x, IN, D);
    } else if (L == 2) {
      reduce(gout, dl, [&]() { policy_grad_put(brow, h0); }, r.n_in[1], D);
      float d0[W];
      policy_backprop<MT_MAX_DOF, W>(wl, r.n_in[1], D, dl, d0);
#pragma unroll
      for (int k = 0; k < W; ++k) d0[k] = d0[k] * policy_act_slope(r.hidden_act, h0[k]);
      reduce(gh0, d0, put_x, IN, r.n_out[0]);
    } else {
      reduce(gout, dl, [&]() { policy_grad_put(brow, h1); }, r.n_in[2], D);
      float d1[W];
      policy_backprop<MT_MAX_DOF, W>(wl, r.n_in[2], D, dl, d1);
#pragma unroll
      for (int k = 0; k < W; ++k) d1[k] = d1[k] * policy_act_slope(r.hidden_act, h1[k]);
      reduce(gh1, d1, [&]() { policy_grad_put(brow, h0); }, r.n_in[1], r.n_out[1]);
      float d0[W];
      policy_backprop<W, W>(as_weights(r.w[1]), r.n_in[1], r.n_out[1], d1, d0);
#pragma unroll
      for (int k = 0; k < W; ++k) d0[k] = d0[k] * policy_act_slope(r.hidden_act, h0[k]);
      reduce(gh0, d0, put_x, IN, r.n_out[0]);
    }
  }

  float* part = r.partials + (int64_t)blockIdx.x * (r.P + 1 + (MODE == 1 ? kPpoExtras : 0));
  policy_grad_store(gout, part + r.off[L - 1], r.n_in[L - 1], D);
  if (L >= 2) policy_grad_store(gh0, part + r.off[0], IN, r.n_out[0]);
  if (L == 3) policy_grad_store(gh1, part + r.off[1], r.n_in[1], r.n_out[1]);
  __syncthreads();
  if constexpr (MODE == 0) {
    img[threadIdx.x] = loss;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int q = 0; q < kBlock; ++q) s = s + img[q];
      part[r.P] = s;
    }
  } else {  // thread 0 adds the objective, thread q > 0 the lanes' extra sum q - 1, each in thread order
    img[threadIdx.x] = loss;
    __syncthreads();
    if (threadIdx.x < 1 + kPpoExtras) {
      const float* col = threadIdx.x ? ppo_lane_sums() + (threadIdx.x - 1) * kBlock : img;
      if (threadIdx.x < 2 + MT_MAX_DOF) {
        float s = 0.f;
        for (int q = 0; q < kBlock; ++q) s = s + col[q];
        part[r.P + threadIdx.x] = s;
      } else {  // a block's counts fit 32 bits: it sees at most max(kBlock, samples / blocks) samples
        int s = 0;
        for (int q = 0; q < kBlock; ++q) s += __float_as_int(col[q]);
        part[r.P + threadIdx.x] = __int_as_float(s);
      }
    }
  }
}

// grad[i] = scale * (partials[0][i] + partials[1][i] + ...), ascending; word P is the loss
inline __global__ __launch_bounds__(kBlock) void policy_grad_reduce_kernel(const PolicyGradArgs r) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > r.P) return;
  float s = 0.f;
  for (int b = 0; b < r.blocks; ++b) s = s + r.partials[(int64_t)b * (r.P + 1) + i];
  s = s * r.scale;
  if (i < r.P) r.grad[i] = s;
  else if (r.loss) r.loss[0] = s;
}

// mt_ppo_grad's second pass: the same sums over rows of P + 1 + kPpoExtras words; the last two words are integer counts
inline __global__ __launch_bounds__(kBlock) void ppo_grad_reduce_kernel(const PpoGradArgs r) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t pitch = r.P + 1 + kPpoExtras;
  if (i >= pitch) return;
  const int64_t e = i - r.P;  // 0: the objective, 1: kl, 2 .. 1 + MT_MAX_DOF: sigma, then used, clipped
  if (e >= 2 + MT_MAX_DOF) {
    long long s = 0;
    for (int b = 0; b < r.blocks; ++b) s += (long long)__float_as_int(r.partials[(int64_t)b * pitch + i]);
    if (r.count) r.count[e - (2 + MT_MAX_DOF)] = s;
    return;
  }
  float s = 0.f;
  for (int b = 0; b < r.blocks; ++b) s = s + r.partials[(int64_t)b * pitch + i];
  s = s * r.scale;
  if (i < r.P) r.grad[i] = s;
  else if (e == 0) { if (r.loss) r.loss[0] = s; }
  else if (e == 1) { if (r.kl) r.kl[0] = s; }
  else if (e - 2 < r.D && r.sigma_grad) r.sigma_grad[e - 2] = s;
}

struct RewardToGoArgs {
  const int8_t* reward;  // [T][log_ld]
  const uint8_t* done;
  int64_t log_ld;
  float* out;  // [T][out_ld]
  int64_t out_ld;
  int64_t n;
  int32_t T;
  float gamma, baseline;
  uint32_t mask_after_done;
};
// one lane per env, backwards over t: R_t = fmaf(gamma, done_t ? 0 : R_t+1, r_t); steps behind the first done are 0 when masked
inline __global__ __launch_bounds__(kBlock) void reward_to_go_kernel(const RewardToGoArgs r) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.n) return;
  int first = r.T;
  if (r.mask_after_done) {
    for (int t = r.T - 1; t >= 0; --t)
      if (r.done[(int64_t)t * r.log_ld + i]) first = t;
  }
  float R = 0.f;
  for (int t = r.T - 1; t >= 0; --t) {
    float v = 0.f;
    if (t <= first) {
      const bool d = r.done[(int64_t)t * r.log_ld + i] != 0;
      R = __builtin_fmaf(r.gamma, d ? 0.f : R, (float)r.reward[(int64_t)t * r.log_ld + i]);
      v = R - r.baseline;
    }
    r.out[(int64_t)t * r.out_ld + i] = v;
  }
}

// ---------------------------------------------------------------------------
// The forward pass alone over logged observations (mt_policy_eval) and the advantages a critic's values turn the logs into
// (mt_gae).  As above, neither depends on the DH table nor touches a handle's state.
//
// policy_eval_kernel<W>: one sample (t, i) per lane, block (x, y) = tile x of kBlock consecutive envs of step y.  No LDS,
// no barrier: a lane behind n_envs returns at once.  The forward pass is policy_grad_kernel's text -- policy_bias /
// policy_feed over x streamed from obs in triples, policy_finish, policy_hidden, policy_dot -- so mu has the bits of the
// rollout and of the gradient; the weights are wave-uniform scalar operands, h0 / h1 register arrays that policy_hidden
// rotates (no register array is indexed dynamically), and only about 2 W floats are live: no backward pass keeps them.
// logp follows policy_grad_kernel's sequence word for word (e, d = e * inv_var, lp = fmaf(e, d, lp), -0.5f * lp).
// ---------------------------------------------------------------------------
struct PolicyEvalArgs {
  const float* w[3];
  const float* b[3];
  int32_t n_in[3], n_out[3];  // per layer, as PolicyArgs; n_out[L - 1] = NO
  int32_t L, K, n_pose, NO;   // n_pose: the joint angles behind the 3 K words of x (0 without MT_POLICY_SEE_POSE)
  int32_t hidden_act, out_act;
  float out_scale;
  float inv_var[MT_MAX_DOF];  // the fp32 nearest to 1 / sigma_j^2 (read with logp)
  const float* obs;  // [T * IN][obs_ld]
  int64_t obs_ld;
  const float* action;  // [T * NO][act_ld] or NULL
  int64_t act_ld;
  float* mean;  // [T * NO][mean_ld] or NULL
  int64_t mean_ld;
  float* logp;  // [T][logp_ld] or NULL (then action is not read)
  int64_t logp_ld;
  int64_t n;  // envs
};

template <int W>
__global__ __launch_bounds__(kBlock) void policy_eval_kernel(const PolicyEvalArgs r) {
  const int64_t t = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.n) return;
  const int L = r.L, IN = r.n_in[0], NO = r.NO;
  const weight_ptr w0 = as_weights(r.w[0]), b0 = as_weights(r.b[0]);
  const weight_ptr wl = as_weights(r.w[L - 1]), bl = as_weights(r.b[L - 1]);  // the output layer
  const float* xcol = r.obs + t * IN * r.obs_ld + i;                          // x_k = xcol[k obs_ld]
  auto first_layer = [&](auto& acc, int n_out) {
    policy_bias(acc, b0, n_out);
    for (int k = 0; k < r.K; ++k) {
      float tri[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) tri[q] = xcol[(int64_t)(3 * k + q) * r.obs_ld];
      policy_feed(acc, w0, IN, n_out, 3 * k, tri);
    }
    for (int j = 0; j < r.n_pose; ++j) {
      const float xj[1] = {xcol[(int64_t)(3 * r.K + j) * r.obs_ld]};
      policy_feed(acc, w0, IN, n_out, 3 * r.K + j, xj);
    }
  };

  float y[MT_MAX_DOF];
  if (L == 1) {
    first_layer(y, NO);
  } else {
    float h0[W];
    first_layer(h0, r.n_out[0]);
    policy_finish(h0, r.hidden_act, r.n_out[0]);
    if (L == 2) {
#pragma unroll
      for (int j = 0; j < MT_MAX_DOF; ++j) y[j] = j < NO ? policy_dot<W>(wl + (int64_t)j * r.n_in[1], bl[j], r.n_in[1], h0) : 0.f;
    } else {
      float h1[W];
#pragma unroll
      for (int o = 0; o < W; ++o) h1[o] = 0.f;
      policy_hidden<W>(as_weights(r.w[1]), as_weights(r.b[1]), r.n_in[1], r.n_out[1], r.hidden_act, h0, h1);
#pragma unroll
      for (int j = 0; j < MT_MAX_DOF; ++j) y[j] = j < NO ? policy_dot<W>(wl + (int64_t)j * r.n_in[2], bl[j], r.n_in[2], h1) : 0.f;
    }
  }

  float lp = 0.f;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < MT_MAX_DOF; ++j) {
    if (j < NO) {
      const float tj = policy_act(r.out_act, y[j]);
      const float mu = r.out_scale * tj;
      if (r.mean) r.mean[(t * NO + j) * r.mean_ld + i] = mu;
      if (r.logp) {
        const float a = r.action[(t * NO + j) * r.act_ld + i];
        bad |= unusable_angle(a);
        const float e = a - mu;
        const float d = e * r.inv_var[j];
        lp = __builtin_fmaf(e, d, lp);
      }
    }
  }
  if (r.logp) r.logp[t * r.logp_ld + i] = bad ? 0.f : -0.5f * lp;
}

struct GaeArgs {
  const int8_t* reward;  // [T][log_ld]
  const uint8_t* done;
  int64_t log_ld;
  const float* value;  // [T][value_ld]
  int64_t value_ld;
  const float* last_value;  // [n] or NULL
  float gamma, gl;          // gl: the fp32 product gamma * lambda
  float* adv;               // [T][adv_ld]
  int64_t adv_ld;
  float* ret;  // [T][ret_ld] or NULL
  int64_t ret_ld;
  float* weight;  // [T][weight_ld] or NULL
  int64_t weight_ld;
  int64_t n;
  int32_t T;
  uint32_t mask_after_done;
};
// one lane per env, backwards over t, as reward_to_go_kernel: delta = fmaf(gamma, done_t ? 0 : V_t+1, r_t) - V_t,
// A_t = fmaf(gl, done_t ? 0 : A_t+1, delta), ret_t = A_t + V_t; steps behind the first done are 0 (and not read) when masked
inline __global__ __launch_bounds__(kBlock) void gae_kernel(const GaeArgs r) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= r.n) return;
  int first = r.T;
  if (r.mask_after_done) {
    for (int t = r.T - 1; t >= 0; --t)
      if (r.done[(int64_t)t * r.log_ld + i]) first = t;
  }
  float A = 0.f, Vn = r.last_value ? r.last_value[i] : 0.f;
  for (int t = r.T - 1; t >= 0; --t) {
    float adv = 0.f, ret = 0.f, wt = 0.f;
    if (t <= first) {
      const bool d = r.done[(int64_t)t * r.log_ld + i] != 0;
      const float V = r.value[(int64_t)t * r.value_ld + i];
      const float delta = __builtin_fmaf(r.gamma, d ? 0.f : Vn, (float)r.reward[(int64_t)t * r.log_ld + i]) - V;
      A = __builtin_fmaf(r.gl, d ? 0.f : A, delta);
      adv = A;
      ret = A + V;
      wt = 1.f;
      Vn = V;
    }
    r.adv[(int64_t)t * r.adv_ld + i] = adv;
    if (r.ret) r.ret[(int64_t)t * r.ret_ld + i] = ret;
    if (r.weight) r.weight[(int64_t)t * r.weight_ld + i] = wt;
  }
}

// ---------------------------------------------------------------------------
// mt_shoot's evaluation: C candidate tapes per env scored from the SAME resident state, the best one named.  For env i
// and candidate c, returns[c][i] is what rollout_tape_kernel's dry run writes to return_out[i] for plane c, bit for bit;
// best[i] is the smallest c whose return is maximal.  Nothing resident is written.
//
// One block owns kShootEnvs = 64 consecutive envs; its four waves split the candidates (wave w scores c = w, w + 4, ...,
// one after the other), lane l is env 64 b + l in every wave.  A wave is thus 64 consecutive, 64-aligned envs of ONE
// candidate with the tail lanes of the last wave inactive -- the very lanes that share a wave in the tape kernel.  That
// is what bit identity needs: route_kinematics takes its wide form per wave (__any), so an env's z-minimum can depend on
// its wave-mates; candidates side by side in a wave would break it.
//   state   : start pose and alive mask are loaded once per lane and kept in registers; every candidate restarts from
//             them with nothing known about the pose (pose_valid = false), as the dry run does.
//   targets : one READ-ONLY [3K][64] LDS tile shared by the four waves (24 KB at K = 32).  The dry run's dead-target
//             zeroing serves the observation of a committing call; no return depends on it, so there is no
//             per-candidate copy.
//   a step  : plan_step, shared with cem_kernel and mppi_kernel: every bit identity between the three rests on that one
//             text.  It is what the tape kernel's intermediate steps run -- unusable_angle screening (held pose, NOT counted),
//             route_kinematics<Tbl, 0, true, false> with the PoseCache kept across the steps of one candidate, within_box
//             on the alive targets, the reward rule.  MT_FLAG_TERMINATE_ON_GROUND changes `done` only, and without a
//             re-arm `done` feeds nothing a return depends on: there is nothing to compute for it.
//   select  : every wave keeps (best return, its lowest index) per lane over its own candidates, visited in ascending
//             order; the four pairs meet in 2 KB of LDS and wave 0 writes best / best_return.  No atomics, no init
//             pass, no dependence between blocks: the result is a function of (state, plans) alone.
// Per env: the state is read once (4 D + 4 + 12 K bytes) where C dry runs read it C times, 4 D T C bytes of plans, and
// 4 C bytes of scores only where returns_out is given.
// ---------------------------------------------------------------------------
constexpr int kShootEnvs = 64;
constexpr int kShootWaves = kBlock / 64;
struct ShootArgs {
  const float* plans;     // candidate c, step t, joint j, env i = plans[c * cand_stride + (t * D + j) * ld + i]
  int64_t ld, cand_stride;
  float* returns_out;     // [C][ret_ld] or NULL
  int64_t ret_ld;
  int32_t* best_out;      // [n] or NULL
  float* best_return_out; // [n] or NULL
  int32_t T, C;
};

// The block prologue of shoot_kernel, cem_kernel and mppi_kernel: a live lane loads its start pose and alive mask, and the
// four waves fill the [3K][64] target tile.  The barrier that publishes the tile is the caller's.
template <int D>
__device__ __forceinline__ void plan_start(const StepArgs& a, bool live, uint32_t lane, uint32_t w, LaneOffset<true>& o4, float* tile,
                                           float (&g0)[D], uint32_t& am0) {
  const int64_t ld = a.ld;
  am0 = 0u;
  if (live) {
#pragma unroll
    for (int j = 0; j < D; ++j) g0[j] = ldr(a.goals + j * ld, o4);
    am0 = ldr(a.alive, o4);
    for (int k = (int)w; k < 3 * a.K; k += kShootWaves) tile[k * kShootEnvs + lane] = ldr(a.points + (int64_t)k * ld, o4);
  }
}

// One step of one candidate, the only copy: the angles `raw` take pose g, alive mask am, return ret and the PoseCache of
// this candidate one step on.  `col` is the lane's column of the target tile.
template <class Tbl>
__device__ __forceinline__ void plan_step(const Tbl& t, const StepArgs& a, const float (&raw)[Tbl::D], float (&g)[Tbl::D], uint32_t& am,
                                          float& ret, PoseCache<Tbl::D>& pose, bool& pose_valid, const float* col) {
  constexpr int D = Tbl::D;
  float act[D], el[3], e[3];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < D; ++j) bad |= unusable_angle(raw[j]);
#pragma unroll
  for (int j = 0; j < D; ++j) act[j] = bad ? g[j] : raw[j];  // the env holds its pose this step

  const float zmin = route_kinematics<Tbl, 0, true, false>(t, a.S, a.inv_sm1, g, act, el, e, &pose, pose_valid, nullptr, false);
  pose_valid = true;
  const bool ground = zmin < 0.f;
  uint32_t nam = am;
  for (int k = 0; k < a.K; ++k) {
    if (!((am >> k) & 1u)) continue;
    const float* pk = col + 3 * k * kShootEnvs;
    if (within_box(e, pk[0], pk[kShootEnvs], pk[2 * kShootEnvs], a.tol)) nam &= ~(1u << k);
  }
  ret += (float)(ground ? -1 : ((nam != am) ? 1 : 0));
  am = nam;
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = act[j];
}

template <class Tbl>
__global__ __launch_bounds__(kBlock) void shoot_kernel(const StepArgs a, const ShootArgs r) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [3K][64] targets, [4][64] best returns, [4][64] best indices
  constexpr int D = Tbl::D;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kShootEnvs + lane;
  const bool live = i < a.n;  // the tail lanes of the last block load, score and store nothing, but meet the barriers
  LaneOffset<true> o4{i * 4u};
  const float* col = tile + lane;
  float* best_v = tile + 3 * a.K * kShootEnvs;
  int32_t* best_c = reinterpret_cast<int32_t*>(best_v + kShootWaves * kShootEnvs);

  float g0[D];
  uint32_t am0;
  plan_start<D>(a, live, lane, w, o4, tile, g0, am0);
  __syncthreads();

  float top = -__builtin_inff();  // (a return is a finite sum of -1 / 0 / +1)
  int32_t top_c = 0x7FFFFFFF;
  if (live) {
    for (int c = (int)w; c < r.C; c += kShootWaves) {  // (wave-uniform)
      const float* plane = r.plans + (int64_t)c * r.cand_stride;
      float g[D];
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = g0[j];
      uint32_t am = am0;
      float ret = 0.f;
      PoseCache<D> pose;
      bool pose_valid = false;
      for (int s = 0; s < r.T; ++s) {
        float raw[D];
#pragma unroll
        for (int j = 0; j < D; ++j) raw[j] = tape_load(plane + ((int64_t)s * D + j) * r.ld, o4, false);
        plan_step<Tbl>(t, a, raw, g, am, ret, pose, pose_valid, col);
      }
      if (r.returns_out) str_stream(r.returns_out + (int64_t)c * r.ret_ld, o4, ret);
      if (ret > top) {  // ascending c: a tie keeps the earlier candidate
        top = ret;
        top_c = c;
      }
    }
  }
  best_v[w * kShootEnvs + lane] = top;
  best_c[w * kShootEnvs + lane] = top_c;
  __syncthreads();
  if (w != 0 || !live) return;
#pragma unroll
  for (int q = 1; q < kShootWaves; ++q) {  // a wave without candidates (C < 4) left (-inf, INT_MAX)
    const float v = best_v[q * kShootEnvs + lane];
    const int32_t vc = best_c[q * kShootEnvs + lane];
    if (v > top || (v == top && vc < top_c)) {
      top = v;
      top_c = vc;
    }
  }
  if (r.best_out) str(r.best_out, o4, top_c);
  if (r.best_return_out) str_stream(r.best_return_out, o4, top);
}

// ---------------------------------------------------------------------------
// mt_cem: one iteration of the cross-entropy method where the data sits.  The candidates shoot_kernel reads from a
// (C, T, D, N) block are DRAWN here -- a candidate angle is a pure function of (seed, global env id, draw, c, t, j) and
// of the env's mean and sigma (philox.h: the plan stream) -- so the block never exists; mt_sample_plans
// (sample_plans_kernel) writes it out for whoever wants it, and the evaluation below equals shoot_kernel on that block
// bit for bit: same block / wave / lane shape (a wave = 64 consecutive envs of ONE candidate, plan_start), same step
// (plan_step).
//   an angle : x = mean + sigma * z (two roundings; contraction is off); unusable_angle(x) is handed on as it is (the
//              step holds the pose), anything else is clamped to [lo, hi].  KEEP_MEAN: candidate 0 has z = 0.
//   scores   : every candidate's return goes into a [C][64] LDS tile as well.  Behind the barrier each wave ranks ITS
//              candidates against the tile (rank = number of candidates that beat it: a higher return, or the same
//              return and a lower index; a lane reads its own column: conflict-free), sets the bits of those with
//              rank < E in its own [64] mask row and names the one with rank 0 (exactly one per env) as best.
//   refit    : behind a second barrier the waves split the T steps.  For step t a lane regenerates the angles of its E
//              elites in ascending index order (lowest set bit first) -- twice, first for the mean, then for the squared
//              deviations, nothing is stored -- and writes mean_out / sigma_out[t][.][i].  With mean_out == mean the
//              element is read and written by this one thread, after the block's last scoring read.  The same pass
//              writes rows t < H of chosen_out from the best candidate (refit_head, shared with mppi_kernel).
// No atomics on global memory, no init pass, no dependence between blocks.  Tail lanes meet every barrier and store nothing.
// ---------------------------------------------------------------------------
struct CemArgs {
  const float *mean, *sigma;  // [T * D][ld]
  int64_t ld;
  float *mean_out, *sigma_out;  // [T * D][out_ld] or both NULL
  int64_t out_ld;
  float* returns_out;  // [C][ret_ld] or NULL
  int64_t ret_ld;
  int32_t* best_out;               // [n] or NULL
  float* best_return_out;          // [n] or NULL
  unsigned long long* elite_mask;  // [n] or NULL
  float* chosen_out;               // [H * D][chosen_ld] or NULL (H == 0)
  int64_t chosen_ld;
  int32_t T, C, E, H;
  uint32_t draw, keep_mean;
  uint32_t seed_lo, seed_hi;
  float lo, hi, sigma_min, inv_e;
};

// the D angles of candidate c at step t from the env's mean / sigma rows of that step
template <int D, class Args>
__device__ __forceinline__ void plan_angles(const Args& r, uint64_t seed, uint64_t env_id, uint32_t c, uint32_t t,
                                            const float (&mu)[D], const float (&sg)[D], float (&x)[D]) {
  static_assert(D <= 8, "a plan step is at most two Philox blocks");
  const bool zero = (r.keep_mean != 0u) & (c == 0u);
  const u32x4 b0 = stream_block(seed, env_id, kTagPlan, r.draw, plan_minor(c, 0u, t));
  uint32_t w[8] = {b0.x, b0.y, b0.z, b0.w, 0u, 0u, 0u, 0u};
  if constexpr (D > 4) {
    const u32x4 b1 = stream_block(seed, env_id, kTagPlan, r.draw, plan_minor(c, 1u, t));
    w[4] = b1.x;
    w[5] = b1.y;
    w[6] = b1.z;
    w[7] = b1.w;
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const float z = zero ? 0.f : plan_noise(w[j]);
    const float sz = sg[j] * z;
    const float v = mu[j] + sz;
    x[j] = unusable_angle(v) ? v : fminf(fmaxf(v, r.lo), r.hi);
  }
}

// The head of step s in cem_kernel's and mppi_kernel's refit loops: the env's mean / sigma rows of that step and, where
// `pick` is set (s < H), row s of chosen_out from the best candidate top_c (x is scratch; the caller reuses it).
template <int D, class Args>
__device__ __forceinline__ void refit_head(const Args& r, uint64_t seed, uint64_t env_id, int32_t top_c, int s, bool pick,
                                           LaneOffset<true>& o4, float (&mu)[D], float (&sg)[D], float (&x)[D]) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
    mu[j] = tape_load(r.mean + ((int64_t)s * D + j) * r.ld, o4, false);
    sg[j] = tape_load(r.sigma + ((int64_t)s * D + j) * r.ld, o4, false);
  }
  if (pick) {
    plan_angles<D>(r, seed, env_id, (uint32_t)top_c, (uint32_t)s, mu, sg, x);
#pragma unroll
    for (int j = 0; j < D; ++j) str(r.chosen_out + ((int64_t)s * D + j) * r.chosen_ld, o4, x[j]);
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void sample_plans_kernel(const CemArgs r, float* plans, int64_t ld, int64_t cand_stride, int64_t n,
                                                              int64_t env_base) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = blockIdx.y, c = blockIdx.z;
  LaneOffset<true> o4{i * 4u};
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  float mu[D], sg[D], x[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    mu[j] = tape_load(r.mean + ((int64_t)t * D + j) * r.ld, o4, false);
    sg[j] = tape_load(r.sigma + ((int64_t)t * D + j) * r.ld, o4, false);
  }
  plan_angles<D>(r, seed, (uint64_t)(env_base + i), c, t, mu, sg, x);
  float* plane = plans + (int64_t)c * cand_stride;
#pragma unroll
  for (int j = 0; j < D; ++j) str_stream(plane + ((int64_t)t * D + j) * ld, o4, x[j]);
}

template <class Tbl>
__global__ __launch_bounds__(kBlock) void cem_kernel(const StepArgs a, const CemArgs r) {
  // [3K][64] targets, [C][64] returns, [4][64] 64-bit elite masks (one row per wave), [64] best indices
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int D = Tbl::D;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kShootEnvs + lane;
  const bool live = i < a.n;
  LaneOffset<true> o4{i * 4u};
  const float* col = tile + lane;
  float* rets = tile + 3 * a.K * kShootEnvs;
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(rets + r.C * kShootEnvs);
  int32_t* best_c = reinterpret_cast<int32_t*>(masks + kShootWaves * kShootEnvs);
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);

  float g0[D];
  uint32_t am0;
  plan_start<D>(a, live, lane, w, o4, tile, g0, am0);
  __syncthreads();

  // ---- score: shoot_kernel's loop with the drawn angles in place of the tape's ----
  if (live) {
    for (int c = (int)w; c < r.C; c += kShootWaves) {  // (wave-uniform)
      float g[D];
#pragma unroll
      for (int j = 0; j < D; ++j) g[j] = g0[j];
      uint32_t am = am0;
      float ret = 0.f;
      PoseCache<D> pose;
      bool pose_valid = false;
      for (int s = 0; s < r.T; ++s) {
        float raw[D], mu[D], sg[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {  // requested at the head of the step: the Philox rounds below cover the latency
          mu[j] = tape_load(r.mean + ((int64_t)s * D + j) * r.ld, o4, false);
          sg[j] = tape_load(r.sigma + ((int64_t)s * D + j) * r.ld, o4, false);
        }
        plan_angles<D>(r, seed, env_id, (uint32_t)c, (uint32_t)s, mu, sg, raw);
        plan_step<Tbl>(t, a, raw, g, am, ret, pose, pose_valid, col);
      }
      if (r.returns_out) str_stream(r.returns_out + (int64_t)c * r.ret_ld, o4, ret);
      rets[c * kShootEnvs + lane] = ret;
    }
  }
  __syncthreads();

  // ---- rank this wave's candidates against all C ----
  unsigned long long mine = 0ull;
  if (live) {
    for (int c = (int)w; c < r.C; c += kShootWaves) {
      const float v = rets[c * kShootEnvs + lane];
      int rank = 0;
      for (int q = 0; q < r.C; ++q) {
        const float u = rets[q * kShootEnvs + lane];
        rank += ((u > v) | ((u == v) & (q < c))) ? 1 : 0;
      }
      if (rank < r.E) mine |= 1ull << c;
      if (rank == 0) best_c[lane] = c;
    }
  }
  masks[w * kShootEnvs + lane] = mine;
  __syncthreads();
  if (!live) return;  // (no barrier below)

  unsigned long long elite = 0ull;
#pragma unroll
  for (int q = 0; q < kShootWaves; ++q) elite |= masks[q * kShootEnvs + lane];
  const int32_t top_c = best_c[lane];
  if (w == 0) {
    if (r.best_out) str(r.best_out, o4, top_c);
    if (r.best_return_out) str_stream(r.best_return_out, o4, rets[top_c * kShootEnvs + lane]);
    if (r.elite_mask) r.elite_mask[i] = elite;
  }

  // ---- refit and the chosen rows: the waves split the steps ----
  const bool refit = r.mean_out != nullptr;
  for (int s = (int)w; s < r.T; s += kShootWaves) {  // (wave-uniform)
    const bool pick = s < r.H;
    if (!refit && !pick) break;  // (H <= T and s ascends: nothing further down either)
    float mu[D], sg[D], x[D];
    refit_head<D>(r, seed, env_id, top_c, s, pick, o4, mu, sg, x);
    if (!refit) continue;
    float m[D] = {}, v[D] = {};  // (both overwritten by the first elite: the sums start from x_0 and d_0 * d_0)
    unsigned long long left = elite;
    for (int k = 0; k < r.E; ++k) {  // every live lane has exactly E elites; each lane walks its own, lowest index first
      const uint32_t c = (uint32_t)__builtin_ctzll(left);
      left &= left - 1ull;
      plan_angles<D>(r, seed, env_id, c, (uint32_t)s, mu, sg, x);
#pragma unroll
      for (int j = 0; j < D; ++j) m[j] = (k == 0) ? x[j] : m[j] + x[j];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) m[j] = m[j] * r.inv_e;
    left = elite;
    for (int k = 0; k < r.E; ++k) {
      const uint32_t c = (uint32_t)__builtin_ctzll(left);
      left &= left - 1ull;
      plan_angles<D>(r, seed, env_id, c, (uint32_t)s, mu, sg, x);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float d = x[j] - m[j];
        const float dd = d * d;
        v[j] = (k == 0) ? dd : v[j] + dd;
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
      str(r.mean_out + ((int64_t)s * D + j) * r.out_ld, o4, m[j]);
      str(r.sigma_out + ((int64_t)s * D + j) * r.out_ld, o4, fmaxf(sqrtf(v[j] * r.inv_e), r.sigma_min));
    }
  }
}

// The return of drawn candidate c over r.T steps from the start pose g0 and alive mask am0, for mppi_kernel (Args: any
// block with mean / sigma / ld / T and plan_angles' fields).  The step exists once, as plan_step; the dozen lines around it
// -- restart from (g0, am0), load mean / sigma, draw, step -- exist twice, here and in cem_kernel.  Routed through this
// function cem_kernel compiles to one VGPR more in every instantiation (the callee is simplified on its own before it is
// inlined), and the register rows of existing kernels stay as they are.
template <class Tbl, class Args>
__device__ __forceinline__ float plan_return(const Tbl& t, const StepArgs& a, const Args& r, uint64_t seed, uint64_t env_id, uint32_t c,
                                             LaneOffset<true> o4, const float (&g0)[Tbl::D], uint32_t am0, const float* col) {
  constexpr int D = Tbl::D;
  float g[D];
#pragma unroll
  for (int j = 0; j < D; ++j) g[j] = g0[j];
  uint32_t am = am0;
  float ret = 0.f;
  PoseCache<D> pose;
  bool pose_valid = false;
  for (int s = 0; s < r.T; ++s) {
    float raw[D], mu[D], sg[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {  // requested at the head of the step: the Philox rounds below cover the latency
      mu[j] = tape_load(r.mean + ((int64_t)s * D + j) * r.ld, o4, false);
      sg[j] = tape_load(r.sigma + ((int64_t)s * D + j) * r.ld, o4, false);
    }
    plan_angles<D>(r, seed, env_id, c, (uint32_t)s, mu, sg, raw);
    plan_step<Tbl>(t, a, raw, g, am, ret, pose, pose_valid, col);
  }
  return ret;
}

// ---------------------------------------------------------------------------
// mt_mppi: one MPPI (model-predictive path integral) iteration where the data sits.  cem_kernel's shape and scoring --
// the same plan stream, the same block / wave / lane layout (plan_start), the same step (plan_step, through plan_return)
// -- so the evaluation equals shoot_kernel on the block mt_sample_plans writes, bit for bit.  There is no elite set: candidate c weighs rho^k, k = best return - its own.
//   weights  : a step's reward is -1, 0 or +1, so a return is an integer in [-T, T] and the gap k an integer in [0, 2T].
//              W[0] = 1, W[k] = W[k-1] * rho (one rounding each) is built by thread 0 in LDS ahead of the first barrier;
//              no transcendental function is evaluated and numpy restates the table bit for bit.
//   select   : behind the scoring barrier every lane reads its own column of the [C][64] score tile (conflict-free) for
//              the maximum and the lowest index that reaches it.  Behind a third barrier each wave turns ITS rows of the
//              tile into weights (w = W[(int)(top - score)]) and writes them to weights_out.
//   refit    : behind the fourth barrier every lane sums its column, S = sum of w_c from +0 in ascending c, and the waves
//              split the T steps.  For step t a lane walks c = 0 .. C-1, regenerates the angles (nothing is stored) and
//              accumulates A += w_c * x_c; m = A / S is one correctly rounded division.  With sigma_out a second walk
//              accumulates Q += w_c * (x_c - m)^2 and sigma_out = max(sqrt(Q / S), sigma_min).  A candidate whose weight
//              is 0 in every lane of the wave is skipped: its terms are +-0 on sums that started from +0.  With mean_out
//              == mean the element is read and written by this one thread, after the block's last scoring read.  The same
//              pass writes rows t < H of chosen_out from the best candidate (refit_head).
// No atomics on global memory, no init pass, no dependence between blocks.  Tail lanes meet every barrier and store nothing.
// ---------------------------------------------------------------------------
constexpr int kMppiMaxSteps = 127;
constexpr int kMppiTable = 2 * kMppiMaxSteps + 2;  // 2T + 1 <= 255 entries, rounded up to whole 16-byte slots
struct MppiArgs {
  const float *mean, *sigma;  // [T * D][ld]
  int64_t ld;
  float *mean_out, *sigma_out;  // [T * D][out_ld]; mean_out alone, both, or neither
  int64_t out_ld;
  float* returns_out;  // [C][ret_ld] or NULL
  int64_t ret_ld;
  float* weights_out;  // [C][w_ld] or NULL
  int64_t w_ld;
  float* weight_sum_out;   // [n] or NULL
  int32_t* best_out;       // [n] or NULL
  float* best_return_out;  // [n] or NULL
  float* chosen_out;       // [H * D][chosen_ld] or NULL (H == 0)
  int64_t chosen_ld;
  int32_t T, C, H;
  uint32_t draw, keep_mean;
  uint32_t seed_lo, seed_hi;
  float lo, hi, sigma_min, decay;
};

template <class Tbl>
__global__ __launch_bounds__(kBlock) void mppi_kernel(const StepArgs a, const MppiArgs r) {
  // [3K][64] targets, [C][64] returns (then weights), [kMppiTable] powers of decay
  extern __shared__ __attribute__((aligned(16))) float tile[];
  constexpr int D = Tbl::D;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kShootEnvs + lane;
  const bool live = i < a.n;
  LaneOffset<true> o4{i * 4u};
  const float* col = tile + lane;
  float* rets = tile + 3 * a.K * kShootEnvs;
  float* table = rets + r.C * kShootEnvs;
  const uint64_t seed = ((uint64_t)r.seed_hi << 32) | r.seed_lo;
  const uint64_t env_id = (uint64_t)(a.env_base + i);

  float g0[D];
  uint32_t am0;
  plan_start<D>(a, live, lane, w, o4, tile, g0, am0);
  if (threadIdx.x == 0) {  // the recurrence, nothing else: every weight of the call is one of these 2T + 1 floats
    float p = 1.f;
    table[0] = p;
    for (int k = 1; k <= 2 * r.T; ++k) {
      p = p * r.decay;
      table[k] = p;
    }
  }
  __syncthreads();

  // ---- score: cem_kernel's loop ----
  if (live) {
    for (int c = (int)w; c < r.C; c += kShootWaves) {  // (wave-uniform)
      const float ret = plan_return<Tbl>(t, a, r, seed, env_id, (uint32_t)c, o4, g0, am0, col);
      if (r.returns_out) str_stream(r.returns_out + (int64_t)c * r.ret_ld, o4, ret);
      rets[c * kShootEnvs + lane] = ret;
    }
  }
  __syncthreads();

  // ---- the maximum and the lowest index that reaches it: every wave for itself, a lane reads its own column ----
  float top = 0.f;
  int32_t top_c = 0;
  if (live) {
    top = rets[lane];  // (C >= 1)
    for (int c = 1; c < r.C; ++c) {
      const float v = rets[c * kShootEnvs + lane];
      if (v > top) {  // ascending c: a tie keeps the earlier candidate
        top = v;
        top_c = c;
      }
    }
  }
  __syncthreads();  // every wave has read the scores it needs

  // ---- scores -> weights: each wave its own rows ----
  if (live) {
    for (int c = (int)w; c < r.C; c += kShootWaves) {
      const int gap = (int)(top - rets[c * kShootEnvs + lane]);  // exact: both are integers within +-T
      const float wt = table[gap];
      rets[c * kShootEnvs + lane] = wt;
      if (r.weights_out) str_stream(r.weights_out + (int64_t)c * r.w_ld, o4, wt);
    }
  }
  __syncthreads();
  if (!live) return;  // (no barrier below)

  float sum = 0.f;
  for (int c = 0; c < r.C; ++c) sum += rets[c * kShootEnvs + lane];
  if (w == 0) {
    if (r.best_out) str(r.best_out, o4, top_c);
    if (r.best_return_out) str_stream(r.best_return_out, o4, top);
    if (r.weight_sum_out) str_stream(r.weight_sum_out, o4, sum);
  }

  // ---- refit and the chosen rows: the waves split the steps ----
  const bool refit = r.mean_out != nullptr, spread = r.sigma_out != nullptr;
  for (int s = (int)w; s < r.T; s += kShootWaves) {  // (wave-uniform)
    const bool pick = s < r.H;
    if (!refit && !pick) break;  // (H <= T and s ascends: nothing further down either)
    float mu[D], sg[D], x[D];
    refit_head<D>(r, seed, env_id, top_c, s, pick, o4, mu, sg, x);
    if (!refit) continue;
    float m[D] = {}, q[D] = {};
    for (int c = 0; c < r.C; ++c) {
      const float wt = rets[c * kShootEnvs + lane];
      if (!__any(wt != 0.f)) continue;  // (wave-uniform)
      plan_angles<D>(r, seed, env_id, (uint32_t)c, (uint32_t)s, mu, sg, x);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const float wx = wt * x[j];
        m[j] = m[j] + wx;
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) m[j] = m[j] / sum;
    if (spread) {
      for (int c = 0; c < r.C; ++c) {
        const float wt = rets[c * kShootEnvs + lane];
        if (!__any(wt != 0.f)) continue;
        plan_angles<D>(r, seed, env_id, (uint32_t)c, (uint32_t)s, mu, sg, x);
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const float d = x[j] - m[j];
          const float dd = d * d;
          const float wd = wt * dd;
          q[j] = q[j] + wd;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
      str(r.mean_out + ((int64_t)s * D + j) * r.out_ld, o4, m[j]);
      if (spread) str(r.sigma_out + ((int64_t)s * D + j) * r.out_ld, o4, fmaxf(sqrtf(q[j] / sum), r.sigma_min));
    }
  }
}

// ---------------------------------------------------------------------------
// Inverse kinematics of the pickup frame (mt_jacobian, mt_ik): the analytic position Jacobian and a fixed number of
// damped-least-squares iterations, one env per lane.  Not in the reference: it has no solver.
//
// The driven point p is the origin of the pickup frame (Tbl: the frame after all D joints; RtTableF: row fe of
// joints_coordinates, fe >= 1 -- the host refuses the origin row).  With z_j, o_j the Z axis and the origin of the frame
// BEFORE joint j, column j of the Jacobian is z_j x (p - o_j) per radian for every joint the frame depends on and exactly 0
// behind it.  One forward pass keeps the 6 D floats of (z_j, o_j) in registers and forms the columns once p is known.
// The chain is chain_all's, operation for operation, so p rounds as the frame origins do everywhere else; with a
// compile-time table the products with 0 / +-1 fall away and joint 0 never enters a z (z_0 is the constant (0, 0, 1)).
// ---------------------------------------------------------------------------
constexpr float kRadPerDeg = 0.017453292519943295f;
constexpr float kDegPerRad = 57.29577951308232f;

template <class Tbl, bool JAC>
__device__ __forceinline__ void ik_forward(const float (&q)[Tbl::D], const Tbl& t, float (&p)[3], float (&J)[3][Tbl::D]) {
  constexpr int D = Tbl::D;
  float X[3] = {1.f, 0.f, 0.f}, Y[3] = {0.f, 1.f, 0.f}, Z[3] = {0.f, 0.f, 1.f};
  float o[3] = {0.f, 0.f, 0.f};
  float zj[D][3], oj[D][3];
  if constexpr (Tbl::kFrames) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = 0.f;
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    float s, c;
    sincos_deg_off(q[j], t.off(j), s, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      zj[j][a] = Z[a];
      oj[j][a] = o[a];
      const float nx = pfma(X[a], c, pmul(Y[a], s));
      const float tt = pfma(Y[a], c, -pmul(X[a], s));
      o[a] = pfma(t.a(j), nx, pfma(t.d(j), Z[a], o[a]));
      X[a] = nx;
      Y[a] = pfma(tt, t.ca(j), pmul(Z[a], t.sa(j)));
      Z[a] = pfma(Z[a], t.ca(j), -pmul(tt, t.sa(j)));
      if constexpr (Tbl::kFrames) p[a] = (j >= 1 && j == t.fe()) ? o[a] : p[a];
    }
  }
  if constexpr (!Tbl::kFrames) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = o[a];
  }
  if constexpr (JAC) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const float r0 = p[0] - oj[j][0], r1 = p[1] - oj[j][1], r2 = p[2] - oj[j][2];
      float c0 = pfma(zj[j][1], r2, -pmul(zj[j][2], r1));
      float c1 = pfma(zj[j][2], r0, -pmul(zj[j][0], r2));
      float c2 = pfma(zj[j][0], r1, -pmul(zj[j][1], r0));
      if constexpr (Tbl::kFrames) {  // a joint behind the driven frame does not move it
        const bool drives = j <= t.fe();
        c0 = drives ? c0 : 0.f;
        c1 = drives ? c1 : 0.f;
        c2 = drives ? c2 : 0.f;
      }
      J[0][j] = c0;
      J[1][j] = c1;
      J[2][j] = c2;
    }
  }
}

struct JacobianArgs {
  const float* angles;  // [D][angles_ld] degrees
  int64_t angles_ld;
  float* jac;           // [3 D][jac_ld]: row 3 j + a = d p_a / d q_j per DEGREE
  int64_t jac_ld;
  float* pos;           // [3][pos_ld] or NULL: p
  int64_t pos_ld;
  int64_t n;
  DhConst dh;
};

template <class Tbl>
__global__ __launch_bounds__(kBlock) void jacobian_kernel(const JacobianArgs a) {
  constexpr int D = Tbl::D;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  float q[D], p[3], J[3][D];
#pragma unroll
  for (int j = 0; j < D; ++j) q[j] = (a.angles + j * a.angles_ld)[i];
  ik_forward<Tbl, true>(q, t, p, J);
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) (a.jac + (int64_t)(3 * j + c) * a.jac_ld)[i] = J[c][j] * kRadPerDeg;
  if (a.pos) {
#pragma unroll
    for (int c = 0; c < 3; ++c) (a.pos + c * a.pos_ld)[i] = p[c];
  }
}

// mt_ik.  Per iteration, with the per-radian J at the current pose:
//   e = x - p;  A = J J^T + lambda^2 I;  y = A^-1 e;  dq = (180 / pi) J^T y;  m = max |dq_j|;  m > max_step: dq *= max_step / m
// A is symmetric positive definite with every pivot >= lambda^2, so it is factored as L D L^T without pivoting: three
// divisions, and no cancellation of the size the adjugate's 2 x 2 minors carry when J J^T is close to singular.
// Every product is written as an fma chain in a fixed order (the build does not contract), so an env's result is a function
// of its own inputs alone: batch size, neighbours and the launch shape change no bit.
// An env freezes when its box residual max |e_a| is <= tol BEFORE an iteration (tol > 0 only): it takes no further step,
// which leaves exactly the angles of a run with fewer iterations; a wave whose lanes are all frozen leaves the loop -- the
// ballot is the kernel's only cross-lane operation.  No LDS, no atomics.
// Held envs (angles = start bit for bit, 0 steps): an unusable start angle or a non-finite target (residual NaN), and in
// nearest mode an env without an alive target (index -1, residual 0).  They compute on the zero pose and re-read their start.
struct IkArgs {
  const float* start;   // [D][start_ld] degrees (the caller's, or MT_F_GOALS)
  int64_t start_ld;
  const float* target;  // [3][target_ld], or NULL: each env's nearest alive target
  int64_t target_ld;
  const float* points;  // resident rows, read in nearest mode only: [3K][ld]
  const uint32_t* alive;
  int64_t ld;
  float* angles;        // [D][angles_ld] or NULL
  int64_t angles_ld;
  float* stage;         // MT_F_ACTIONS ([D][ld]) or NULL
  float* residual;      // [n] or NULL
  int32_t* steps;       // [n] or NULL
  int32_t* index;       // [n] or NULL (nearest mode)
  int64_t n;
  int32_t K, iters;
  uint32_t wrap;
  float lambda2, max_step, tol;
  DhConst dh;
};

template <class Tbl>
__global__ __launch_bounds__(kBlock) void ik_kernel(const IkArgs a) {
  constexpr int D = Tbl::D;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  const Tbl t = TableMaker<Tbl>::make(a.dh);
  float q[D], p[3], J[3][D], x[3] = {0.f, 0.f, 0.f};
  bool poisoned = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    q[j] = (a.start + j * a.start_ld)[i];
    poisoned |= unusable_angle(q[j]);
  }
  if (poisoned) {
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = 0.f;
  }
  int idx = -1;
  if (a.target) {
    // read as words: the build is -ffinite-math-only, under which a float that is TESTED for NaN may be assumed not to be one
    const uint32_t* words = reinterpret_cast<const uint32_t*>(a.target);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t w = (words + c * a.target_ld)[i];
      poisoned |= (w & 0x7F800000u) == 0x7F800000u;
      x[c] = __uint_as_float(w);
    }
  } else {
    ik_forward<Tbl, false>(q, t, p, J);
    const uint32_t am = poisoned ? 0u : a.alive[i];
    float best = 0.f;
    for (int k = 0; k < a.K; ++k) {
      if (!((am >> k) & 1u)) continue;
      const float* row = a.points + (int64_t)(3 * k) * a.ld;
      const float tx = row[i], ty = (row + a.ld)[i], tz = (row + 2 * a.ld)[i];
      const float dx = tx - p[0], dy = ty - p[1], dz = tz - p[2];
      const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
      if (idx < 0 || d2 < best) {  // (ascending k and a strict compare: the lowest index wins a tie)
        best = d2;
        idx = k;
        x[0] = tx;
        x[1] = ty;
        x[2] = tz;
      }
    }  // (resident targets are finite: every way into MT_F_POINTS is screened)
  }
  const bool held = poisoned || (!a.target && idx < 0);
  if (poisoned) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = 0.f;
  }
  bool frozen = held;
  int steps = 0;
  for (int it = 0; it < a.iters; ++it) {
    if (__ballot(!frozen) == 0ull) break;  // (wave-uniform)
    ik_forward<Tbl, true>(q, t, p, J);
    const float e0 = x[0] - p[0], e1 = x[1] - p[1], e2 = x[2] - p[2];
    const float box = fmaxf(fmaxf(fabsf(e0), fabsf(e1)), fabsf(e2));
    frozen |= (a.tol > 0.f) && (box <= a.tol);
    float a00 = a.lambda2, a11 = a.lambda2, a22 = a.lambda2, a01 = 0.f, a02 = 0.f, a12 = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      a00 = pfma(J[0][j], J[0][j], a00);
      a01 = pfma(J[0][j], J[1][j], a01);
      a02 = pfma(J[0][j], J[2][j], a02);
      a11 = pfma(J[1][j], J[1][j], a11);
      a12 = pfma(J[1][j], J[2][j], a12);
      a22 = pfma(J[2][j], J[2][j], a22);
    }
    // A = L D L^T, then L w = e, D v = w, L^T y = v
    const float i0 = 1.0f / a00;
    const float l10 = a01 * i0, l20 = a02 * i0;
    const float i1 = 1.0f / __builtin_fmaf(-l10, a01, a11);
    const float u12 = __builtin_fmaf(-l20, a01, a12);
    const float l21 = u12 * i1;
    const float i2 = 1.0f / __builtin_fmaf(-l21, u12, __builtin_fmaf(-l20, a02, a22));
    const float w1 = __builtin_fmaf(-l10, e0, e1);
    const float w2 = __builtin_fmaf(-l21, w1, __builtin_fmaf(-l20, e0, e2));
    const float y2 = w2 * i2;
    const float y1 = __builtin_fmaf(-l21, y2, w1 * i1);
    const float y0 = __builtin_fmaf(-l20, y2, __builtin_fmaf(-l10, y1, e0 * i0));
    float dq[D], m = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      dq[j] = kDegPerRad * pfma(J[2][j], y2, pfma(J[1][j], y1, pmul(J[0][j], y0)));
      m = fmaxf(m, fabsf(dq[j]));
    }
    const float scale = (m > a.max_step) ? a.max_step / m : 1.0f;  // (m > max_step > 0: never a division by 0)
    if (!frozen) {
#pragma unroll
      for (int j = 0; j < D; ++j) q[j] = __builtin_fmaf(dq[j], scale, q[j]);
      ++steps;
    }
  }
  float res;
  if (held) {
#pragma unroll
    for (int j = 0; j < D; ++j) q[j] = (a.start + j * a.start_ld)[i];
    res = poisoned ? __uint_as_float(0x7FC00000u) : 0.f;
  } else {
    if (a.wrap) {  // into [-180, 180): q - 360 k is exact in fp32 (the result is a smaller multiple of q's ulp)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        float r = __builtin_fmaf(__builtin_rintf(q[j] * (1.0f / 360.0f)), -360.0f, q[j]);
        r = (r >= 180.0f) ? r - 360.0f : r;
        q[j] = (r < -180.0f) ? r + 360.0f : r;
      }
    }
    ik_forward<Tbl, false>(q, t, p, J);
    res = fmaxf(fmaxf(fabsf(x[0] - p[0]), fabsf(x[1] - p[1])), fabsf(x[2] - p[2]));
  }
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if (a.angles) (a.angles + j * a.angles_ld)[i] = q[j];
    if (a.stage) (a.stage + j * a.ld)[i] = q[j];
  }
  if (a.residual) a.residual[i] = res;
  if (a.steps) a.steps[i] = steps;
  if (a.index) a.index[i] = idx;
}

// ---------------------------------------------------------------------------
// get_observations() at the current pose (manytor.py:141-153).
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void observe_kernel(const StepArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  const int64_t ld = a.ld;
  float s[D], c[D], p[D][3];
#pragma unroll
  for (int j = 0; j < D; ++j) sincos_deg_off((a.goals + j * ld)[i], a.dh.off_deg[j], s[j], c[j]);
  const RtTableF<D> t{a.dh};
  chain_all<RtTableF<D>>(s, c, t, p);
  float el[3], e_unused[3];
  pick_frames<RtTableF<D>>(t, p, el, e_unused);
  const uint32_t am = a.alive[i];
  for (int k = 0; k < a.K; ++k) {
    float* row = a.points + (int64_t)(3 * k) * ld;
    const float x = row[i], y = (row + ld)[i], z = (row + 2 * ld)[i];
    float dist = 0.f, r = 0.f, th = 0.f;
    if ((am >> k) & 1u) {
      observe_target(el, x, y, z, dist, r, th);
    } else if ((x != 0.f) | (y != 0.f) | (z != 0.f)) {
      row[i] = 0.f;
      (row + ld)[i] = 0.f;
      (row + 2 * ld)[i] = 0.f;
    }
    float* orow = a.obs + (int64_t)(3 * k) * ld;
    orow[i] = dist;
    (orow + ld)[i] = r;
    (orow + 2 * ld)[i] = th;
  }
}

// ---------------------------------------------------------------------------
// is_done() at the current pose (manytor.py:155-173).
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void check_done_kernel(const StepArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  const int64_t ld = a.ld;
  float s[D], c[D], p[D][3];
#pragma unroll
  for (int j = 0; j < D; ++j) sincos_deg_off((a.goals + j * ld)[i], a.dh.off_deg[j], s[j], c[j]);
  const RtTableF<D> t{a.dh};
  chain_all<RtTableF<D>>(s, c, t, p);
  float el_unused[3], e[3];
  pick_frames<RtTableF<D>>(t, p, el_unused, e);
  uint32_t am = a.alive[i];
  for (int k = 0; k < a.K; ++k) {
    if (!((am >> k) & 1u)) continue;
    const float* row = a.points + (int64_t)(3 * k) * ld;
    if (within_box(e, row[i], (row + ld)[i], (row + 2 * ld)[i], a.tol)) am &= ~(1u << k);
  }
  a.alive[i] = am;
  const bool done = (am == 0u);
  a.done[i] = done ? 1 : 0;
  const unsigned long long bits = __ballot(done);
  if ((threadIdx.x & 63) == 0) a.done_bits[i >> 6] = bits;
}

// joints_coordinates for all envs, env-major (N, D, 3): row 0 zeros, row j the
// frame after j+1 joints (manytor.py:188-189).
template <int D>
__global__ __launch_bounds__(kBlock) void joints_kernel(const StepArgs a, float* out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  const int64_t ld = a.ld;
  float s[D], c[D], p[D][3];
#pragma unroll
  for (int j = 0; j < D; ++j) sincos_deg_off((a.goals + j * ld)[i], a.dh.off_deg[j], s[j], c[j]);
  chain_all<RtTable<D>>(s, c, RtTable<D>{a.dh}, p);
  float* o = out + (int64_t)i * (3 * D);
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) o[3 * j + q] = (j == 0) ? 0.f : p[j][q];
}

// ---------------------------------------------------------------------------
// Layout conversion between the resident SoA rows and the reference's
// env-major arrays.  Off the hot path (host getters / setters only).
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void soa_to_env_major(const T* src, int64_t ld, int rows, int64_t n, T* dst) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  for (int r = 0; r < rows; ++r) dst[(int64_t)i * rows + r] = (src + (int64_t)r * ld)[i];
}

template <typename S>
__global__ __launch_bounds__(kBlock) void env_major_to_soa(const S* src, int rows, int64_t n, float* dst, int64_t ld) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  for (int r = 0; r < rows; ++r) (dst + (int64_t)r * ld)[i] = (float)src[(int64_t)i * rows + r];
}

template <typename S>
__global__ __launch_bounds__(kBlock) void soa_to_soa_f32(const S* src, int rows, int64_t n, int64_t ld, float* dst) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  for (int r = 0; r < rows; ++r) (dst + (int64_t)r * ld)[i] = (float)(src + (int64_t)r * ld)[i];
}

inline __global__ __launch_bounds__(kBlock) void alive_unpack(const uint32_t* mask, int K, int64_t n, uint8_t* dst) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  const uint32_t m = mask[i];
  for (int k = 0; k < K; ++k) dst[(int64_t)i * K + k] = (m >> k) & 1u;
}

inline __global__ __launch_bounds__(kBlock) void alive_pack(const uint8_t* src, int K, int64_t n, uint32_t* mask) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  uint32_t m = 0;
  for (int k = 0; k < K; ++k) m |= (src[(int64_t)i * K + k] ? 1u : 0u) << k;
  mask[i] = m;
}

// ---------------------------------------------------------------------------
// Stateless helpers: fk()/dh() (manytor.py:25-53) and r_theta() (:17-22).
// ---------------------------------------------------------------------------
struct FkArgs {
  const float* angles;  // (n, dof)
  float* out;           // (n, 16) row-major 4x4
  int64_t n;
  int dof, mode, radians;
  DhConst dh;
};

inline __global__ __launch_bounds__(kBlock) void fk_kernel(const FkArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= a.n) return;
  float X[3] = {1.f, 0.f, 0.f}, Y[3] = {0.f, 1.f, 0.f}, Z[3] = {0.f, 0.f, 1.f}, o[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < a.mode; ++j) {
    float ang = a.angles[(int64_t)i * a.dof + j];
    if (a.radians) ang *= 57.29577951308232f;
    float s, c;
    sincos_deg_off(ang, a.dh.off_deg[j], s, c);
    for (int q = 0; q < 3; ++q) {
      const float nx = __builtin_fmaf(X[q], c, Y[q] * s);
      const float tt = __builtin_fmaf(Y[q], c, -(X[q] * s));
      o[q] = __builtin_fmaf(a.dh.a[j], nx, __builtin_fmaf(a.dh.d[j], Z[q], o[q]));
      X[q] = nx;
      Y[q] = __builtin_fmaf(tt, a.dh.ca[j], Z[q] * a.dh.sa[j]);
      Z[q] = __builtin_fmaf(Z[q], a.dh.ca[j], -(tt * a.dh.sa[j]));
    }
  }
  float* m = a.out + (int64_t)i * 16;
  for (int q = 0; q < 3; ++q) {
    m[4 * q + 0] = X[q];
    m[4 * q + 1] = Y[q];
    m[4 * q + 2] = Z[q];
    m[4 * q + 3] = o[q];
  }
  m[12] = 0.f;
  m[13] = 0.f;
  m[14] = 0.f;
  m[15] = 1.f;
}

// Sub-step trajectory export: joints_coordinates at every one of the S poses of the
// route prev -> action (manytor.py:182-190), for a handful of envs the host wants to draw or log.  One thread per
// (env, sub-step); every pose gets the full polynomial sincos (this is not the timed path).
struct TraceArgs {
  const float* prev;    // (n, dof) degrees
  const float* action;  // (n, dof)
  float* out;           // (n, S, dof, 3)
  int64_t n;
  int dof, S;
  DhConst dh;
};

inline __global__ __launch_bounds__(kBlock) void route_trace_kernel(const TraceArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= a.n * a.S) return;
  const int64_t env = gid / a.S;
  const int k = (int)(gid % a.S);
  const float inv = 1.0f / (float)(a.S - 1);
  float X[3] = {1.f, 0.f, 0.f}, Y[3] = {0.f, 1.f, 0.f}, Z[3] = {0.f, 0.f, 1.f}, o[3] = {0.f, 0.f, 0.f};
  float* out = a.out + gid * (int64_t)(3 * a.dof);
  for (int j = 0; j < a.dof; ++j) {
    const float g = a.prev[env * a.dof + j], act = a.action[env * a.dof + j];
    // np.linspace: start + k * step, last element = stop exactly (manytor.py:182)
    float s, c;
    if (wide_angle(g) | wide_angle(act)) {  // see route_kinematics_wide
      if (k == a.S - 1)
        sincos_deg_off(act, a.dh.off_deg[j], s, c);
      else
        sincos_deg_route(g, act, (double)k / (double)(a.S - 1), a.dh.off_deg[j], s, c);
    } else {
      const float pose = (k == a.S - 1) ? act : __builtin_fmaf((float)k, (act - g) * inv, g);
      sincos_deg(pose + a.dh.off_deg[j], s, c);
    }
    for (int q = 0; q < 3; ++q) {
      const float nx = __builtin_fmaf(X[q], c, Y[q] * s);
      const float tt = __builtin_fmaf(Y[q], c, -(X[q] * s));
      o[q] = __builtin_fmaf(a.dh.a[j], nx, __builtin_fmaf(a.dh.d[j], Z[q], o[q]));
      X[q] = nx;
      Y[q] = __builtin_fmaf(tt, a.dh.ca[j], Z[q] * a.dh.sa[j]);
      Z[q] = __builtin_fmaf(Z[q], a.dh.ca[j], -(tt * a.dh.sa[j]));
      out[3 * j + q] = (j == 0) ? 0.f : o[q];   // row 0 is zeros, row j the frame after j+1 joints (manytor.py:189)
    }
  }
}

inline __global__ __launch_bounds__(kBlock) void r_theta_kernel(const float* v1, const float* v2, int64_t n, float* out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // 32-bit lane offset: rows are addressed as uniform base + i
  if (i >= n) return;
  const int64_t b3 = 3 * (int64_t)i;
  const float d0 = fabsf(v1[b3] - v2[b3]), d1 = fabsf(v1[b3 + 1] - v2[b3 + 1]), d2 = fabsf(v1[b3 + 2] - v2[b3 + 2]);
  const float h = __builtin_amdgcn_sqrtf(__builtin_fmaf(d0, d0, d1 * d1));
  out[2 * (int64_t)i] = atan2_deg_q1(d0, d1);
  out[2 * (int64_t)i + 1] = atan2_deg_q1(h, d2);
}

// ---------------------------------------------------------------------------
// Streaming yardstick (mt_stream_probe): the step kernel's memory operations with none of its arithmetic -- per env the
// D + 3K + 2 state rows are read (goals, targets, alive mask, return), D + 2 of them are written back in place (plain
// stores: goals, alive mask, return), and 3K + 4 output rows (obs, reward, end effector) plus one byte row (done) are
// written with non-temporal stores: exactly the 8 D + 24 K + 33 bytes per env mt_step_random moves, with the same row
// addressing (SGPR row base + 32-bit lane offset) and one env per lane.  What this kernel reaches on a box is what the
// step kernel's access shape can reach there; bench.py quotes the step against it (roofline.achievable_gbs).
// ---------------------------------------------------------------------------
template <int D, int K>
__global__ __launch_bounds__(kBlock) void stream_probe_kernel(float* state, float* out, uint8_t* bytes, int64_t n, int64_t ld) {
  constexpr int RD = D + 3 * K + 2, WP = D + 2, WN = 3 * K + 4;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  LaneOffset<true> o4{i * 4u}, o1{i};
  if (i >= n) return;
  float v[RD], acc = 0.f;
#pragma unroll
  for (int r = 0; r < RD; ++r) {
    v[r] = ldr(state + (int64_t)r * ld, o4);
    acc += v[r];
  }
  acc *= 1e-30f;  // keeps every load alive without letting the state drift
#pragma unroll
  for (int r = 0; r < WN; ++r) str_stream(out + (int64_t)r * ld, o4, v[r % RD] + acc);
#pragma unroll
  for (int r = 0; r < WP; ++r) {  // the rows the step rewrites in place: goals (rows 0 .. D-1) and the last two
    const int row = r < D ? r : RD - 2 + (r - D);
    str(state + (int64_t)row * ld, o4, v[row] + acc);
  }
  str_stream(bytes, o1, (uint8_t)(acc > 1.f ? 1 : 0));
}

}  // namespace mt
