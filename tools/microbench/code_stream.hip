// Would reading each target as an 8-byte draw code instead of three floats speed up the 1 M step?  The streaming yardstick
// of probe_alu.hip (the rows of one mt_step_random read / rewritten / nt-written per env, one env per lane, every load first,
// then ALU independent fused multiply-adds, then every store) with the K targets read in one of two layouts:
//   F: 3 K float rows (12 B per target, today's MT_F_POINTS)
//   C: 2 K uint32 rows (8 B per target: the 63-bit code of the three 21-bit Philox fields)
// Per pass: goals D, alive, return read and rewritten; obs 3 K, reward, ee 3 and done byte nt-written.  The two layouts run
// alternately, several rounds, in two launches of n / 2 envs on two streams (the chained dispatch of the library at 1 M).
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize tools/microbench/code_stream.hip -o tools/microbench/code_stream
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr int D = 4, K = 7, WP = D + 2, WN = 3 * K + 4, BLOCK = 256;

template <bool CODES, int ALU>
__global__ __launch_bounds__(BLOCK) void k_stream(float* state, const float* pts, float* out, unsigned char* bytes, long n, long ld) {
  constexpr int TR = CODES ? 2 * K : 3 * K;  // target rows
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  float v[WP], t[TR], acc = 0.f;
#pragma unroll
  for (int r = 0; r < WP; ++r) v[r] = state[(long)r * ld + i];
#pragma unroll
  for (int r = 0; r < TR; ++r) t[r] = pts[(long)r * ld + i];
#pragma unroll
  for (int r = 0; r < WP; ++r) acc += v[r];
  if (CODES) {  // what a decode costs: the three fields out of two words, converted and scaled (x, y, z of target k)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned lo = __float_as_uint(t[2 * k]), hi = __float_as_uint(t[2 * k + 1]);
      const float x = (float)(lo & 0x1FFFFFu) * 4.76837158203125e-07f, y = (float)((lo >> 21) | ((hi & 0x3FFu) << 11)) * 4.76837158203125e-07f,
                  z = (float)(hi >> 10) * 4.76837158203125e-07f;
      acc += x + y + z;
    }
  } else {
#pragma unroll
    for (int r = 0; r < TR; ++r) acc += t[r];
  }
  float c0 = v[0], c1 = v[1], c2 = v[2], c3 = v[3], c4 = v[4], c5 = v[5], c6 = acc, c7 = acc;
  const float m = 1.0000001f, a = 1e-9f;
  for (int it = 0; it < ALU / 8; ++it) {
    c0 = __builtin_fmaf(c0, m, a);
    c1 = __builtin_fmaf(c1, m, a);
    c2 = __builtin_fmaf(c2, m, a);
    c3 = __builtin_fmaf(c3, m, a);
    c4 = __builtin_fmaf(c4, m, a);
    c5 = __builtin_fmaf(c5, m, a);
    c6 = __builtin_fmaf(c6, m, a);
    c7 = __builtin_fmaf(c7, m, a);
  }
  acc = (acc + c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7) * 1e-30f;
#pragma unroll
  for (int r = 0; r < WN; ++r) __builtin_nontemporal_store(acc + (float)r, out + (long)r * ld + i);
#pragma unroll
  for (int r = 0; r < WP; ++r) state[(long)r * ld + i] = v[r] + acc;
  __builtin_nontemporal_store((unsigned char)(acc > 1.f ? 1 : 0), bytes + i);
}

struct Bufs {
  float *state, *pts, *out;
  unsigned char* bytes;
};

template <bool CODES, int ALU>
static float run(const Bufs& b, long n, long ld, hipStream_t* st, int reps) {
  const long per = n / 2;
  auto pass = [&]() {
    for (int c = 0; c < 2; ++c)
      hipLaunchKernelGGL((k_stream<CODES, ALU>), dim3((unsigned)(per / BLOCK)), dim3(BLOCK), 0, st[c], b.state + c * per, b.pts + c * per,
                         b.out + c * per, b.bytes + c * per, per, ld);
  };
  for (int w = 0; w < 5; ++w) pass();
  (void)hipDeviceSynchronize();
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, st[0]);
  for (int r = 0; r < reps; ++r) pass();
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e1, st[0]);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms * 1e3f / reps;
}

static float median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 5;
  hipStream_t st[2];
  (void)hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking);
  (void)hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking);
  for (long n : {1048576L, 4194304L}) {
    const long ld = n + 256;
    Bufs b;
    if (hipMalloc(&b.state, (size_t)WP * ld * 4) != hipSuccess || hipMalloc(&b.pts, (size_t)3 * K * ld * 4) != hipSuccess ||
        hipMalloc(&b.out, (size_t)WN * ld * 4) != hipSuccess || hipMalloc(&b.bytes, (size_t)ld) != hipSuccess)
      return 1;
    (void)hipMemset(b.state, 0, (size_t)WP * ld * 4);
    (void)hipMemset(b.pts, 0, (size_t)3 * K * ld * 4);
    const double mbf = (double)(8 * WP + 12 * K + 4 * WN + 1) * n / 1e6, mbc = (double)(8 * WP + 8 * K + 4 * WN + 1) * n / 1e6;
    std::vector<float> f0, c0, f1, c1;
    for (int r = 0; r < rounds; ++r) {  // interleaved: F and C alternate inside every round
      f0.push_back(run<false, 0>(b, n, ld, st, 200));
      c0.push_back(run<true, 0>(b, n, ld, st, 200));
      f1.push_back(run<false, 1024>(b, n, ld, st, 200));
      c1.push_back(run<true, 1024>(b, n, ld, st, 200));
    }
    printf("%ld envs, two launches of %ld; F = %d float target rows (%.1f MB per pass), C = %d code rows (%.1f MB)\n", n, n / 2, 3 * K, mbf,
           2 * K, mbc);
    for (int r = 0; r < rounds; ++r)
      printf("  round %d: ALU 0  F %7.2f  C %7.2f us | ALU 1024  F %7.2f  C %7.2f us\n", r, f0[r], c0[r], f1[r], c1[r]);
    const float mf0 = median(f0), mc0 = median(c0), mf1 = median(f1), mc1 = median(c1);
    printf("  median: ALU 0  F %7.2f  C %7.2f us (C faster by %5.1f %%) | ALU 1024  F %7.2f  C %7.2f us (C faster by %5.1f %%)\n", mf0, mc0,
           100.0 * (mf0 - mc0) / mf0, mf1, mc1, 100.0 * (mf1 - mc1) / mf1);
    (void)hipFree(b.state);
    (void)hipFree(b.pts);
    (void)hipFree(b.out);
    (void)hipFree(b.bytes);
  }
  return 0;
}
