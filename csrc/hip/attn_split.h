// Key splits of the attention kernels (attention_f32x.hip, attention_h3g.hip):
// when one workgroup per query block leaves resident-workgroup slots of the
// (budgeted) CUs empty, the keys are split so the grid fills them; every split
// stores an unnormalised partial (O, m, l) and a merge kernel combines them.
// Partial buffer: O [nsplit][B * Sq][H * D] fp32, then (m, l) pairs
// [nsplit][B * Sq][H][2]; m in log2 units, O on the unit scale.  Each including
// source gets its own copy of the kernel (internal linkage) under its own flags.
#pragma once
#include "common.h"
#include "split_f16.h"

namespace {

constexpr int MAX_SPLIT = 4;

// Number of key splits: `forced` (a set_kvsplit knob; 0 = auto: fill the
// wg_per_cu slots of the CUs), at most MAX_SPLIT and never so fine that a
// split has no tile.
inline int pick_split(int forced, long long nwg1, int ntiles, int wg_per_cu) {
  int n = forced;
  if (n == 0) {
    const long long slots = (long long)wg_per_cu * nos_effective_cus();
    n = nwg1 >= slots ? 1 : (int)(slots / nwg1);
  }
  n = n < 1 ? 1 : (n > MAX_SPLIT ? MAX_SPLIT : n);
  while (n > 1 && (long long)(n - 1) * ((ntiles + n - 1) / n) >= ntiles) --n;  // the last split non-empty
  return n;
}

// room for MAX_SPLIT partials
inline long long part_bytes(int B, int H, int Sq, int D) { return (long long)MAX_SPLIT * B * Sq * H * (D + 2) * 4; }

__host__ __device__ __forceinline__ long long part_row(int sp, int B, int b, int Sq, int s) {
  return ((long long)sp * B + b) * Sq + s;
}
// head h's D partial outputs of a row (ldh = H * D)
__host__ __device__ __forceinline__ float* part_o(float* part, long long row, int ldh, int D, int h) {
  return part + row * ldh + h * D;
}
// head h's (m, l) of a row
__host__ __device__ __forceinline__ float* part_ml(float* part, int nsplit, int B, int Sq, int H, int ldh,
                                                   long long row, int h) {
  return part + (long long)nsplit * B * Sq * ldh + (row * H + h) * 2;
}

// Merge, per (batch, row, head) and 4 dims: O = sum_i O_i 2^(m_i - M) /
// sum_i l_i 2^(m_i - M), M = max_i m_i.  DC: the head dim when it is a
// compile-time constant, 0 = the runtime D.  PLANES: O as the next h3 GEMM's A
// planes (hi at op, lo at op + opl) on the scale osc instead of fp32 o.  LSE:
// also each row's log-sum-exp (natural log) to lse [B][H][Sq].
template <int DC, bool PLANES, bool LSE>
__global__ __launch_bounds__(256) void merge_splits_kernel(float* __restrict__ part, float* __restrict__ o, int B,
                                                           int H, int Drt, int Sq, int nsplit, int ldo, long long bso,
                                                           long long n4, float* __restrict__ lse,
                                                           _Float16* __restrict__ op, long long opl, float osc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int D = DC ? DC : Drt;
  const int ldh = H * D;
  const long long row = i / (ldh / 4);               // b * Sq + s
  const int col = (int)(i - row * (ldh / 4)) * 4;    // h * D + d
  const int h = col / D;
  const long long b = row / Sq, s = row - b * Sq;
  float mx = -INFINITY;
  for (int sp = 0; sp < nsplit; ++sp)
    mx = fmaxf(mx, *part_ml(part, nsplit, B, Sq, H, ldh, part_row(sp, B, (int)b, Sq, (int)s), h));
  float L = 0.f;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < nsplit; ++sp) {
    const long long r = part_row(sp, B, (int)b, Sq, (int)s);
    const float* ml = part_ml(part, nsplit, B, Sq, H, ldh, r, h);
    const float a = __builtin_amdgcn_exp2f(ml[0] - mx);
    L = fmaf(ml[1], a, L);
    const float4 v = *reinterpret_cast<const float4*>(part_o(part, r, ldh, D, 0) + col);
    acc.x = fmaf(v.x, a, acc.x);
    acc.y = fmaf(v.y, a, acc.y);
    acc.z = fmaf(v.z, a, acc.z);
    acc.w = fmaf(v.w, a, acc.w);
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;  // every split empty (a cache row that sees no key): zeros
  const float4 y = float4{acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv};
  if constexpr (PLANES) {
    f16x2_t h01, l01, h23, l23;
    nos::split2h(f32x2_t{y.x * osc, y.y * osc}, h01, l01);
    nos::split2h(f32x2_t{y.z * osc, y.w * osc}, h23, l23);
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
    *reinterpret_cast<f16x4_t*>(op + b * bso + s * ldo + col) = f16x4_t{h01.x, h01.y, h23.x, h23.y};
    *reinterpret_cast<f16x4_t*>(op + opl + b * bso + s * ldo + col) = f16x4_t{l01.x, l01.y, l23.x, l23.y};
  } else {
    *reinterpret_cast<float4*>(o + b * bso + s * ldo + col) = y;
  }
  if constexpr (LSE) {
    if (col == h * D)
      lse[(b * H + h) * Sq + s] = fmaf(mx, 0.6931471805599453f, __builtin_amdgcn_logf(L) * 0.6931471805599453f);
  }
}

template <int DC, bool PLANES, bool LSE>
int run_merge(float* part, float* o, int B, int H, int D, int Sq, int nsplit, int ldo, long long bso,
              hipStream_t stream, float* lse = nullptr, _Float16* op = nullptr, long long opl = 0, float osc = 1.f) {
  const long long n4 = (long long)B * Sq * H * (D / 4);
  hipLaunchKernelGGL((merge_splits_kernel<DC, PLANES, LSE>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream,
                     part, o, B, H, D, Sq, nsplit, ldo, bso, n4, lse, op, opl, osc);
  return (int)hipGetLastError();
}

}  // namespace
