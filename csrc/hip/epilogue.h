// GEMM / GEMV epilogue flags (the `epi` argument of the host entry points)
// and the erf approximations of the GELU epilogues.
#pragma once
#include "common.h"

// One numbering for every kernel family; an entry point rejects or ignores
// the flags its kernels do not honour.  Python mirrors: nos_amd/ops/__init__.py
// (EPI_BIAS .. EPI_RELU) and nos_amd/ops/tenant.py (EPI_BIAS_ROW,
// EPI_RESID_PRE, EPI_SILU, EPI_GLU).
enum : int {
  EPI_BIAS = 1,        // + bias[n]: every GEMM (gemm*.hip) and decode.hip's GEMVs
  EPI_GELU = 2,        // erf GELU: every GEMM and the GEMVs
  EPI_RESID = 4,       // + R after the activation (transformer residuals): every GEMM and the GEMVs
  EPI_RELU = 8,        // every GEMM and the GEMVs
  EPI_BIAS_ROW = 16,   // + bias[m] (a conv's output channel): gemm_f32h.hip, batched entry only
  EPI_RESID_PRE = 32,  // + R before the activation (ResNet: relu(conv + bn + identity)): gemm_f32h.hip, batched only
  EPI_SILU = 64,       // decode.hip's GEMVs
  EPI_WIDE = 128,      // host-internal, never part of the API: gemm_f32h.hip's launcher sets it for interior
                       // tiles written as fp16 planes to leave through LDS as 16-byte row stores
  EPI_GLU = 256,       // decode.hip's GEMV: W = [gate; up] (2 Nh rows), y [M, Nh] = silu(x . gate_n) * (x . up_n)
};

namespace nos {

// erf by Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7 (far below bf16 output
// precision, and below the fp32 GEMMs' own error bounds), in two forms:
//  * erf_hw: on the hardware reciprocal and exp2 (v_rcp_f32 / v_exp_f32, ~1
//    ulp each) -- an IEEE division and expf's range reduction cost ~15 more
//    VALU per element, and fc1's GELU epilogue is the largest VALU block of
//    the h3 GEMMs (gemm_f32h.hip; gemm.hip's gelu_erf2 is the same on register pairs);
//  * erf_ieee: IEEE divide and expf (gemm_f32.hip, gemm_f32x.hip).
__device__ __forceinline__ float erf_hw(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-ax * ax * 1.4426950408889634f);  // exp(-x^2); 0 past |x| ~ 10
  const float r = fmaf(-p * t, e, 1.f);
  return copysignf(r, x);
}

__device__ __forceinline__ float erf_ieee(float x) {
  const float ax = fabsf(x);
  const float t = 1.f / fmaf(0.3275911f, ax, 1.f);
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float r = fmaf(-p * t, expf(-ax * ax), 1.f);
  return copysignf(r, x);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erf_hw(x * 0.70710678118654752f)); }

}  // namespace nos
