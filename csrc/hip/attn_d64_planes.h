// The K / V plane workspace of the head-dim-64 attention (attention_f32x.hip):
// the one definition its writers -- the QKV epilogues of gemm_f32x.hip and
// gemm_f32h.hip, split_kv_kernel -- and its readers, the two attention
// kernels, share.
//
//   kvs[b][s][plane][H * 64], s < padded_keys(Skv), 16-bit elements;
//   bf16x6: planes K0 K1 K2 V0 V1 V2, fp16x3: planes K hi, K lo, V hi, V lo.
//
// A batch's rows are padded to whole key tiles; the rows past Skv are never
// read (the attention's tail tile re-reads the last key).
#pragma once
#include "common.h"

namespace nos {
namespace kvp {

constexpr int KVB = 32;     // keys per tile
constexpr int X6 = 6;       // planes per token, bf16x6
constexpr int H3 = 4;       // planes per token, fp16x3

__host__ __device__ constexpr int padded_keys(int Skv) { return (Skv + KVB - 1) / KVB * KVB; }

// Bytes of the planes at the start of the attention's workspace: room for six
// planes per token under either layout (the partials follow at this offset).
inline long long planes_bytes(int B, int H, int Skv) {
  return ((long long)B * padded_keys(Skv) * X6 * H * 64 * 2 + 15) / 16 * 16;
}

// A fused QKV projection's K / V columns (>= qcols; K then V, hd = H * 64
// each) as planes: S rows per batch padded to skvp = padded_keys(S); with
// kvsc the fp16x3 planes, each head on the power-of-two scale kvsc[0 / 1][head],
// without it the bf16x6 planes.
struct KvOut {
  unsigned short* kvs = nullptr;
  const float* kvsc = nullptr;
  int qcols = 0, hd = 0, S = 0, skvp = 0;
};

// the caller's padded row count is the layout's own
inline bool skvp_ok(int S, int skvp) { return S > 0 && skvp == padded_keys(S); }

// Token (b, s) is row b * skvp + s; with NP planes per token of ld elements,
// tensor t (0: K, 1: V), piece p, column c of a row is element
//   (row * NP + NP / 2 * t + p) * ld + c.
// The GEMM epilogues and split_kv_kernel spell this inline from NP = X6 / H3
// (a helper call moved their instruction schedules).

// batch b's first token
template <int NP, class T>
__device__ __forceinline__ T* batch_planes(T* kvs, int b, int skvp, int ld) {
  return kvs + (long long)b * skvp * (NP * ld);
}

}  // namespace kvp
}  // namespace nos
