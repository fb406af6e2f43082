// The K / V pre-pass of the general h3 attention (attention_h3g.hip) and its
// backward (attention_h3g_bwd.hip): measure max |k|, |v| per (batch, kv head),
// turn them into power-of-two scales and write K / V as four fp16 planes per
// token.  Each including source gets its own copy of the kernels (internal
// linkage); both sources produce the same planes from the same K / V.
//
//  1. kv_absmax: max |k| and |v| per (batch, kv head) over row chunks;
//  2. kv_scale: the power of two that puts each head's max just under 2^14
//     (for rotated keys: the host's bound max|cos| + max|sin| on top);
//  3. split_kv: K (rotated on the fly) and V as four fp16 planes per token,
//     [b][kv head][token][K hi, K lo, V hi, V lo][D], 16-byte stores.
//
// 1' and 3' are their forms over a K / V cache at device-side counters (the
// forward over caches, attention_h3g.hip nos_attn_h3g_cache*): only the rows
// the step attends are read.
//
// Below the kernels: what the two host paths share -- the padded sizes, the
// launches of the pre-pass and the argument checks of the entry points.
#pragma once
#include "common.h"
#include "kv_ring.h"
#include "split_f16.h"

namespace {

constexpr int KVB = 32;                 // keys per tile
constexpr int ABS_ROWS = 256;           // rows per absmax chunk

__host__ __device__ constexpr int padded_keys(int Skv) { return (Skv + KVB - 1) / KVB * KVB; }  // whole tiles
constexpr int abs_chunks(int S) { return (S + ABS_ROWS - 1) / ABS_ROWS; }
constexpr long long align256(long long x) { return (x + 255) / 256 * 256; }  // workspace sections

__device__ __forceinline__ float xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

__device__ __forceinline__ float xor32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---------------------------------------------------------------- 1. absmax
// part[(bh * nchunk + chunk) * 2 + (0: K, 1: V)] = max |x| over the chunk's rows
__global__ __launch_bounds__(256) void kv_absmax_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                        float* __restrict__ part, int S, int Hkv, int D, int ldk,
                                                        long long bsk, int ldv, long long bsv, int nchunk) {
  __shared__ float red[2][4];
  const int bh = blockIdx.y, chunk = blockIdx.x;
  const int b = bh / Hkv, h = bh - b * Hkv;
  const int r0 = chunk * ABS_ROWS, r1 = min(S, r0 + ABS_ROWS);
  const int d4 = D / 4;
  const int n = (r1 - r0) * d4;
  float mk = 0.f, mv = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int r = r0 + i / d4, c = (i % d4) * 4;
    const float4 a = *reinterpret_cast<const float4*>(k + b * bsk + (long long)r * ldk + h * D + c);
    const float4 e = *reinterpret_cast<const float4*>(v + b * bsv + (long long)r * ldv + h * D + c);
    mk = fmaxf(mk, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
    mv = fmaxf(mv, fmaxf(fmaxf(fabsf(e.x), fabsf(e.y)), fmaxf(fabsf(e.z), fabsf(e.w))));
  }
  mk = nos::wave_max(mk);
  mv = nos::wave_max(mv);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mk;
    red[1][threadIdx.x >> 6] = mv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* r = red[threadIdx.x];
    part[((long long)bh * nchunk + chunk) * 2 + threadIdx.x] = fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
  }
}

// ---------------------------------------------------------------- 2. scales
// kvsc[bh * 2 + t] = 2^e with (max_t * bound_t) 2^e < 2^14 (bound: K's rotary growth)
__global__ __launch_bounds__(256) void kv_scale_kernel(const float* __restrict__ part, float* __restrict__ kvsc,
                                                       int n, int nchunk, float kbound) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int bh = i >> 1, t = i & 1;
  float m = 0.f;
  for (int c = 0; c < nchunk; ++c) m = fmaxf(m, part[((long long)bh * nchunk + c) * 2 + t]);
  kvsc[i] = nos::pow2i(nos::h3_scale_exp(t == 0 ? m * kbound : m));
}

// ---------------------------------------------------------------- 3. split
// one thread: 8 dims of one (b, kv head, token, K|V): planes
// kvs[(bh * skvp + s) * 4 + 2t + piece][D]; K rotated first when cos != null
// (rows of the [Skv][D] tables = key positions)
__global__ __launch_bounds__(256) void split_kv_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                       const float* __restrict__ kvsc, _Float16* __restrict__ kvs,
                                                       int S, int skvp, int Hkv, int D, int ldk, long long bsk,
                                                       int ldv, long long bsv, const float* __restrict__ rc,
                                                       const float* __restrict__ rs, long long n8) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c8 = D / 8;
  const int ch = (int)(i % c8);
  long long rest = i / c8;
  const int t = (int)(rest & 1);
  rest >>= 1;
  const int s = (int)(rest % S);
  const int bh = (int)(rest / S);
  const int b = bh / Hkv, h = bh - b * Hkv;
  const float* src = t == 0 ? k + b * bsk + (long long)s * ldk + h * D : v + b * bsv + (long long)s * ldv + h * D;
  float x[8];
  {
    const float4 a = *reinterpret_cast<const float4*>(src + ch * 8);
    const float4 e = *reinterpret_cast<const float4*>(src + ch * 8 + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = e.x; x[5] = e.y; x[6] = e.z; x[7] = e.w;
  }
  if (t == 0 && rc != nullptr) {  // rotate_half: partner chunk D/16 away
    const int half = c8 / 2;
    const bool lo = ch < half;
    const int pc = lo ? ch + half : ch - half;
    const float4 a = *reinterpret_cast<const float4*>(src + pc * 8);
    const float4 e = *reinterpret_cast<const float4*>(src + pc * 8 + 4);
    const float p[8] = {a.x, a.y, a.z, a.w, e.x, e.y, e.z, e.w};
    const float* cr = rc + (long long)s * D + ch * 8;
    const float* sr = rs + (long long)s * D + ch * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = lo ? fmaf(x[j], cr[j], -p[j] * sr[j]) : fmaf(x[j], cr[j], p[j] * sr[j]);
  }
  f16x8_t hi, lo;
  nos::split8h(x, kvsc[bh * 2 + t], hi, lo);
  _Float16* dst = kvs + (((long long)bh * skvp + s) * 4 + 2 * t) * D + ch * 8;
  *reinterpret_cast<f16x8_t*>(dst) = hi;
  *reinterpret_cast<f16x8_t*>(dst + D) = lo;
}

// ---------------------------------------------------------------- 1', 3': over a K / V cache
// The pre-pass of the flash attention over K / V caches [B, L, Hkv, D] (contiguous fp32, keys stored
// rotated) at the device-side counters pos [B]: only the rows the step of Sq tokens at pos[b] attends
// are read -- stale rows (a rejected draft's, a sequence's from before a reset, a ring's never written
// slots) neither set the scales nor reach the planes.
struct CacheStep {
  const int* pos;    // i32 [B]
  int Sq, W, limit;  // W == 0: a plain cache; else a ring of L slots (kv_ring.h)
  int R;             // rows of the attention's rotary tables for Q (row pos[b] + i, clamped)
};

// row (slot) s of sequence b's caches is read: plain, s < min(pos[b], L) + Sq (the keys 0 .. the last
// query's); a ring, slot s holds a position some query row sees (>= the first row's oldest) -- none at a
// counter outside [0, limit)
__device__ __forceinline__ bool cache_row_live(int s, int p0, int L, const CacheStep& cs) {
  if (cs.W == 0) return s < min(p0, L) + cs.Sq;
  if (p0 < 0 || p0 >= cs.limit) return false;
  const int pmax = p0 + cs.Sq - 1;
  return nos::ring_position(s, pmax, L) >= nos::ring_oldest(p0, pmax, L, cs.W);
}

// kv_absmax_kernel over the live rows of the caches
__global__ __launch_bounds__(256) void kv_absmax_cache_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                              float* __restrict__ part, int L, int Hkv, int D,
                                                              int nchunk, CacheStep cs) {
  __shared__ float red[2][4];
  const int bh = blockIdx.y, chunk = blockIdx.x;
  const int b = bh / Hkv, h = bh - b * Hkv;
  const int p0 = cs.pos[b];
  const int r0 = chunk * ABS_ROWS, r1 = min(L, r0 + ABS_ROWS);
  const int d4 = D / 4;
  const int n = (r1 - r0) * d4;
  float mk = 0.f, mv = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int r = r0 + i / d4, c = (i % d4) * 4;
    if (!cache_row_live(r, p0, L, cs)) continue;
    const long long at = (((long long)b * L + r) * Hkv + h) * D + c;
    const float4 a = *reinterpret_cast<const float4*>(k + at);
    const float4 e = *reinterpret_cast<const float4*>(v + at);
    mk = fmaxf(mk, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
    mv = fmaxf(mv, fmaxf(fmaxf(fabsf(e.x), fabsf(e.y)), fmaxf(fabsf(e.z), fabsf(e.w))));
  }
  mk = nos::wave_max(mk);
  mv = nos::wave_max(mv);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mk;
    red[1][threadIdx.x >> 6] = mv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const float* r = red[threadIdx.x];
    part[((long long)bh * nchunk + chunk) * 2 + threadIdx.x] = fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
  }
}

// split_kv_kernel over the caches (no rotation: the keys are stored rotated): the planes of the live
// rows; a ring's other slots get zero planes (the attention walks every slot), a plain cache's rows past
// the step are not written (the attention never loads them)
__global__ __launch_bounds__(256) void split_kv_cache_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                             const float* __restrict__ kvsc,
                                                             _Float16* __restrict__ kvs, int L, int skvp, int Hkv,
                                                             int D, long long n8, CacheStep cs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int c8 = D / 8;
  const int ch = (int)(i % c8);
  long long rest = i / c8;
  const int t = (int)(rest & 1);
  rest >>= 1;
  const int s = (int)(rest % L);
  const int bh = (int)(rest / L);
  const int b = bh / Hkv, h = bh - b * Hkv;
  const bool live = cache_row_live(s, cs.pos[b], L, cs);
  if (!live && cs.W == 0) return;
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* src = (t == 0 ? k : v) + (((long long)b * L + s) * Hkv + h) * D + ch * 8;
    const float4 a = *reinterpret_cast<const float4*>(src);
    const float4 e = *reinterpret_cast<const float4*>(src + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = e.x; x[5] = e.y; x[6] = e.z; x[7] = e.w;
  }
  f16x8_t hi, lo;
  nos::split8h(x, kvsc[bh * 2 + t], hi, lo);
  _Float16* dst = kvs + (((long long)bh * skvp + s) * 4 + 2 * t) * D + ch * 8;
  *reinterpret_cast<f16x8_t*>(dst) = hi;
  *reinterpret_cast<f16x8_t*>(dst + D) = lo;
}

// ---------------------------------------------------------------- host
// a [B, S, heads, D] fp32 operand: token row stride ld, batch stride bs (floats)
struct Rows {
  const float* p;
  int ld;
  long long bs;
  bool ok(int heads, int D) const {
    return p != nullptr && ((uintptr_t)p & 15) == 0 && ld >= heads * D && (ld & 3) == 0 && (bs & 3) == 0;
  }
};

// the absmax launch: a / b [nb / heads, S, heads, D] -> part[nb][abs_chunks(S)][2]
inline void launch_absmax(const Rows& a, const Rows& b, float* part, int nb, int S, int heads, int D,
                          hipStream_t stream) {
  const int nchunk = abs_chunks(S);
  hipLaunchKernelGGL(kv_absmax_kernel, dim3((unsigned)nchunk, (unsigned)nb), dim3(256), 0, stream, a.p, b.p, part, S,
                     heads, D, a.ld, a.bs, b.ld, b.bs, nchunk);
}

// the three launches: k / v [B, Skv, Hkv, D] -> absmax partials, scales kvsc
// [B * Hkv][2] and planes kvs (padded_keys(Skv) rows per head); rc / rs: the
// rotary tables of K (or null) under the bound kbound
inline void launch_kv_prepass(const Rows& k, const Rows& v, float* absmax, float* kvsc, _Float16* kvs, int B, int Hkv,
                              int Skv, int D, float kbound, const float* rc, const float* rs, hipStream_t stream) {
  const int nbh = B * Hkv;
  launch_absmax(k, v, absmax, nbh, Skv, Hkv, D, stream);
  hipLaunchKernelGGL(kv_scale_kernel, dim3((unsigned)((2 * nbh + 255) / 256)), dim3(256), 0, stream, absmax, kvsc,
                     2 * nbh, abs_chunks(Skv), kbound);
  const long long n8 = (long long)nbh * Skv * 2 * (D / 8);
  hipLaunchKernelGGL(split_kv_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, k.p, v.p, kvsc, kvs, Skv,
                     padded_keys(Skv), Hkv, D, k.ld, k.bs, v.ld, v.bs, rc, rs, n8);
}

// the three launches over caches kc / vc [B, L, Hkv, D]: grids sized from L alone, the rows read
// bounded by the device-side counters (cs)
inline void launch_kv_cache_prepass(const float* kc, const float* vc, float* absmax, float* kvsc, _Float16* kvs, int B,
                                    int Hkv, int L, int D, const CacheStep& cs, hipStream_t stream) {
  const int nbh = B * Hkv, nchunk = abs_chunks(L);
  hipLaunchKernelGGL(kv_absmax_cache_kernel, dim3((unsigned)nchunk, (unsigned)nbh), dim3(256), 0, stream, kc, vc,
                     absmax, L, Hkv, D, nchunk, cs);
  hipLaunchKernelGGL(kv_scale_kernel, dim3((unsigned)((2 * nbh + 255) / 256)), dim3(256), 0, stream, absmax, kvsc,
                     2 * nbh, nchunk, 1.f);
  const long long n8 = (long long)nbh * L * 2 * (D / 8);
  hipLaunchKernelGGL(split_kv_cache_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, kc, vc, kvsc, kvs,
                     L, padded_keys(L), Hkv, D, n8, cs);
}

// the checks every entry point makes; need: its workspace function (-1 for bad dims)
inline bool attn_dims_ok(int B, int H, int Hkv, int Sq, int Skv, int D) {
  return B > 0 && H > 0 && Hkv > 0 && Sq > 0 && Skv > 0 && (D == 64 || D == 128);
}
inline bool attn_call_ok(int B, int H, int Hkv, int Sq, int Skv, int D, int causal, float scale, const void* ws,
                         long long ws_bytes, long long (*need)(int, int, int, int, int, int)) {
  return attn_dims_ok(B, H, Hkv, Sq, Skv, D) && H % Hkv == 0 && scale > 0.f && !(causal && Sq > Skv) &&
         ws != nullptr && ((uintptr_t)ws & 255) == 0 && ws_bytes >= need(B, H, Hkv, Sq, Skv, D);
}

}  // namespace
